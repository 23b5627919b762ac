"""TryonEngine._cached_fill on a CPU engine: for every kind of cache, the table class / entry point it selects and what the slice it launches
for (bi, p) does to set p -- interpreted on CPU tensors by tests/garment_support.py's interpreter -- against _fill_set on the 16-bit
cache that holds the same values.  No GPU: ops.stream_address is data_ptr, launches are recorded and interpreted instead of made."""
import ctypes as C

import pytest
import torch

from tests.garment_support import BLOCKS, DTYPE, FEATS, GINDEX, K, N_T, ORDERS, P, Event, apply_records

SMALL = [(16, 64), (16, 128)]                            # a compact garment: half the K rows / V^T positions of feature 0, so ONE zero tail

#         kind     packed  transport resident  table class      entry point
CASES = [("plain", False, "kernel", "device", None, None),
         ("plain", True, "kernel", "device", "KvUnpackTable", "kv_unpack"),
         ("plain", False, "kernel", "host", "KvStreamTable", "kv_stream"),
         ("plain", True, "kernel", "host", "KvStreamTable", "kv_stream"),
         ("shelf", False, "kernel", "host", "KvFillTable", "kv_fill"),
         ("shelf", True, "kernel", "host", "KvFillTable", "kv_fill"),
         ("plain", False, "copy", "host", "KvPlaceTable", "kv_place"),
         ("plain", True, "copy", "host", "KvPlaceTable", "kv_place"),
         ("shelf", False, "copy", "host", "KvPlaceTable", "kv_place"),
         ("shelf", True, "copy", "host", "KvPlaceTable", "kv_place")]


def _garments(feats, G, seed):
    from idm_vton_amd.garment_cache import GarmentCache
    g = torch.Generator().manual_seed(seed)
    kv = [(torch.randn(N_T * G * N, Cc, generator=g).to(DTYPE), torch.randn(N_T * G, Cc, N, generator=g).to(DTYPE)) for N, Cc in feats]
    return GarmentCache(G=G, timesteps=list(range(900, 900 - 200 * N_T, -200)), h=8, w=4, gh=8 if feats is FEATS else 4, gw=4, dtype=DTYPE, attn_fp8=False,
                        f8_exp=(2, 2, 2), weights_id="w0", kv=kv)


def _source(kind, packed):
    """-> (the cache a call is made on, the 16-bit cache of the same values that _fill_set reads, per garment the K rows it fills per feature)."""
    from idm_vton_amd.garment_cache import GarmentShelf
    if kind == "plain":
        cache = _garments(FEATS, 3, 1)
        if packed:
            cache = cache.pack()
            cache.exps.copy_(torch.arange(cache.exps.numel(), dtype=torch.int32).view_as(cache.exps) % 7 - 2)    # distinct per (garment, feature, K | V^T)
        return cache, cache.unpack() if packed else cache, [[N for N, _ in FEATS]] * 3
    shelf = GarmentShelf(_garments(FEATS, 1, 0), storage="e4m3" if packed else "native")
    for key, feats in (("a", SMALL), ("b", SMALL), ("c", FEATS)):    # [2, 2, 0]: the slot-sized c, then a with its one tail -- 4 + 5 records per
        shelf.add(key, _garments(feats, 1, ord(key)))                # timestep, an odd count that is padded to 10
    cache, index = shelf.get(["a", "b", "c"])
    assert index == [0, 1, 2]
    return cache, cache.slotted("cpu"), [[N for N, _ in f] for f in (SMALL, SMALL, FEATS)]


@pytest.mark.parametrize("order", list(ORDERS), ids=list(ORDERS))
@pytest.mark.parametrize("kind,packed,transport,resident,table,entry", CASES, ids=[f"{c[0]}-{'packed' if c[1] else '16bit'}-{c[3]}-{c[2]}" for c in CASES])
def test_cached_fill_selects_the_table_and_fills_the_sets_as_fill_set_does(monkeypatch, kind, packed, transport, resident, table, entry, order):
    """Two features, n = 4 cached timesteps, k = 3, blocks of 1, 2, 1 alternating between two 3-slot sets, G = 3, P = 3, garment_index
    [2, 2, 0]: U = 2 garments into slots 0, 1.  Sets start as 0x7f bytes; after every block both sets must equal, byte for byte, the sets that
    _fill_set fills from the 16-bit cache of the same values (unpack() of a packed cache, slotted("cpu") of a shelf) -- the slot nobody fills
    and the timestep slots behind a short block included.  One exception, which is the shelf's contract: a compact garment's K rows beyond
    its own N'_f are NOT written (no kernel reads them), so they must still be 0x7f where slotted() has zeros."""
    from idm_vton_amd import ops
    from idm_vton_amd.garment_cache import GarmentCache
    from idm_vton_amd.pipeline import TryonEngine
    ffi = ops.ffi
    cache, ref, own = _source(kind, packed)
    if resident == "device":                             # (CPU tensors stand in for device memory)
        monkeypatch.setattr(GarmentCache, "host_resident", property(lambda self: False))
    assert cache.host_resident == (resident == "host") and cache.packed == packed
    made, launches = [], []
    monkeypatch.setattr(ops, "stream_address", lambda t: t.data_ptr())
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "PROFILE", None)
    monkeypatch.setattr(torch.cuda, "Event", Event)
    for name in ("KvUnpackTable", "KvStreamTable", "KvFillTable", "KvPlaceTable"):
        cls = getattr(ops, name)
        monkeypatch.setattr(ops, name, type(name, (cls,), {"__init__": lambda self, *a, _c=cls, _n=name, **kw: (made.append(_n), _c.__init__(self, *a, **kw))[1]}))
    records = lambda at, n: torch.tensor((C.c_int64 * (5 * n)).from_address(at)[:]).view(n, 5)

    def launched(name, a, desc):                         # the launch, recorded and carried out on host memory
        launches.append((name, getattr(a, "workgroups", None)))
        apply_records(records(desc, a.n), packed, DTYPE)
    monkeypatch.setattr(ffi, "call_kv_unpack", lambda a, desc, stream: launched("kv_unpack", a, desc))
    for name in ("kv_stream", "kv_fill", "kv_place"):
        monkeypatch.setattr(ffi, "call_" + name, lambda a, desc, first, stream, name=name: launched(name, a, desc))

    eng, ref_eng = [TryonEngine(None, None, None, dtype=DTYPE, device="cpu") for _ in range(2)]
    st = dict(B=P, h=8, w=4, gh=8, gw=4, k=K, steps_noise=None, gcache=cache, gidx=ORDERS[order], gindex=GINDEX, blocks=BLOCKS, host_transport=transport)
    slots, shapes = eng._cache_set_shapes(st)
    assert slots == P
    got, want = [[eng._alloc_set((), shapes, N_T, K, slots) for _ in range(2)] for _ in range(2)]
    for t in (t for fs in got + want for kvf in fs["kv"] for t in kvf):
        assert t.dtype == DTYPE
        t.view(torch.uint8).fill_(0x7f)
    garment = eng._cached_fill(st, got)
    assert made == ([table] if table else [])
    # K rows (timestep slot, garment slot, row) that the call's garment of that slot does not fill
    beyond = []
    for f, (N, _) in enumerate(FEATS):
        m = torch.zeros(K, P, N, dtype=torch.bool)
        for u, g in enumerate(dict.fromkeys(GINDEX)):
            m[:, u, own[g][f]:] = True
        beyond.append(m.view(-1))
    assert any(m.any() for m in beyond) == (kind == "shelf")
    for bi in range(len(BLOCKS)):
        p = bi & 1
        garment(bi, p)
        ref_eng._fill_set(dict(st, gcache=ref), want[p], *BLOCKS[bi])
        for q in range(2):
            for f, ((gk, gv), (wk, wv)) in enumerate(zip(got[q]["kv"], want[q]["kv"])):
                assert torch.equal(gv.view(torch.uint8), wv.view(torch.uint8)), (bi, q, f)
                assert torch.equal(gk[~beyond[f]].view(torch.uint8), wk[~beyond[f]].view(torch.uint8)), (bi, q, f)
                assert (gk[beyond[f]].view(torch.uint8) == 0x7f).all(), (bi, q, f)
    assert not (got[0]["kv"][0][0][:32].view(torch.uint8) == 0x7f).all() and (got[0]["kv"][0][0][2 * 32:3 * 32].view(torch.uint8) == 0x7f).all()
    # one launch per block through the case's own entry point (the place kernel's grid is the table's: workgroups 0), and its counters alone
    wg = {None: None, "kv_unpack": None, "kv_place": 0}.get(entry, ops.KV_STREAM_WORKGROUPS)
    assert launches == ([(entry, wg)] * len(BLOCKS) if entry else [])
    staged_copies = {"plain": 32, "shelf": 24 if order == "consecutive" else 32}[kind]    # plain: per timestep and garment run; shelf: per part tensor and run of entries
    counters = dict(garment_set_copies=3 if resident == "device" else 0, garment_stream_launches=3 if (resident, transport) == ("host", "kernel") else 0,
                    garment_stage_launches=3 if transport == "copy" else 0, garment_stage_copies=staged_copies if transport == "copy" else 0)
    assert {name: eng.stats[name] for name in counters} == counters
    assert [h[0] for h in eng._streaming] == ([cache] if resident == "host" else [])     # a host-resident cache stays referenced behind its last fill
