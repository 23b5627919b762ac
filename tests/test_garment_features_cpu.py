"""CPU tests of the FEATURE cache (GarmentCache.features): a cache that holds GarmentNet's features F [n * G * N_f][C_f] in place of the
K / V^T that TryonNet's attn1.to_k / to_v make of them -- its sizes, the container primitives, the packed form, the file format, the
refusals, and TryonEngine._cached_fill on a CPU engine: which table class and entry point each kind of feature cache selects, and that
after every block the staging list and the sets hold what _fill_set gives on the K / V^T cache a stand-in projection makes of the same
features.  No GPU: launches are recorded and interpreted on host memory (tests/garment_support.py's interpreter)."""
import ctypes as C
import json
import types

import pytest
import torch

from tests.garment_support import BLOCKS, DTYPE, FEATS, GINDEX, K, META, N_T, ORDERS, P, PACKED, Event, apply_records, same_features, standin_unet



def _features(G, seed, feats=FEATS):
    from idm_vton_amd.garment_cache import GarmentCache
    g = torch.Generator().manual_seed(seed)
    return GarmentCache(G=G, kv=[(torch.randn(N_T * G * N, Cc, generator=g).to(DTYPE),) for N, Cc in feats], features=True, **META)


def _native(G, seed):
    from idm_vton_amd.garment_cache import GarmentCache
    g = torch.Generator().manual_seed(seed)
    return GarmentCache(G=G, kv=[(torch.randn(N_T * G * N, Cc, generator=g).to(DTYPE), torch.randn(N_T * G, Cc, N, generator=g).to(DTYPE)) for N, Cc in FEATS], **META)


# ---- sizes -------------------------------------------------------------------------------------------------------------------------------
def test_nbytes_is_half_the_native_cache_and_a_quarter_packed():
    """The SDXL topology as tests/test_garment_size_cpu.py counts it: 10 features of 640 channels at level 1, 60 of 1280 at level 2, rows
    round16 of the level's tokens.  F is one tensor where the native cache has two of the same element count."""
    from idm_vton_amd.garment_cache import GarmentCache, PackedGarmentCache
    from idm_vton_amd.ops import round16
    half = lambda v: (v + 1) // 2
    for (gh, gw), native in (((128, 96), 9_437_184_000), ((64, 48), 2_359_296_000)):
        N1, N2 = round16(half(gh) * half(gw)), round16(half(half(gh)) * half(half(gw)))
        assert (10 * N1 * 640 + 60 * N2 * 1280) * 2 * 2 * 30 == native
        meta = dict(G=1, timesteps=range(30), h=gh, w=gw, dtype=torch.bfloat16, attn_fp8=False, f8_exp=(2, 2, 2), weights_id="w")
        e = lambda *sh, d=torch.bfloat16: torch.empty(*sh, dtype=d, device="meta")
        nat = GarmentCache(kv=[(e(30 * N1, 640), e(30, 640, N1))] * 10 + [(e(30 * N2, 1280), e(30, 1280, N2))] * 60, **meta)
        fc = GarmentCache(kv=[(e(30 * N1, 640),)] * 10 + [(e(30 * N2, 1280),)] * 60, features=True, **meta)
        assert nat.nbytes == native and 2 * fc.nbytes == nat.nbytes
        pk = PackedGarmentCache(kv=[(e(30 * N1, 640, d=torch.uint8),)] * 10 + [(e(30 * N2, 1280, d=torch.uint8),)] * 60, features=True,
                                exps=torch.empty(1, 70, 1, dtype=torch.int32, device="meta"), **meta)
        assert pk.nbytes == native // 4 + 4 * 1 * 70
        if (gh, gw) == (128, 96):
            assert fc.nbytes == 4_718_592_000 and pk.nbytes == 2_359_296_000 + 4 * 1 * 70


# ---- container operations -----------------------------------------------------------------------------------------------------------------
@PACKED
def test_select_cat_put_take_to_round_trips_are_bit_equal(packed):
    mk = (lambda G, s: _features(G, s).pack()) if packed else _features
    pool = mk(3, 1)
    ones = [pool.take(g) for g in range(3)]
    assert all(o.G == 1 and o.features and o.packed == packed for o in ones)
    assert sum(o.nbytes for o in ones) == pool.nbytes
    same_features(type(pool).cat(ones), pool)
    same_features(pool.select([0, 1, 2]), pool)
    sel = pool.select([2, 0, 2])
    same_features(sel.take(0), ones[2]); same_features(sel.take(1), ones[0]); same_features(sel.take(2), ones[2])
    other = mk(1, 7)
    before = [e[0].data_ptr() for e in pool.kv]
    assert pool.put(1, other) is pool and [e[0].data_ptr() for e in pool.kv] == before     # in place
    same_features(pool.take(1), other); same_features(pool.take(0), ones[0]); same_features(pool.take(2), ones[2])
    moved = pool.to("cpu", pin_memory=False)
    assert moved is pool
    d = pool.for_person_size(16, 16)
    assert d.features and (d.h, d.w) == (16, 16) and d.kv[0][0].data_ptr() == pool.kv[0][0].data_ptr()
    # the layout rule: entry i of F is rows [i * G * N_f, (i + 1) * G * N_f)
    (f0,), (f1,) = pool.run(1, 2)
    assert f0.shape == (2 * 3 * 32, 64) and f0.data_ptr() == pool.kv[0][0][3 * 32:].data_ptr() and f1.shape == (2 * 3 * 16, 128)
    rp = ones[0].repeat_garments(2)
    same_features(rp.take(0), ones[0]); same_features(rp.take(1), ones[0])


@PACKED
def test_save_load_round_trip_writes_version_4(tmp_path, packed):
    from safetensors import safe_open
    from idm_vton_amd.garment_cache import GarmentCache
    c = _features(2, 3).pack() if packed else _features(2, 3)
    path = str(tmp_path / "f.safetensors")
    c.save(path)
    with safe_open(path, framework="pt") as f:
        meta = {k: json.loads(v) for k, v in f.metadata().items()}
        assert meta["version"] == 4 and meta["kind"] == "features" and meta.get("packed", False) == packed
        assert sorted(f.keys()) == sorted(["f.000", "f.001"] + (["exps"] if packed else []))
    back = GarmentCache.load(path)
    same_features(back, c)


def test_a_version_3_file_still_loads(tmp_path):
    from safetensors import safe_open
    from idm_vton_amd.garment_cache import GarmentCache
    c = _native(2, 5).pack()
    path = str(tmp_path / "v3.safetensors")
    c.save(path)
    with safe_open(path, framework="pt") as f:
        assert json.loads(f.metadata()["version"]) == 3 and "kind" not in f.metadata()
    back = GarmentCache.load(path)
    assert back.packed and not back.features and torch.equal(back.exps, c.exps)
    assert all(torch.equal(a, b) for ea, eb in zip(back.kv, c.kv) for a, b in zip(ea, eb))
    plain = str(tmp_path / "v1.safetensors")
    _native(1, 6).save(plain)
    assert not GarmentCache.load(plain).features


def test_mixing_kinds_is_refused_by_name():
    from idm_vton_amd.garment_cache import GarmentCache, GarmentPool, GarmentShelf
    f, kv = _features(1, 1), _native(1, 1)
    for a, b in ((f, kv), (kv, f)):
        with pytest.raises(ValueError, match="features"):
            GarmentCache.cat([a, b])
        with pytest.raises(ValueError, match="features"):
            a.put(0, b)
    with pytest.raises(ValueError, match="features"):
        f.pack().put(0, kv)                               # (a 16-bit K / V^T garment is packed first -- and is still K / V^T)
    with pytest.raises(ValueError, match="packed"):
        f.put(0, f.pack())
    # the one exception, today's rule: a 16-bit feature garment put into a packed feature pool is packed first
    pool, g = _features(2, 2).pack(), _features(1, 9)
    pool.put(1, g)
    same_features(pool.take(1), g.pack())
    # out of scope, each refused by name: slotted caches, mixed-size pools, shelves
    with pytest.raises(ValueError, match="features"):
        GarmentCache(G=1, kv=f.kv, features=True, sizes=[(8, 4)], **META)
    slotted = GarmentCache(G=1, kv=kv.kv, sizes=[(8, 4)], **META)
    with pytest.raises(ValueError, match="features"):
        slotted.put(0, f)
    with pytest.raises(ValueError, match="features"):
        GarmentPool(2, like=f, mixed_sizes=True)
    with pytest.raises(ValueError, match="features"):
        GarmentShelf(kv).add("a", f)
    with pytest.raises(ValueError, match="features"):
        GarmentCache(G=1, kv=f.kv, features=True, **dict(META, attn_fp8=True))


@PACKED
@pytest.mark.parametrize("resident", ["device", "host"])
def test_garment_pool_takes_a_feature_cache_as_like(packed, resident):
    from idm_vton_amd.garment_cache import GarmentPool
    mk = (lambda s: _features(1, s).pack()) if packed else (lambda s: _features(1, s))
    made = {key: mk(ord(key)) for key in "abcd"}
    pool = GarmentPool(2, like=made["a"], spill=resident == "device", resident=resident)
    assert pool.cache.features and pool.cache.packed == packed and pool.cache.G == 2 and pool.cache.nbytes == 2 * made["a"].nbytes
    assert pool.get(["a", "b", "a"], encode=made.__getitem__) == [0, 1, 0]
    assert pool.get(["c", "b"], encode=made.__getitem__) == [0, 1]         # a, the least recently used, leaves (device: spilled to the host)
    same_features(pool.cache.take(0), made["c"]); same_features(pool.cache.take(1), made["b"])
    if resident == "device":
        assert list(pool.host) == ["a"] and pool.host["a"].features
        same_features(pool.host["a"], made["a"])
        assert pool.get(["a", "c"]) == [1, 0] and pool.stats["restored"] == 1          # comes back without `encode`
        same_features(pool.cache.take(1), made["a"])


# ---- pack / unpack ------------------------------------------------------------------------------------------------------------------------
def test_pack_and_unpack_are_the_formats_own_functions():
    from idm_vton_amd.garment_cache import pack_exponent, pack_values, unpack_values
    G = 3
    c = _features(G, 11)
    c.kv[0][0].view(N_T, G, -1)[:, 1] *= 40.0             # garments with different exponents
    c.kv[1][0].view(N_T, G, -1)[:, 2] *= 2.0 ** -9
    p = c.pack()
    assert p.features and p.packed and tuple(p.exps.shape) == (G, len(FEATS), 1) and p.exps.dtype == torch.int32
    assert len({int(e) for e in p.exps.view(-1)}) > 1
    assert p.nbytes == c.nbytes // 2 + 4 * G * len(FEATS)
    u = p.unpack()
    assert u.features and not u.packed and u.nbytes == c.nbytes
    for f, ((x,), (b,), (y,)) in enumerate(zip(c.kv, p.kv, u.kv)):
        xg = x.view(N_T, G, -1)
        e = pack_exponent(xg.abs().amax(dim=(0, 2)).float())
        assert torch.equal(e, p.exps[:, f, 0])
        want_b = pack_values(xg, e.view(1, G, 1))
        assert b.dtype == torch.uint8 and torch.equal(b.view(N_T, G, -1), want_b)
        assert y.dtype == DTYPE and torch.equal(y.view(N_T, G, -1), unpack_values(want_b, e.view(1, G, 1), DTYPE))
    again = u.pack()                                        # idempotent on unpacked values
    same_features(again, p)
    same_features(again.unpack(), u)
    with pytest.raises(ValueError, match="already"):
        p.pack()


# ---- _cached_fill on a CPU engine -----------------------------------------------------------------------------------------------------------
#         packed  transport resident  table class      entry point
CASES = [(False, "kernel", "device", None, None),
         (True, "kernel", "device", "KvUnpackTable", "kv_unpack"),
         (False, "kernel", "host", "KvStreamTable", "kv_stream"),
         (True, "kernel", "host", "KvStreamTable", "kv_stream"),
         (False, "copy", "host", "KvPlaceTable", "kv_place"),
         (True, "copy", "host", "KvPlaceTable", "kv_place")]


@pytest.mark.parametrize("indexed", [True, False], ids=["index", "noindex"])
@pytest.mark.parametrize("order", list(ORDERS), ids=list(ORDERS))
@pytest.mark.parametrize("packed,transport,resident,table,entry", CASES, ids=[f"{'packed' if c[0] else '16bit'}-{c[2]}-{c[1]}" for c in CASES])
def test_cached_fill_stages_the_features_and_projects_them(monkeypatch, packed, transport, resident, table, entry, order, indexed):
    """tests/test_garment_fill_cpu.py's grid on a feature cache: two features, n = 4, k = 3, blocks (1, 2, 1) alternating between two
    sets, G = 3; with garment_index [2, 2, 0] (P = 3 slots, U = 2 garments into slots 0, 1) and without (3 slots, all garments).  The
    reference is the K / V^T cache the stand-in projection makes of the same feature values per cache entry, put into reference sets by
    _fill_set.  After every block: the staging rows the block fills equal the feature values _fill_set's gather names; the sets' slots
    that a person reads equal the reference sets' bit for bit; slots nobody fills are whatever the projection made of the staging filler
    (unread: not compared).  One projection per block, over exactly c * S batch elements."""
    from idm_vton_amd import ops
    from idm_vton_amd.garment_cache import GarmentCache, slot_run
    from idm_vton_amd.pipeline import TryonEngine
    ffi = ops.ffi
    G = 3
    cache = _features(G, 1)
    if packed:
        cache = cache.pack()
        cache.exps.copy_(torch.arange(cache.exps.numel(), dtype=torch.int32).view_as(cache.exps) % 7 - 2)
    values = cache.unpack() if packed else cache           # the 16-bit features a call on `cache` projects
    if resident == "device":
        monkeypatch.setattr(GarmentCache, "host_resident", property(lambda self: False))
    made, launches, calls = [], [], []
    monkeypatch.setattr(ops, "stream_address", lambda t: t.data_ptr())
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "PROFILE", None)
    monkeypatch.setattr(torch.cuda, "Event", Event)
    for name in ("KvUnpackTable", "KvStreamTable", "KvFillTable", "KvPlaceTable"):
        cls = getattr(ops, name)
        monkeypatch.setattr(ops, name, type(name, (cls,), {"__init__": lambda self, *a, _c=cls, _n=name, **kw: (made.append(_n), _c.__init__(self, *a, **kw))[1]}))
    records = lambda at, n: torch.tensor((C.c_int64 * (5 * n)).from_address(at)[:]).view(n, 5)

    def launched(name, a, desc):
        launches.append((name, getattr(a, "workgroups", None)))
        apply_records(records(desc, a.n), packed, DTYPE)
    monkeypatch.setattr(ffi, "call_kv_unpack", lambda a, desc, stream: launched("kv_unpack", a, desc))
    for name in ("kv_stream", "kv_fill", "kv_place"):
        monkeypatch.setattr(ffi, "call_" + name, lambda a, desc, first, stream, name=name: launched(name, a, desc))

    eng, ref_eng = [TryonEngine(standin_unet(calls if i == 0 else []), None, None, dtype=DTYPE, device="cpu") for i in range(2)]
    gindex = GINDEX if indexed else None
    S = P if indexed else G
    st = dict(B=P, h=8, w=4, gh=8, gw=4, k=K, steps_noise=None, gcache=cache, gidx=ORDERS[order], gindex=gindex, blocks=BLOCKS, host_transport=transport)
    # the K / V^T cache of the same features: the stand-in applied per cache entry (its rows do not depend on the batch: plain matmul rows)
    ref_kv = ref_eng.unet.project_garment_kv([f.view(N_T * G, N, Cc) for (f,), (N, Cc) in zip(values.kv, FEATS)])
    ref = GarmentCache(G=G, kv=ref_kv, **META)
    slots, shapes = eng._cache_set_shapes(st)
    assert (slots, shapes) == ref_eng._cache_set_shapes(dict(st, gcache=ref)) and slots == S     # the sets keep the K / V^T cache's shapes
    got, want = [[eng._alloc_set((), shapes, N_T, K, slots) for _ in range(2)] for _ in range(2)]
    for t in (t for fs in got + want for kvf in fs["kv"] for t in kvf):
        t.view(torch.uint8).fill_(0x7f)
    garment = eng._cached_fill(st, got)
    assert made == ([table] if table else [])
    assert [[tuple(f.shape) for f in fs["feats"]] for fs in got] == [[(K * S, N, Cc) for N, Cc in FEATS]] * 2       # a live set's feats shapes
    for fs in got:
        for f in fs["feats"]:
            f.zero_()                                       # (finite filler for the slots nobody fills)
    used = list(dict.fromkeys(GINDEX)) if indexed else list(range(G))
    direct = 0                                              # blocks projected from the cache's own views: 16-bit on the device, consecutive, no index
    for bi, (s0, c) in enumerate(BLOCKS):
        p = bi & 1
        idx = ORDERS[order][s0:s0 + c]
        fast = not packed and resident == "device" and not indexed and idx == list(range(idx[0], idx[0] + c))
        direct += fast
        garment(bi, p)
        ref_eng._fill_set(dict(st, gcache=ref), want[p], s0, c)
        assert calls[-1] == [(c * S, N, Cc) for N, Cc in FEATS] and len(calls) == bi + 1
        for j in range(c):
            i = ORDERS[order][s0 + j]
            if not fast:                                    # the staging list: garment u of timestep slot j is the cache's (entry i, garment g)
                stage = [(f.view(-1, f.shape[-1]),) for f in got[p]["feats"]]
                for u, g in enumerate(used):
                    for (d,), (s,) in zip(slot_run(stage, K, S, j, u), slot_run(values.kv, N_T, G, i, g)):
                        assert torch.equal(d, s), (bi, j, u)
            for u in range(len(used)):
                for (gk, gv), (wk, wv) in zip(slot_run(got[p]["kv"], K, S, j, u), slot_run(want[p]["kv"], K, S, j, u)):
                    assert torch.equal(gk.view(torch.uint8), wk.view(torch.uint8)) and torch.equal(gv.view(torch.uint8), wv.view(torch.uint8)), (bi, j, u)
    wg = {None: None, "kv_unpack": None, "kv_place": 0}.get(entry, ops.KV_STREAM_WORKGROUPS)
    assert launches == ([(entry, wg)] * len(BLOCKS) if entry else [])
    counters = dict(garment_projections=3, garment_batches=0, garment_stream_launches=3 if (resident, transport) == ("host", "kernel") else 0,
                    garment_stage_launches=3 if transport == "copy" else 0,
                    garment_set_copies=0 if resident == "host" else 3 - direct)
    assert {name: eng.stats[name] for name in counters} == counters
    assert [h[0] for h in eng._streaming] == ([cache] if resident == "host" else [])


def test_an_attn_fp8_engine_refuses_feature_caches_before_anything_else():
    from idm_vton_amd.pipeline import TryonEngine
    eng = TryonEngine(types.SimpleNamespace(attn_fp8=True, f8_exp=(2, 2, 2)), None, None, dtype=DTYPE, device="cpu")
    for storage in ("features", "features-e4m3"):
        with pytest.raises(ValueError, match="attn_fp8"):
            eng.encode_garment(cloth=None, text_embeds_cloth=None, noise_cloth=None, num_inference_steps=3, storage=storage)
    with pytest.raises(ValueError, match="attn_fp8"):
        eng.project_garment(_features(1, 1))
    with pytest.raises(ValueError, match="attn_fp8"):
        eng.prepare(image=None, mask_image=None, pose_img=None, cloth=_features(1, 1), prompt_embeds=None, negative_prompt_embeds=None,
                    pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, text_embeds_cloth=None, noise={}, num_inference_steps=3,
                    guidance_scale=2.0)
    with pytest.raises(ValueError, match="storage"):
        eng.encode_garment(cloth=None, text_embeds_cloth=None, noise_cloth=None, num_inference_steps=3, storage="feature")
