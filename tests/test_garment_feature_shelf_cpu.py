"""CPU tests of the FEATURE SHELF: a GarmentShelf of storage "features" / "features-e4m3" keeps every garment as a compact feature cache (F
[n * N'_f][C_f] in place of K / V^T) and hands out a ShelvedGarmentCache with `features` true.  The container (sizes, LRU, refusals), the
records kv_records makes of compact feature parts -- a data run and, exactly where a garment has fewer rows than the slot, a zero ROW run
behind it -- and TryonEngine._cached_fill on a CPU engine: after every block the staging list holds each part's F in front of its slot and
the bits 0x0000 behind, and the sets hold what _fill_set gives on the K / V^T cache a stand-in projection makes of the zero-padded features.
No GPU: launches are recorded and interpreted on host memory (tests/garment_support.py's interpreter)."""
import ctypes as C
import types

import pytest
import torch

from tests.garment_support import BLOCKS, DTYPE, GINDEX, K, META, N_T, ORDERS, P, PACKED, Event, apply_records, record_fields, same_features, standin_unet

SLOT = [(48, 64), (16, 128)]                             # (N_f, C_f) of the slot's two features
# per garment: its own latent size and rows per timestep of the two features -- smaller, smallest, the slot's size
KINDS = {"a": ((8, 4), (32, 16)), "b": ((4, 4), (16, 16)), "c": ((12, 4), (48, 16))}
SLOT_HW = (12, 4)
TRANSPORTS = pytest.mark.parametrize("transport", ["kernel", "copy"])


def _meta(kind):
    (gh, gw), _ = KINDS[kind]
    return dict(META, gh=gh, gw=gw)


def _feat(kind, seed=0, **kw):
    """A G = 1 feature cache at the compact size of KINDS[kind]: F [n * N'_f][C_f] per feature."""
    from idm_vton_amd.garment_cache import GarmentCache
    g = torch.Generator().manual_seed(100 * seed + ord(kind))
    kv = [(torch.randn(N_T * N, Cc, generator=g).to(DTYPE),) for N, (_, Cc) in zip(KINDS[kind][1], SLOT)]
    return GarmentCache(**{**dict(G=1, kv=kv, features=True, **_meta(kind)), **kw})


def _kv(kind, seed=0):
    """The K / V^T cache of the same compact size: K [n * N'_f][C_f], V^T [n][C_f][N'_f]."""
    from idm_vton_amd.garment_cache import GarmentCache
    g = torch.Generator().manual_seed(100 * seed + ord(kind))
    kv = [(torch.randn(N_T * N, Cc, generator=g).to(DTYPE), torch.randn(N_T, Cc, N, generator=g).to(DTYPE)) for N, (_, Cc) in zip(KINDS[kind][1], SLOT)]
    return GarmentCache(G=1, kv=kv, **_meta(kind))


def _like_features():
    return _feat("c", seed=9)


def _like_slotted():
    """What TryonEngine.empty_garment_cache gives: one uninitialised K / V^T slot with `sizes`."""
    from idm_vton_amd.garment_cache import GarmentCache
    kv = [(torch.empty(N_T * N, Cc, dtype=DTYPE), torch.empty(N_T, Cc, N, dtype=DTYPE)) for N, Cc in SLOT]
    return GarmentCache(G=1, kv=kv, sizes=[SLOT_HW], **dict(META, gh=SLOT_HW[0], gw=SLOT_HW[1]))


def _shelf(packed, like=None, **kw):
    from idm_vton_amd.garment_cache import GarmentShelf
    shelf = GarmentShelf(_like_features() if like is None else like, storage="features-e4m3" if packed else "features", **kw)
    for kind in "abc":
        shelf.add(kind, _feat(kind))
    return shelf


def _values(part):
    """The 16-bit F a call on `part` stages: the part's own, or what the format says its bytes widen to."""
    return part.unpack() if part.packed else part


# ------------------------------------------------------------------------------------------------------------------ container
@PACKED
def test_feature_shelf_sizes_add_get_lru_and_eviction(packed):
    from idm_vton_amd.garment_cache import GarmentShelf, PackedGarmentCache, ShelvedGarmentCache
    for like in (_like_features(), _like_slotted(), _kv("c")):            # the slot's F shape is the slot's K shape, or F's own
        assert GarmentShelf(like, storage="features").slot_shapes == [((N, Cc), (Cc, N)) for N, Cc in SLOT]
    assert GarmentShelf(_like_features(), storage="native").slot_shapes == [((N, Cc), (Cc, N)) for N, Cc in SLOT]
    shelf = _shelf(packed, like=_like_slotted())
    assert shelf.features and len(shelf) == 3 and shelf.keys() == ["a", "b", "c"] and (shelf.gh, shelf.gw) == SLOT_HW
    kv_shelf = GarmentShelf(_like_slotted(), storage="e4m3" if packed else "native")
    for kind in "abc":
        kv_shelf.add(kind, _kv(kind))
    for kind in "abc":                                   # compact, and exactly half the compact K / V^T part -- packed: a quarter + 4 B per feature
        part, kv_part = shelf._parts[kind], kv_shelf._parts[kind]
        own = sum(N_T * N * Cc for N, (_, Cc) in zip(KINDS[kind][1], SLOT))
        assert part.features and part.G == 1 and isinstance(part, PackedGarmentCache) == packed
        if packed:
            assert part.nbytes == own + 4 * len(SLOT) and 4 * (part.nbytes - 4 * len(SLOT)) == 2 * own * 2
            assert 2 * (part.nbytes - 4 * len(SLOT)) == kv_part.nbytes - 4 * 2 * len(SLOT)
            assert tuple(part.exps.shape) == (1, len(SLOT), 1)
        else:
            assert part.nbytes == 2 * own and 2 * part.nbytes == kv_part.nbytes
    assert shelf.nbytes == sum(p.nbytes for p in shelf._parts.values()) < 3 * shelf._parts["c"].nbytes
    cache, index = shelf.get(["b", "a", "b"])
    assert isinstance(cache, ShelvedGarmentCache) and cache.features and index == [0, 1, 0] and cache.G == 2 and cache.sizes == [(4, 4), (8, 4)]
    assert cache.packed == packed and cache.host_resident and cache.kv == [] and (cache.gh, cache.gw) == SLOT_HW
    assert cache.slot_shapes == [((N, Cc), (Cc, N)) for N, Cc in SLOT]
    assert cache.nbytes == shelf._parts["a"].nbytes + shelf._parts["b"].nbytes
    assert shelf.keys() == ["c", "b", "a"] and shelf.stats == dict(hits=2, encoded=0, restored=0, evicted=0)
    assert "features" in repr(cache) and "ShelvedGarmentCache(G=2" in repr(cache) and ("e4m3-packed" in repr(cache)) == packed
    calls = []
    enc = lambda key: (calls.append(key), _feat("a", seed=ord(key)))[1]
    with pytest.raises(KeyError, match="'x' is not on the shelf"):
        shelf.get(["a", "x"])
    _, index2 = shelf.get(["x", "c", "x", "y"], encode=enc)
    assert calls == ["x", "y"] and index2 == [0, 1, 0, 2] and shelf.keys() == ["b", "a", "x", "c", "y"] and shelf.stats["encoded"] == 2
    # max_bytes: the least recently used garments the batch does not name go until the shelf fits
    big = shelf._parts["c"].nbytes
    small = _shelf(packed, max_bytes=2 * big + 100)
    kept, _ = small.get(["a"])                               # a + b + c exceed the bound: b, the least recently used, goes
    assert small.keys() == ["c", "a"] and small.stats["evicted"] == 1
    _, idx = small.get(["d", "b"], encode=lambda key: _feat("b", seed=7))
    assert idx == [0, 1] and small.keys() == ["a", "d", "b"] and small.stats["evicted"] == 2 and small.nbytes <= small.max_bytes
    with pytest.raises(ValueError, match="the batch alone holds"):
        small.get(["f", "g", "h"], encode=lambda key: _feat("c", seed=9))
    part = kept.parts[0]
    small.remove("a")
    assert "a" not in small and kept.parts[0] is part


def test_a_16bit_feature_garment_is_packed_on_its_way_in():
    from idm_vton_amd.garment_cache import GarmentShelf
    shelf = GarmentShelf(_like_features(), storage="features-e4m3")
    shelf.add("a", _feat("a"))
    shelf.add("a2", _feat("a").pack())
    same_features(shelf._parts["a"], _feat("a").pack())
    same_features(shelf._parts["a2"], shelf._parts["a"])
    plain = GarmentShelf(_like_features(), storage="features")
    plain.add("a", _feat("a"))
    same_features(plain._parts["a"], _feat("a"))
    assert plain._parts["a"].kv[0][0].data_ptr() != _feat("a").kv[0][0].data_ptr()


@PACKED
def test_shelved_feature_cache_methods(packed):
    shelf = _shelf(packed)
    cache, _ = shelf.get(["a", "b", "c"])
    kw = dict(timesteps=META["timesteps"][1:3], h=8, w=4, dtype=DTYPE, attn_fp8=False, f8_exp=(2, 2, 2), weights_id="w0")
    assert cache.check(persons=4, garment_index=[2, 0, 2, 1], **kw) == ([1, 2], [2, 0, 2, 1])
    assert cache.garment_sizes([2, 0]) == [(12, 4), (8, 4)]
    other = cache.for_person_size(32, 24)
    assert other.features and (other.h, other.w) == (32, 24) and other.parts == cache.parts and other.sizes == cache.sizes
    for g, key in enumerate("abc"):
        t = cache.take(g)
        assert t.G == 1 and t.features and t.packed == packed and (t.gh, t.gw) == KINDS[key][0]
        assert t.kv[0][0].data_ptr() != cache.parts[g].kv[0][0].data_ptr()
        same_features(t, cache.parts[g])
    sel = cache.select([2, 0, 2])
    assert sel.features and sel.G == 3 and sel.sizes == [(12, 4), (8, 4), (12, 4)] and sel.parts[0] is cache.parts[2] and sel.parts[2] is cache.parts[2]
    assert sel.nbytes == 2 * cache.parts[2].nbytes + cache.parts[0].nbytes
    with pytest.raises(ValueError, match="ShelvedGarmentCache slotted: features"):
        cache.slotted()
    for name, args in (("put", (0, _feat("a"))), ("pack", ()), ("unpack", ()), ("run", (0,)), ("to", ("cpu",))):
        with pytest.raises(ValueError, match=f"ShelvedGarmentCache {name}:"):
            getattr(cache, name)(*args)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_feature_shelf_refusals_name_their_field_before_any_launch(monkeypatch):
    from idm_vton_amd import ops
    from idm_vton_amd.garment_cache import GarmentCache, GarmentShelf, ShelvedGarmentCache
    from idm_vton_amd.pipeline import TryonEngine
    launches = []
    for name in ("kv_unpack", "kv_stream", "kv_fill", "kv_place"):
        monkeypatch.setattr(ops.ffi, "call_" + name, lambda *a, name=name: launches.append(name))
    with pytest.raises(ValueError, match="storage='feature'"):
        GarmentShelf(_like_features(), storage="feature")
    shelf, packed_shelf = GarmentShelf(_like_features(), storage="features"), GarmentShelf(_like_features(), storage="features-e4m3")
    for s in (shelf, packed_shelf):                      # kinds do not mix, in both directions
        with pytest.raises(ValueError, match="GarmentShelf add: features mismatch"):
            s.add("x", _kv("a"))
    for storage in ("native", "e4m3"):
        with pytest.raises(ValueError, match="GarmentShelf add: features mismatch"):
            GarmentShelf(_like_slotted(), storage=storage).add("x", _feat("a"))
    with pytest.raises(ValueError, match="GarmentShelf add: packed mismatch"):
        shelf.add("x", _feat("a").pack())
    with pytest.raises(ValueError, match="GarmentShelf add: G mismatch"):
        shelf.add("x", GarmentCache.cat([_feat("a"), _feat("a")]))
    for field, kw in (("timesteps", dict(timesteps=[900, 700, 500, 100])), ("h", dict(h=32)), ("weights_id", dict(weights_id="w1")),
                      ("dtype", dict(dtype=torch.bfloat16))):
        with pytest.raises(ValueError, match=f"GarmentShelf add: {field} mismatch"):
            shelf.add("x", _feat("a", **kw))
    tall = _feat("c")                                    # more rows than the slot holds
    tall.kv[0] = (torch.zeros(N_T * 64, 64, dtype=DTYPE),)
    with pytest.raises(ValueError, match=r"does not fit \(feature 0: .*F rows 64 x 64.*holds 48 x 64"):
        shelf.add("x", tall)
    wide = _feat("a")                                    # another C_f
    wide.kv[1] = (torch.zeros(N_T * 16, 64, dtype=DTYPE),)
    with pytest.raises(ValueError, match=r"does not fit \(feature 1: .*F rows 16 x 64.*holds 16 x 128"):
        shelf.add("x", wide)
    two = _feat("a")
    two.kv = two.kv[:1]
    with pytest.raises(ValueError, match=r"does not fit \(1 features against 2\)"):
        shelf.add("x", two)
    assert len(shelf) == 0 and shelf.nbytes == 0 and len(packed_shelf) == 0
    # mixed parts: kinds, and 16-bit with packed
    shapes = shelf.slot_shapes
    with pytest.raises(ValueError, match="ShelvedGarmentCache: features mismatch"):
        ShelvedGarmentCache([_feat("a"), _kv("b")], gh=12, gw=4, slot_shapes=shapes)
    with pytest.raises(ValueError, match="all packed or all 16-bit"):
        ShelvedGarmentCache([_feat("a"), _feat("b").pack()], gh=12, gw=4, slot_shapes=shapes)
    # the pinned constructor refusal: features and sizes never meet on a tensor list
    with pytest.raises(ValueError, match="features"):
        GarmentCache(G=1, kv=_feat("a").kv, features=True, sizes=[(8, 4)], **_meta("a"))
    # the engine: an attn_fp8 engine, a pageable part, slotted()
    good = ShelvedGarmentCache([_feat("a"), _feat("c")], gh=12, gw=4, slot_shapes=shapes)
    assert good.features and not any(t.is_pinned() for p in good.parts for e in p.kv for t in e)
    eng8 = TryonEngine(types.SimpleNamespace(attn_fp8=True, f8_exp=(2, 2, 2)), None, None, dtype=DTYPE, device="cpu")
    with pytest.raises(ValueError, match="attn_fp8"):
        eng8.prepare(image=None, mask_image=None, pose_img=None, cloth=good, garment_index=[0, 1], prompt_embeds=None, negative_prompt_embeds=None,
                     pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, text_embeds_cloth=None, noise={}, num_inference_steps=3,
                     guidance_scale=2.0)
    with pytest.raises(ValueError, match="attn_fp8 mismatch.*does not stream"):
        eng8._check_host_cache(good)
    with pytest.raises(ValueError, match="attn_fp8"):
        eng8.project_garment(good)
    eng = TryonEngine(types.SimpleNamespace(attn_fp8=False, f8_exp=(2, 2, 2)), None, None, dtype=DTYPE, device="cpu")
    with pytest.raises(ValueError, match="kv mismatch.*pageable.*pin_memory"):
        eng._check_host_cache(good)
    with pytest.raises(ValueError, match="slotted: features"):
        good.slotted()
    assert launches == [] and dict(eng.stats) == dict(TryonEngine(None, None, None, dtype=DTYPE, device="cpu").stats)


# ------------------------------------------------------------------------------------------------------------------ records
def _staging(k, S, fill=0x7f):
    dst = [(torch.empty(k * S * N, Cc, dtype=DTYPE),) for N, Cc in SLOT]
    for t, in dst:
        t.view(torch.uint8).fill_(fill)
    return dst


@PACKED
@pytest.mark.parametrize("garments", [[2, 0], [0, 1], [2]], ids=["c,a", "a,b", "c"])
def test_records_of_compact_feature_parts(packed, garments):
    """Per (timestep, garment, feature): a data run of the part's N'_f rows into the front of the slot and, exactly where N'_f < N_f, a zero
    run (src 0, exp 0) of the (N_f - N'_f) rows directly behind it.  Entries by value, in non-consecutive order."""
    from idm_vton_amd import ffi, ops
    from idm_vton_amd.garment_cache import shelf_records
    cache, _ = _shelf(packed).get(["a", "b", "c"])
    parts = [cache.parts[g] for g in garments]
    k, S, entries, tslots, gslots = 3, 3, [3, 1, 2], [0, 1, 2], list(range(len(garments)))
    dst = _staging(k, S)
    asked = []

    def address(t):
        asked.append(t.data_ptr())
        return t.data_ptr()
    rec, per = shelf_records(parts, packed, dst, k, S, entries, tslots, gslots, address=address)
    assert sorted(asked) == sorted([e[0].data_ptr() for p in parts for e in p.kv] + ([p.exps.data_ptr() for p in parts] if packed else []))
    su = 1 if packed else 2                              # source / column unit: bytes of e4m3, else byte units of the 16-bit copy form
    want = []
    for i, j in zip(entries, tslots):
        step = []
        for part, u in zip(parts, gslots):
            for f, ((src,), (d,), (N, Cc)) in enumerate(zip(part.kv, dst, SLOT)):
                Nf = src.shape[0] // N_T
                at = d.data_ptr() + (j * S + u) * N * Cc * 2
                step.append((src.data_ptr() + i * Nf * Cc * su, at, part.exps.data_ptr() + 4 * f if packed else 0, Nf, Cc * su, Cc * su, Cc * su))
                if Nf < N:
                    step.append((0, at + Nf * Cc * 2, 0, N - Nf, Cc * su, Cc * su, Cc * su))
        if len(step) % 2:
            step.append(min(step, key=lambda r: r[3] * (r[4] // 16)))
        want += step
    got = record_fields(rec)
    assert [r[:5] + r[6:] for r in got] == [r[:5] + r[6:] for r in want]                     # (lds of a zero run is not looked at)
    assert all(g[5] == w[5] for g, w in zip(got, want) if g[0])
    zero = [r for r in got if r[0] == 0]
    tails = sum(Nf < N for g in garments for Nf, (N, _) in zip(KINDS["abc"[g]][1], SLOT))
    raw = 2 * len(garments) + tails
    assert per == raw + raw % 2 and per % 2 == 0 and tuple(rec.shape) == (len(entries) * per, 5)
    assert all(r[2] == 0 for r in zero) and (len(zero) >= len(entries) * tails) and (not zero) == (garments == [2])
    table = ops.KvFillTable(rec, "cpu", ffi.KVS_WIDEN_E4M3 if packed else ffi.KVS_COPY, [(t * per, per) for t in range(len(entries))])
    items = [r[3] * (r[4] // 16) for r in got]
    assert table.items.tolist() == items
    assert table.first_host[:per + 1].tolist() == [sum((it + 1023) // 1024 for it in items[:m]) for m in range(per + 1)]
    # the bytes a timestep loads are the compact parts' own (the pad record here is a zero run, the smallest)
    assert table.link_bytes(0, per) == sum(p.nbytes - (p.exps.numel() * 4 if packed else 0) for p in parts) / N_T
    apply_records(rec, packed, DTYPE)
    for i, j in zip(entries, tslots):
        for u in range(S):
            for f, ((d,), (N, Cc)) in enumerate(zip(dst, SLOT)):
                slot = d[(j * S + u) * N:(j * S + u + 1) * N]
                if u >= len(garments):                   # a slot no garment of the call fills: untouched
                    assert (slot.view(torch.uint8) == 0x7f).all()
                    continue
                v = _values(parts[u]).kv[f][0]
                Nf = v.shape[0] // N_T
                assert torch.equal(slot[:Nf].view(torch.int16), v[i * Nf:(i + 1) * Nf].view(torch.int16)), (i, u, f)
                assert (slot[Nf:].view(torch.int16) == 0).all(), (i, u, f)


@PACKED
def test_staged_plan_serves_feature_parts(packed):
    """The copy transport as data: the arena holds the compact parts' own bytes for k timesteps, copies are per part tensor, the place
    records carry the zero-row runs."""
    from idm_vton_amd.garment_cache import staged_plan
    cache, _ = _shelf(packed).get(["a", "b", "c"])
    k, S = 3, 3
    dsts = [_staging(k, S), _staging(k, S)]
    plan = staged_plan(cache, GINDEX, k, S, dsts, "cpu")
    used = [cache.parts[g] for g in dict.fromkeys(GINDEX)]                                   # c, then a
    own = sum(p.nbytes - (p.exps.numel() * 4 if packed else 0) for p in used)
    assert plan["nbytes"] == own // N_T * k and plan["arena"].dtype == torch.uint8
    assert (plan["exps"] is not None) == packed and len(plan["exps_copies"]) == (len(used) if packed else 0)
    if packed:
        assert tuple(plan["exps"].shape) == (len(used), len(SLOT), 1)
    assert len(plan["copies"]([1, 2])) == len(used) * len(SLOT) and len(plan["copies"]([3, 1])) == 2 * len(used) * len(SLOT)
    got = record_fields(plan["rec"])
    per = plan["per"]
    assert per == 6 and len(got) == 2 * k * per                                              # 2 + 3 records per timestep, padded
    zero = [r for r in got if r[0] == 0]
    assert len(zero) == 2 * k * 2 and all(r[2] == 0 and r[3] == 16 for r in zero)            # a's 16-row tail of feature 0 (and the pad: the same run)
    lo, hi = plan["arena"].data_ptr(), plan["arena"].data_ptr() + plan["nbytes"]
    assert all(lo <= r[0] < hi for r in got if r[0])                                         # every data run reads the arena


# ------------------------------------------------------------------------------------------------------------------ _cached_fill
@pytest.mark.parametrize("order", list(ORDERS), ids=list(ORDERS))
@TRANSPORTS
@PACKED
def test_cached_fill_stages_compact_features_with_zero_rows_and_projects_them(monkeypatch, packed, transport, order):
    """n = 4, k = 3, blocks (1, 2, 1) alternating between two sets, three garments (32, 16), (16, 16), (48, 16) rows in slots of (48, 16),
    garment_index [2, 2, 0]: U = 2 garments into slots 0, 1 of 3-slot staging lists.  Staging lists and sets start as 0x7f bytes.  After
    every block: each used staging slot holds the part's F rows in front and the bits 0x0000 behind; the sets equal, bit for bit, what
    _fill_set gives on the K / V^T cache the stand-in projection makes of the zero-padded features.  One launch and one projection per block."""
    from idm_vton_amd import ops
    from idm_vton_amd.garment_cache import GarmentCache, slot_run
    from idm_vton_amd.pipeline import TryonEngine
    ffi = ops.ffi
    cache, _ = _shelf(packed).get(["a", "b", "c"])
    if packed:
        for g, part in enumerate(cache.parts):
            part.exps.copy_(torch.arange(part.exps.numel(), dtype=torch.int32).view_as(part.exps) % 5 - 2 + g)
    made, tables, launches, calls = [], [], [], []
    monkeypatch.setattr(ops, "stream_address", lambda t: t.data_ptr())
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "PROFILE", None)
    monkeypatch.setattr(torch.cuda, "Event", Event)
    for name in ("KvUnpackTable", "KvStreamTable", "KvFillTable", "KvPlaceTable"):
        cls = getattr(ops, name)
        monkeypatch.setattr(ops, name, type(name, (cls,), {"__init__": lambda self, *a, _c=cls, _n=name, **kw: (made.append(_n), tables.append(self),
                                                                                                                  _c.__init__(self, *a, **kw))[2]}))
    records = lambda at, n: torch.tensor((C.c_int64 * (5 * n)).from_address(at)[:]).view(n, 5)

    def launched(name, a, desc):
        launches.append((name, getattr(a, "workgroups", None)))
        apply_records(records(desc, a.n), packed, DTYPE)
    monkeypatch.setattr(ffi, "call_kv_unpack", lambda a, desc, stream: launched("kv_unpack", a, desc))
    for name in ("kv_stream", "kv_fill", "kv_place"):
        monkeypatch.setattr(ffi, "call_" + name, lambda a, desc, first, stream, name=name: launched(name, a, desc))

    eng, ref_eng = [TryonEngine(standin_unet(calls if i == 0 else []), None, None, dtype=DTYPE, device="cpu") for i in range(2)]
    S, G = P, cache.G
    st = dict(B=P, h=8, w=4, gh=SLOT_HW[0], gw=SLOT_HW[1], k=K, steps_noise=None, gcache=cache, gidx=ORDERS[order], gindex=GINDEX, blocks=BLOCKS,
              host_transport=transport)
    # the reference: every garment's F zero-padded to the slot's rows, projected per cache entry by the stand-in -> a slot-sized K / V^T cache
    padded = []
    for f, (N, Cc) in enumerate(SLOT):
        t = torch.zeros(N_T, G, N, Cc, dtype=DTYPE)
        for g, part in enumerate(cache.parts):
            v = _values(part).kv[f][0]
            t[:, g, :v.shape[0] // N_T] = v.view(N_T, -1, Cc)
        padded.append(t.view(N_T * G, N, Cc))
    ref = GarmentCache(G=G, kv=ref_eng.unet.project_garment_kv(padded), **dict(META, gh=SLOT_HW[0], gw=SLOT_HW[1]))
    slots, shapes = eng._cache_set_shapes(st)
    assert slots == S and shapes == [((N_T * S * N, Cc), (N_T * S, Cc, N), DTYPE) for N, Cc in SLOT]   # from slot_shapes: the cache has no kv
    got, want = [[eng._alloc_set((), shapes, N_T, K, slots) for _ in range(2)] for _ in range(2)]
    for t in (t for fs in got + want for kvf in fs["kv"] for t in kvf):
        t.view(torch.uint8).fill_(0x7f)
    garment = eng._cached_fill(st, got)
    table = "KvFillTable" if transport == "kernel" else "KvPlaceTable"
    assert made == [table]
    assert [[tuple(f.shape) for f in fs["feats"]] for fs in got] == [[(K * S, N, Cc) for N, Cc in SLOT]] * 2
    for fs in got:
        for f in fs["feats"]:
            f.view(torch.uint8).fill_(0x7f)
    used = list(dict.fromkeys(GINDEX))
    own_bytes = sum(cache.parts[g].nbytes - (cache.parts[g].exps.numel() * 4 if packed else 0) for g in used) // N_T     # per timestep
    for bi, (s0, c) in enumerate(BLOCKS):
        p = bi & 1
        garment(bi, p)
        ref_eng._fill_set(dict(st, gcache=ref), want[p], s0, c)
        assert calls[-1] == [(c * S, N, Cc) for N, Cc in SLOT] and len(calls) == bi + 1
        stage = [(f.view(-1, f.shape[-1]),) for f in got[p]["feats"]]
        for j in range(c):
            i = ORDERS[order][s0 + j]
            for u, g in enumerate(used):
                v = _values(cache.parts[g])
                for f, ((d,), (s,)) in enumerate(zip(slot_run(stage, K, S, j, u), timestep_run_one(v, i))):
                    Nf = s.shape[0]
                    assert torch.equal(d[:Nf].view(torch.int16), s.view(torch.int16)), (bi, j, u, f)
                    assert (d[Nf:].view(torch.int16) == 0).all(), (bi, j, u, f)
                for (gk, gv), (wk, wv) in zip(slot_run(got[p]["kv"], K, S, j, u), slot_run(want[p]["kv"], K, S, j, u)):
                    assert torch.equal(gk.view(torch.int16), wk.view(torch.int16)) and torch.equal(gv.view(torch.int16), wv.view(torch.int16)), (bi, j, u)
            for f, ((d,), (N, _)) in enumerate(zip(slot_run(stage, K, S, j, len(used)), SLOT)):      # the slot nobody fills: untouched
                assert (d.view(torch.uint8) == 0x7f).all()
    # the V^T tail behind garment a's 32 keys is zero, as a K / V^T shelf's fill would have written it
    assert (slot_run(got[0]["kv"], K, S, 0, 1)[0][1][..., 32:] == 0).all() and (slot_run(got[0]["kv"], K, S, 0, 1)[0][0][32:] == 0).all()
    entry, wg = ("kv_fill", ops.KV_STREAM_WORKGROUPS) if transport == "kernel" else ("kv_place", 0)
    assert launches == [(entry, wg)] * len(BLOCKS)
    t = tables[0]
    for which, (f0, cnt) in enumerate(t.slices):         # what a block loads is the compact parts' own bytes of its timesteps
        assert t.link_bytes(f0, cnt) == own_bytes * (cnt // 6), which
    copies = len(used) * len(SLOT) * (3 if order == "consecutive" else 4)                     # per part tensor and run of consecutive entries
    counters = dict(garment_projections=3, garment_batches=0, garment_set_copies=0, garment_stream_launches=3 if transport == "kernel" else 0,
                    garment_stage_launches=3 if transport == "copy" else 0, garment_stage_copies=copies if transport == "copy" else 0)
    assert {name: eng.stats[name] for name in counters} == counters
    assert [h[0] for h in eng._streaming] == [cache]


def timestep_run_one(cache, i):
    from idm_vton_amd.garment_cache import timestep_run
    return timestep_run(cache.kv, N_T, 1, i)
