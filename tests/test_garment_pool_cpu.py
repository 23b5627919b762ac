"""CPU tests of the garment pool: GarmentCache's pool primitives (select / cat / put / to / save / load / check with a garment_index) and
GarmentPool's LRU map on CPU tensors (no kernels), and the two indexed attention entry points: exported, validating on the host (no launch),
with the C ABI where it was."""
import ctypes as C

import pytest
import torch

from tests.garment_support import POOL_FEATS, TABLE, ask, attn_args, attn_f8_args, caches_equal, pool_cache


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_indexed_entry_points_are_exported_and_the_abi_did_not_move():
    from idm_vton_amd import ffi
    L = ffi.lib()
    for s in ("idmvton_attn_fwd_indexed", "idmvton_attn_f8_indexed"):
        assert s in ffi.SYMBOLS and hasattr(L, s), s
    assert L.idmvton_abi_version() == 9 == ffi.ABI_VERSION
    assert L.idmvton_sizeof(b"idmvton_attn_args") == 144 == C.sizeof(ffi.AttnArgs)
    assert L.idmvton_sizeof(b"idmvton_attn_f8_args") == 128 == C.sizeof(ffi.AttnF8Args)


@pytest.mark.parametrize("fn,make", [("idmvton_attn_fwd_indexed", lambda **kw: attn_args(0, **kw)), ("idmvton_attn_f8_indexed", attn_f8_args)],
                         ids=["attn_fwd_indexed", "attn_f8_indexed"])
def test_indexed_arguments_are_validated_on_the_host(fn, make):
    from idm_vton_amd import ffi
    L = ffi.lib()
    nb, ix = (C.c_int32 * 2)(0, 1), (C.c_void_p * 2)(None, TABLE)
    assert getattr(L, fn)(None, nb, ix, None) == -5 and b"null args" in L.idmvton_last_error()        # NULL args: an error code, no device
    assert getattr(L, fn)(None, None, None, None) == -5
    assert getattr(L, fn)(C.byref(make()), None, ix, None) == -5 and b"null seg_nb / seg_index" in L.idmvton_last_error()
    assert getattr(L, fn)(C.byref(make()), nb, None, None) == -5 and b"null seg_nb / seg_index" in L.idmvton_last_error()
    with pytest.raises(RuntimeError, match=r"seg 1 has a table: needs seg_nb >= 1 \(0\)"):
        ffi.call_indexed(fn, make(), (0, 0), (0, TABLE), 0)
    with pytest.raises(RuntimeError, match=r"seg 1 has a table: needs seg_nb >= 1 \(-2\)"):
        ffi.call_indexed(fn, make(), (0, -2), (0, TABLE), 0)
    with pytest.raises(RuntimeError, match=r"seg_b0 < B \(4, 4\)"):                  # no conditional batch: a table of no entries
        ffi.call_indexed(fn, make(b0=4), (0, 1), (0, TABLE), 0)
    with pytest.raises(RuntimeError, match=r"table is not 4-byte aligned"):
        ffi.call_indexed(fn, make(), (0, 1), (0, TABLE + 2), 0)
    # a segment without a table keeps _shared's bound, also next to one that has a table
    with pytest.raises(RuntimeError, match=r"seg 0 seg_nb=5 outside \[0, B - seg_b0 = 4\]"):
        ffi.call_indexed(fn, make(), (5, 1), (0, TABLE), 0)
    with pytest.raises(RuntimeError, match=r"seg 1 seg_nb=3 outside \[0, B - seg_b0 = 2\]"):
        ffi.call_indexed(fn, make(), (0, 3), (0, 0), 0)


def test_cross_mode_takes_no_table():
    from idm_vton_amd import ffi
    with pytest.raises(RuntimeError, match=r"CROSS mode takes no table"):
        ffi.call_indexed("idmvton_attn_fwd_indexed", attn_args(ffi.ATTN_CROSS, b0=0), (0, 1), (0, TABLE), 0)
    with pytest.raises(RuntimeError, match=r"CROSS mode takes no table"):
        ffi.call_indexed("idmvton_attn_fwd_indexed", attn_args(ffi.ATTN_CROSS, b0=0), (1, 0), (TABLE, 0), 0)


def test_ops_segment_dicts_without_an_index_keep_their_entry_points():
    from idm_vton_amd import ops
    assert ops._seg_index([dict(nk=4), dict(nk=4, b0=2, nb=2)], 4) is None
    assert ops._seg_index([dict(nk=4), dict(nk=4, b0=2, nb=2, index=None)], 4) is None
    with pytest.raises(ValueError, match="int32 device tensor of B - b0 = 2 entries"):
        ops._seg_index([dict(nk=4), dict(nk=4, b0=2, nb=2, index=torch.zeros(2, dtype=torch.int32))], 4)       # a host tensor


# ------------------------------------------------------------------------------------------------------------------ GarmentCache


def _garment(c, i, g):
    """[(K rows, V^T element)] of garment g at timestep entry i, cut by hand."""
    out = []
    for k, vt in c.step(i):
        N = k.shape[0] // c.G
        out.append((k[g * N:(g + 1) * N], vt[g]))
    return out


def _same_garment(a, b):
    return all(torch.equal(ka, kb) and torch.equal(va, vb) for (ka, va), (kb, vb) in zip(a, b))


def test_select_gathers_garments_in_the_order_asked():
    c = pool_cache(G=3)
    ids = [2, 0, 2, 1]
    s = c.select(ids)
    assert s.G == 4 and s.timesteps == c.timesteps and s.nbytes == c.nbytes // 3 * 4
    for i in range(len(c.timesteps)):
        for j, g in enumerate(ids):
            assert _same_garment(_garment(s, i, j), _garment(c, i, g)), (i, j, g)
    assert all(ks.data_ptr() != kc.data_ptr() for (ks, _), (kc, _) in zip(s.kv, c.kv))     # a copy
    assert caches_equal(c.select([0, 1, 2, 0, 1, 2]), c.repeat_garments(2))                      # what the modulo rule reads, materialised
    assert caches_equal(c.select([0, 1, 2]), c)
    with pytest.raises(ValueError, match="GarmentCache garment_index mismatch"):
        c.select([0, 3])


def test_cat_joins_caches_and_names_the_field_that_differs():
    from idm_vton_amd.garment_cache import GarmentCache
    a, b, c = pool_cache(G=1, seed=1), pool_cache(G=2, seed=2), pool_cache(G=1, seed=3)
    j = GarmentCache.cat([a, b, c])
    assert j.G == 4 and j.nbytes == a.nbytes + b.nbytes + c.nbytes
    for i in range(len(a.timesteps)):
        for slot, (src, g) in enumerate([(a, 0), (b, 0), (b, 1), (c, 0)]):
            assert _same_garment(_garment(j, i, slot), _garment(src, i, g)), (i, slot)
    assert caches_equal(GarmentCache.cat([b.select([0]), b.select([1])]), b)
    for field, other in (("timesteps", pool_cache(G=1, ts=(900, 700, 500, 300, 99))), ("h", pool_cache(G=1, h=6, w=2)), ("dtype", pool_cache(G=1, dtype=torch.bfloat16)),
                         ("attn_fp8", pool_cache(G=1, attn_fp8=True)), ("f8_exp", pool_cache(G=1, f8_exp=(2, 3, 2))), ("weights_id", pool_cache(G=1, wid="w1")),
                         ("gh", a.for_person_size(4, 3)._like(gh=2, gw=6))):
        with pytest.raises(ValueError, match=f"GarmentCache cat: {field} mismatch"):
            GarmentCache.cat([a, other])
    with pytest.raises(ValueError, match="GarmentCache cat: kv mismatch"):
        GarmentCache.cat([a, a._like(kv=a.kv[:1])])
    with pytest.raises(ValueError, match="no caches"):
        GarmentCache.cat([])


@pytest.mark.parametrize("dtype", [torch.float16, torch.uint8], ids=["f16", "e4m3_bytes"])
def test_put_overwrites_exactly_one_slot_of_every_tensor_at_every_timestep(dtype):
    c, one = pool_cache(G=3, dtype=dtype, seed=4), pool_cache(G=1, dtype=dtype, seed=5)
    before = c.select([0, 1, 2])
    ptrs = [(k.data_ptr(), vt.data_ptr()) for k, vt in c.kv]
    assert c.put(1, one) is c
    assert ptrs == [(k.data_ptr(), vt.data_ptr()) for k, vt in c.kv]                       # in place: the tensors did not move
    for i in range(len(c.timesteps)):
        assert _same_garment(_garment(c, i, 1), _garment(one, i, 0)), i
        for g in (0, 2):
            assert _same_garment(_garment(c, i, g), _garment(before, i, g)), (i, g)
    assert not caches_equal(c, before)
    # element for element: everything outside slot 1 is what it was
    for (k, vt), (k0, vt0) in zip(c.kv, before.kv):
        n, N = len(c.timesteps), k.shape[0] // (len(c.timesteps) * 3)
        keep = torch.ones(n, 3, dtype=torch.bool)
        keep[:, 1] = False
        assert torch.equal(k.view(n, 3, N, -1)[keep], k0.view(n, 3, N, -1)[keep]) and torch.equal(vt.view(n, 3, *vt.shape[1:])[keep], vt0.view(n, 3, *vt.shape[1:])[keep])
    with pytest.raises(ValueError, match="put: slot mismatch"):
        c.put(3, one)
    with pytest.raises(ValueError, match="put: G mismatch"):
        c.put(0, before)
    with pytest.raises(ValueError, match="put: weights_id mismatch"):
        c.put(0, pool_cache(G=1, dtype=dtype, wid="w1"))
    with pytest.raises(ValueError, match="put: kv mismatch"):
        c.put(0, pool_cache(G=1, dtype=torch.uint8 if dtype != torch.uint8 else torch.float16))


def test_take_copies_one_slot_out_and_put_brings_it_back():
    c = pool_cache(G=3, seed=6)
    one = c.take(2)
    assert one.G == 1 and one.timesteps == c.timesteps and one.nbytes == c.nbytes // 3
    assert all(_same_garment(_garment(one, i, 0), _garment(c, i, 2)) for i in range(len(c.timesteps)))
    assert all(k1.data_ptr() != k.data_ptr() for (k1, _), (k, _) in zip(one.kv, c.kv))     # a copy
    assert caches_equal(one, c.select([2])) and caches_equal(c.take(0, "cpu"), c.select([0]))
    d = pool_cache(G=3, seed=7)
    d.put(0, one)
    assert all(_same_garment(_garment(d, i, 0), _garment(c, i, 2)) for i in range(len(c.timesteps)))
    with pytest.raises(ValueError, match="take: slot mismatch"):
        c.take(3)


def test_to_cpu_keeps_the_cache():
    c = pool_cache(G=2)
    assert c.to("cpu") is c                                                                # nothing to move
    d = c.to(torch.device("cpu"))
    assert caches_equal(c, d)


@pytest.mark.parametrize("dtype,fp8", [(torch.float16, False), (torch.bfloat16, False), (torch.uint8, True)], ids=["f16", "bf16", "e4m3_bytes"])
def test_save_load_round_trip_is_bit_equal_with_all_metadata(tmp_path, dtype, fp8):
    import json
    from safetensors import safe_open
    from idm_vton_amd.garment_cache import GarmentCache
    c = pool_cache(G=2, dtype=dtype, attn_fp8=fp8, f8_exp=(1, 2, 3), wid="abc:def", h=4, w=3)._like(gh=2, gw=6)
    path = str(tmp_path / "garments.safetensors")
    c.save(path)
    d = GarmentCache.load(path)
    assert caches_equal(c, d) and (d.gh, d.gw) == (2, 6) and {k.dtype for k, _ in d.kv} == {dtype}
    with safe_open(path, framework="pt") as f:
        meta = {k: json.loads(v) for k, v in f.metadata().items()}
    assert meta == dict(format="idmvton_garment_cache", version=1, G=2, timesteps=list(c.timesteps), h=4, w=3, gh=2, gw=6, dtype=str(c.dtype),
                        attn_fp8=fp8, f8_exp=[1, 2, 3], weights_id="abc:def", features=2)
    ask = dict(timesteps=c.timesteps, h=4, w=3, dtype=c.dtype, attn_fp8=fp8, f8_exp=(1, 2, 3), weights_id="abc:def", persons=2)
    assert d.check(**ask) == [0, 1, 2, 3, 4]                                               # the engine that made it takes it
    for field, over in (("weights", dict(weights_id="abc:xyz")), ("dtype", dict(dtype=torch.float32)), ("attn_fp8", dict(attn_fp8=not fp8))):
        with pytest.raises(ValueError, match=f"GarmentCache {field} mismatch"):            # any other engine: the existing messages
            d.check(**{**ask, **over})
    # a file whose weights_id was edited is refused by the engine the original was made on
    from safetensors.torch import load_file, save_file
    meta["weights_id"] = "abc:edited"
    path2 = str(tmp_path / "edited.safetensors")
    save_file(load_file(path), path2, metadata={k: json.dumps(v) for k, v in meta.items()})
    with pytest.raises(ValueError, match="GarmentCache weights mismatch"):
        GarmentCache.load(path2).check(**ask)
    save_file(load_file(path), path2, metadata={"format": json.dumps("something else")})
    with pytest.raises(ValueError, match="not a garment cache of format version 1"):
        GarmentCache.load(path2)


def test_check_with_a_garment_index_replaces_the_modulo_rule():
    c = pool_cache(G=3)
    with pytest.raises(ValueError, match="GarmentCache persons mismatch"):
        ask(c, persons=4)                                                                 # without an index: P % G, as ever
    # with an index: (cache entries, the validated index as ints) -- what the engine needs
    assert ask(c, persons=4, garment_index=[2, 0, 2, 1]) == ([0, 1, 2, 3, 4], [2, 0, 2, 1])
    assert ask(c, persons=1, garment_index=(2,)) == ([0, 1, 2, 3, 4], [2])
    assert ask(c, persons=2, garment_index=torch.tensor([1, 1]), timesteps=[300, 900]) == ([3, 0], [1, 1])
    assert ask(c, persons=3) == [0, 1, 2, 3, 4]                                           # without: the entries alone, as ever
    assert c.garment_ids(torch.tensor([1, 2], dtype=torch.int32), 2) == [1, 2]
    for bad, persons, what in (([0, 1, 2], 4, "3 entries for P = 4 persons"), ([0, 1, 2, 0, 1], 4, "5 entries for P = 4"), ([0, 3, 1, 1], 4, r"\[3\] outside \[0, G = 3\)"),
                               ([0, -1], 2, r"\[-1\] outside"), ([], 0, "0 entries for P = 0"), (7, 1, "expected a sequence"), (["a"], 1, "expected a sequence")):
        with pytest.raises(ValueError, match=f"GarmentCache garment_index mismatch: .*{what}"):
            ask(c, persons=persons, garment_index=bad)
    # the other fields are held as before, index or not
    with pytest.raises(ValueError, match="GarmentCache weights mismatch"):
        ask(c, persons=4, garment_index=[2, 0, 2, 1], weights_id="w1")
    with pytest.raises(ValueError, match="GarmentCache timesteps mismatch"):
        ask(c, persons=4, garment_index=[2, 0, 2, 1], timesteps=[901])


def test_slot_run_and_index_runs_follow_the_layout_rule():
    from idm_vton_amd.garment_cache import index_runs, slot_run
    c = pool_cache(G=3)
    n = len(c.timesteps)
    for i in (0, 3):
        two = slot_run(c.kv, n, 3, i, 1, 2)
        for f, (k, vt) in enumerate(two):
            N = POOL_FEATS[f][0]
            assert torch.equal(k[:N], _garment(c, i, 1)[f][0]) and torch.equal(k[N:], _garment(c, i, 2)[f][0])
            assert torch.equal(vt[0], _garment(c, i, 1)[f][1]) and torch.equal(vt[1], _garment(c, i, 2)[f][1])
            assert k.data_ptr() == _garment(c, i, 1)[f][0].data_ptr()                      # views
    assert index_runs([3, 4, 5, 0, 1]) == [(0, 3, 3), (3, 0, 2)]
    assert index_runs([2, 0, 1]) == [(0, 2, 1), (1, 0, 2)]
    assert index_runs([0, 1, 2, 3]) == [(0, 0, 4)] and index_runs([5]) == [(0, 5, 1)] and index_runs([]) == []


# ------------------------------------------------------------------------------------------------------------------ GarmentPool
def _pool(capacity, spill=False):
    from idm_vton_amd.garment_cache import GarmentPool
    made = []
    garments = {}

    def encode(key):
        made.append(key)
        garments.setdefault(key, pool_cache(G=1, seed=100 + key))
        return garments[key]
    pool = GarmentPool(capacity, like=pool_cache(G=1, seed=99), spill=spill)
    return pool, encode, made, lambda key: pool_cache(G=1, seed=100 + key)


def _holds(pool, slot, one):
    return all(_same_garment(_garment(pool.cache, i, slot), _garment(one, i, 0)) for i in range(len(one.timesteps)))


def test_pool_returns_the_index_of_a_batch_and_evicts_the_least_recently_used():
    pool, encode, made, truth = _pool(3)
    assert pool.cache.G == 3 and pool.cache.timesteps == truth(0).timesteps
    idx = pool.get([7, 7, 3, 9], encode)
    assert idx == [0, 0, 1, 2] and made == [7, 3, 9]                                       # one encode per distinct garment, free slots in order
    assert all(_holds(pool, s, truth(k)) for k, s in pool.slots().items())
    assert pool.get([3, 7], encode) == [1, 0] and made == [7, 3, 9]                        # hits: nothing encoded
    assert list(pool.slots()) == [9, 3, 7]                                                 # use order: 9 is now the oldest
    assert pool.get([5], encode) == [2] and made[-1] == 5 and 9 not in pool                # ... and it is 9's slot that goes
    assert list(pool.slots()) == [3, 7, 5]
    assert pool.get([4, 3], encode) == [0, 1] and 7 not in pool                            # 3 is older than 7 but the batch needs it: 7 goes
    assert all(_holds(pool, s, truth(k)) for k, s in pool.slots().items())
    assert pool.stats == dict(hits=3, encoded=5, restored=0, evicted=2)
    ptr = pool.cache.kv[0][0].data_ptr()
    pool.get([1, 2, 6], encode)                                                            # a batch that replaces everything
    assert sorted(pool.slots()) == [1, 2, 6] and pool.cache.kv[0][0].data_ptr() == ptr     # the pool's tensors never move
    assert pool.cache.check(timesteps=truth(0).timesteps, h=4, w=3, dtype=torch.float16, attn_fp8=False, f8_exp=(2, 2, 2), weights_id="w0",
                            persons=3, garment_index=pool.get([6, 1, 2], encode))[0] == [0, 1, 2, 3, 4]


def test_pool_never_evicts_a_slot_the_batch_uses():
    pool, encode, made, truth = _pool(2)
    pool.get([1, 2], encode)
    idx = pool.get([2, 3], encode)                                                         # 1 is the only garment the batch does not name
    assert idx == [1, 0] and 1 not in pool and _holds(pool, 1, truth(2)) and _holds(pool, 0, truth(3))
    idx = pool.get([4, 3], encode)                                                         # 2 is older than 3, and it is 2 that may go
    assert idx == [1, 0] and _holds(pool, 0, truth(3)) and _holds(pool, 1, truth(4))
    with pytest.raises(ValueError, match="3 distinct garments, the pool has capacity 2"):
        pool.get([1, 2, 3], encode)
    assert pool.get([4, 4, 4, 3], encode) == [1, 1, 1, 0]                                  # repeats are one garment
    with pytest.raises(KeyError, match="not resident and no `encode`"):
        pool.get([8])


def test_pool_spills_to_the_host_and_restores_without_encoding():
    pool, encode, made, truth = _pool(2, spill=True)
    pool.get([1, 2], encode)
    pool.get([3], encode)                                                                  # evicts 1 -> host
    assert 1 not in pool and list(pool.host) == [1] and caches_equal(pool.host[1], truth(1))
    n = len(made)
    assert pool.get([1], encode) == [1] and len(made) == n                                 # 2 was the oldest; 1 comes back from the host copy
    assert _holds(pool, 1, truth(1)) and pool.stats["restored"] == 1 and pool.stats["encoded"] == 3
    assert pool.get([1], None) == [1]
    pool.drop(2)
    assert list(pool.host) == [1]
    pool.drop(2)                                                                           # dropping what is not there is no error


def test_pool_bounds_its_host_copies_and_loses_no_slot_when_encode_fails():
    pool, encode, made, truth = _pool(1, spill=2)                                          # one slot, at most two garments on the host
    assert pool.host_capacity == 2
    for key in (1, 2, 3, 4):
        pool.get([key], encode)                                                            # each evicts its predecessor -> host
    assert list(pool.host) == [2, 3] and all(caches_equal(pool.host[k], truth(k)) for k in (2, 3))   # 1, spilled longest ago, was dropped
    n = len(made)
    assert pool.get([2], encode) == [0] and len(made) == n and _holds(pool, 0, truth(2))   # restored; 4 spilled, 3 stays, 2 is in use
    assert list(pool.host) == [2, 4]                                                       # 3 was the oldest copy not in use

    def failing(key):
        raise MemoryError("no room to encode")
    pool2, encode2, _, truth2 = _pool(2)
    pool2.get([1], encode2)
    with pytest.raises(MemoryError):
        pool2.get([9], failing)                                                            # a free slot was available: it still is
    assert pool2.slots() == {1: 0} and pool2.get([5], encode2) == [1]
    with pytest.raises(MemoryError):
        pool2.get([9], failing)                                                            # full pool: nothing is evicted for a garment that never came
    assert pool2.slots() == {1: 0, 5: 1} and _holds(pool2, 0, truth2(1)) and _holds(pool2, 1, truth2(5))
    assert pool2.get([6, 7], encode2) == [0, 1]                                            # the pool still has both its slots
    from idm_vton_amd.garment_cache import GarmentPool
    with pytest.raises(ValueError, match="must hold one garment"):
        GarmentPool(2, like=pool_cache(G=2))
    with pytest.raises(ValueError, match="capacity 0 < 1"):
        GarmentPool(0, like=pool_cache(G=1))


# ------------------------------------------------------------------------------------------------------------------ engine, host side
def test_fill_set_gathers_the_distinct_garments_of_a_call_into_person_sized_sets():
    """The graph forms' gather on CPU tensors (plain torch copies): U distinct garments in first-use order -> slots 0 .. U - 1 of every
    timestep slot of a P-slot set, the table maps persons to those slots, nothing beyond slot U - 1 is written, and the graph key of an
    indexed state carries P and not G."""
    from idm_vton_amd.garment_cache import kv_shapes, timestep_run
    from idm_vton_amd.pipeline import TryonEngine
    eng = TryonEngine(None, None, None, dtype=torch.float16, device="cpu")
    pool = pool_cache(G=6, seed=8)
    n, P, k = len(pool.timesteps), 4, 3
    gindex = [5, 2, 5, 3]                                                                  # U = 3: garments 5, 2, 3 -> slots 0, 1, 2
    st = dict(B=P, h=4, w=3, gh=4, gw=3, k=k, steps_noise=None, gcache=pool, gidx=[1, 2, 4], gindex=gindex)      # timesteps not consecutive
    assert eng._slot_table(st).tolist() == [0, 1, 0, 2] and eng._slot_table(st).dtype == torch.int32
    assert eng._slot_table(dict(st, gindex=None)) is None
    shapes = [((a[0] // pool.G * P,) + a[1:], (b[0] // pool.G * P,) + b[1:], d) for a, b, d in kv_shapes(pool.kv)]
    fset = eng._alloc_set((), shapes, n, k, P)
    for kk, vt in fset["kv"]:
        kk.fill_(-7.0); vt.fill_(-7.0)
    eng._fill_set(st, fset, 1, 2)                                                          # steps 1, 2 of the call = cache entries 2, 4 -> timestep slots 0, 1
    assert eng.stats["garment_set_copies"] == 1
    for j, i in enumerate([2, 4]):
        for f, (kk, vt) in enumerate(timestep_run(fset["kv"], k, P, j)):
            N = POOL_FEATS[f][0]
            assert tuple(vt.shape) == (P, POOL_FEATS[f][1], N) and tuple(kk.shape) == (P * N, POOL_FEATS[f][1])
            for slot, g in enumerate([5, 2, 3]):
                gk, gvt = _garment(pool, i, g)[f]
                assert torch.equal(kk[slot * N:(slot + 1) * N], gk) and torch.equal(vt[slot], gvt), (j, f, slot)
            assert (kk[3 * N:] == -7.0).all() and (vt[3] == -7.0).all()                    # slot U = 3: never written, never indexed
    for kk, vt in timestep_run(fset["kv"], k, P, 2):                                       # the block had two timesteps: the third slot is untouched
        assert (kk == -7.0).all() and (vt == -7.0).all()
    # one state for every pool size and assignment; never the state of the call without an index, nor a live one
    key = TryonEngine._graph_key(st, False)
    assert key == TryonEngine._graph_key(dict(st, gcache=pool_cache(G=2), gindex=[0, 1, 1, 0]), False)
    assert key != TryonEngine._graph_key(dict(st, gindex=None), False) and key != TryonEngine._graph_key(st, True)
    assert key != TryonEngine._graph_key(dict(st, B=2, gindex=[5, 2]), False)
