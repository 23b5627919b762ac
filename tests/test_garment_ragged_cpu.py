"""CPU tests of mixed garment sizes in one pool: a GarmentCache with `sizes` (slots of one size, each garment at the front of its own) --
put / take / select / cat / save / load and GarmentPool(mixed_sizes=True) on CPU tensors, no kernels -- and the two ragged attention entry
points: exported, validating on the host (no launch), with the C ABI where it was."""
import ctypes as C
import functools

import pytest
import torch

from tests.garment_support import TABLE, attn_args, attn_f8_args, caches_equal

_equal = functools.partial(caches_equal, sizes=True)    # slotted caches: the slots' garment sizes are facts too


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_ragged_entry_points_are_exported_and_the_abi_did_not_move():
    from idm_vton_amd import ffi
    L = ffi.lib()
    for s in ("idmvton_attn_fwd_ragged", "idmvton_attn_f8_ragged"):
        assert s in ffi.SYMBOLS and hasattr(L, s), s
    assert L.idmvton_abi_version() == 9 == ffi.ABI_VERSION
    assert L.idmvton_sizeof(b"idmvton_attn_args") == 144 == C.sizeof(ffi.AttnArgs)
    assert L.idmvton_sizeof(b"idmvton_attn_f8_args") == 128 == C.sizeof(ffi.AttnF8Args)


@pytest.mark.parametrize("fn,make", [("idmvton_attn_fwd_ragged", lambda **kw: attn_args(0, **kw)), ("idmvton_attn_f8_ragged", attn_f8_args)],
                         ids=["attn_fwd_ragged", "attn_f8_ragged"])
def test_ragged_arguments_are_validated_on_the_host(fn, make):
    from idm_vton_amd import ffi
    L = ffi.lib()
    nb, ix, nk = (C.c_int32 * 2)(0, 1), (C.c_void_p * 2)(None, TABLE), (C.c_void_p * 2)(None, TABLE + 64)
    assert getattr(L, fn)(None, nb, ix, nk, None) == -5 and b"null args" in L.idmvton_last_error()    # NULL args: an error code, no device
    assert getattr(L, fn)(None, None, None, None, None) == -5
    assert getattr(L, fn)(C.byref(make()), nb, ix, None, None) == -5 and b"null seg_nb / seg_nk" in L.idmvton_last_error()
    assert getattr(L, fn)(C.byref(make()), None, ix, nk, None) == -5 and b"null seg_nb / seg_nk" in L.idmvton_last_error()
    with pytest.raises(RuntimeError, match=r"seg 1 key-count table is not 4-byte aligned"):
        ffi.call_ragged(fn, make(), (0, 1), (0, TABLE), (0, TABLE + 66), 0)
    with pytest.raises(RuntimeError, match=r"seg 0 key-count table is not 4-byte aligned"):     # without an index table, on the own-token segment
        ffi.call_ragged(fn, make(), (0, 0), None, (TABLE + 1, 0), 0)
    # the index table's rules hold next to a key-count table
    with pytest.raises(RuntimeError, match=r"seg 1 has a table: needs seg_nb >= 1 \(0\)"):
        ffi.call_ragged(fn, make(), (0, 0), (0, TABLE), (0, TABLE + 64), 0)
    with pytest.raises(RuntimeError, match=r"seg 1 seg_nb=3 outside \[0, B - seg_b0 = 2\]"):
        ffi.call_ragged(fn, make(), (0, 3), (0, 0), (0, TABLE + 64), 0)


def test_cross_mode_takes_no_key_count_table():
    from idm_vton_amd import ffi
    for nk in ((0, TABLE), (TABLE, 0)):
        with pytest.raises(RuntimeError, match=r"attn_fwd_ragged: CROSS mode takes no table"):
            ffi.call_ragged("idmvton_attn_fwd_ragged", attn_args(ffi.ATTN_CROSS, b0=0), (0, 0), None, nk, 0)


def test_ops_segment_dicts_without_a_key_count_table_keep_their_entry_points(monkeypatch):
    from idm_vton_amd import ffi, ops
    assert ops._seg_nk([dict(nk=4), dict(nk=4, b0=2, nb=2)], 4) is None
    assert ops._seg_nk([dict(nk=4), dict(nk=4, b0=2, nb=2, nk_table=None)], 4) is None
    with pytest.raises(ValueError, match="nk_table must be a contiguous int32 device tensor of B = 4 entries"):
        ops._seg_nk([dict(nk=4), dict(nk=4, b0=2, nk_table=torch.zeros(4, dtype=torch.int32))], 4)           # a host tensor
    # which entry point a launch goes through: the ragged one only with a table
    seen = []
    monkeypatch.setattr(ffi, "call", lambda fn, *a: seen.append(("call", fn)))
    monkeypatch.setattr(ffi, "call_shared", lambda fn, *a: seen.append(("call_shared", fn)))
    monkeypatch.setattr(ffi, "call_indexed", lambda fn, *a: seen.append(("call_indexed", fn)))
    monkeypatch.setattr(ffi, "call_ragged", lambda fn, *a: seen.append(("call_ragged", fn)))
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    ops._call("idmvton_attn_fwd", None)
    ops._call("idmvton_attn_fwd_shared", None, seg_nb=[0, 2])
    ops._call("idmvton_attn_fwd_indexed", None, seg_nb=[0, 2], seg_index=[0, TABLE])
    ops._call("idmvton_attn_fwd_ragged", None, seg_nb=[0, 2], seg_index=[0, TABLE], seg_nk=[0, TABLE])
    ops._call("idmvton_attn_fwd_ragged", None, seg_nb=[0, 0], seg_index=None, seg_nk=[0, TABLE])
    assert seen == [("call", "idmvton_attn_fwd"), ("call_shared", "idmvton_attn_fwd_shared"), ("call_indexed", "idmvton_attn_fwd_indexed"),
                    ("call_ragged", "idmvton_attn_fwd_ragged"), ("call_ragged", "idmvton_attn_fwd_ragged")]


# ------------------------------------------------------------------------------------------------------------------ GarmentCache
# (token rows, channels) of two features at three garment sizes (latent gh x gw): what an engine's feature_tokens / round16 would give them
SIZES = {(4, 4): ((16, 64), (16, 128)), (4, 3): ((16, 64), (16, 128)), (8, 6): ((48, 64), (16, 128)), (8, 8): ((64, 64), (16, 128))}
SLOT = (8, 8)
TS = (900, 700, 500, 300, 100)


def _cache(size, G=1, sizes=None, dtype=torch.float16, seed=0, ts=TS, wid="w0", fill=None):
    """A synthetic cache of garments of latent `size`; every (timestep, garment, feature) block has values of its own (a seeded draw, or
    the constant `fill`)."""
    from idm_vton_amd.garment_cache import GarmentCache
    n, kv = len(ts), []
    g = torch.Generator().manual_seed(seed)
    for N, Cc in SIZES[size]:
        if fill is None:
            k, vt = torch.randn(n * G * N, Cc, generator=g).to(dtype), torch.randn(n * G, Cc, N, generator=g).to(dtype)
        else:
            k, vt = torch.full((n * G * N, Cc), fill, dtype=dtype), torch.full((n * G, Cc, N), fill, dtype=dtype)
        kv.append((k, vt))
    return GarmentCache(G=G, timesteps=ts, h=8, w=8, gh=size[0], gw=size[1], dtype=dtype, attn_fp8=False, f8_exp=(2, 2, 2), weights_id=wid, kv=kv,
                        sizes=sizes)


def _slotted(G, fill=7.0):
    return _cache(SLOT, G=G, sizes=[SLOT] * G, fill=fill)


def _slot_views(c, i, g):
    """[(K rows, V^T element)] of slot g at timestep entry i, cut by hand."""
    out = []
    for k, vt in c.step(i):
        N = k.shape[0] // c.G
        out.append((k[g * N:(g + 1) * N], vt[g]))
    return out


def test_put_of_a_smaller_garment_fills_the_front_of_its_slot_and_zeroes_the_vt_tail():
    pool = _slotted(3)
    before = [(k.clone(), vt.clone()) for k, vt in pool.kv]
    ptrs = [(k.data_ptr(), vt.data_ptr()) for k, vt in pool.kv]
    one = _cache((8, 6), seed=5)
    assert pool.put(1, one) is pool
    assert pool.sizes == [SLOT, (8, 6), SLOT] and (pool.gh, pool.gw) == SLOT
    assert [(k.data_ptr(), vt.data_ptr()) for k, vt in pool.kv] == ptrs
    for i in range(len(TS)):
        for f, ((k, vt), (ok, ovt)) in enumerate(zip(_slot_views(pool, i, 1), one.step(i))):
            Nf, N = ok.shape[0], k.shape[0]
            assert torch.equal(k[:Nf], ok) and torch.equal(vt[:, :Nf], ovt[0])
            assert not vt[:, Nf:].any()                                        # the rest of the slot's V^T: zero
            assert (k[Nf:] == 7.0).all()                                       # the K tail keeps what it held
            assert (Nf < N) == (f == 0)                                        # (feature 0 is the one that is smaller than its slot here)
        for g in (0, 2):                                                       # every other slot element for element what it was
            for f, (k, vt) in enumerate(_slot_views(pool, i, g)):
                bk, bvt = before[f]
                N = k.shape[0]
                r = bk.shape[0] // len(TS)
                assert torch.equal(k, bk[i * r + g * N:i * r + (g + 1) * N]) and torch.equal(vt, bvt[i * 3 + g])


def test_take_returns_the_garment_at_its_own_compact_size_and_put_round_trips():
    pool = _slotted(2)
    one, full = _cache((4, 3), seed=3), _cache(SLOT, seed=4)
    pool.put(0, one)
    pool.put(1, full)
    back = pool.take(0)
    assert back.sizes is None and _equal(back, one) and back.nbytes == one.nbytes < full.nbytes
    assert _equal(pool.take(1), full)
    other = _slotted(2, fill=1.0)
    other.put(1, back)
    assert _equal(other.take(1), one)
    # a slot that shrinks: the new garment's zero tail covers what the larger one left
    pool.put(1, one)
    assert pool.sizes == [(4, 3), (4, 3)] and _equal(pool.take(1), one)
    for i in range(len(TS)):
        assert not _slot_views(pool, i, 1)[0][1][:, 16:].any()


def test_a_garment_that_does_not_fit_is_refused_with_nothing_written():
    from idm_vton_amd.garment_cache import GarmentCache
    small = _cache((8, 6), G=2, sizes=[(8, 6)] * 2, fill=7.0)
    before = [(k.clone(), vt.clone()) for k, vt in small.kv]
    with pytest.raises(ValueError, match=r"put: does not fit"):
        small.put(0, _cache(SLOT, seed=1))                                     # feature 0: 64 rows into 48
    wide = _cache((8, 6), seed=1)
    wide.kv[1] = (torch.zeros(len(TS) * 16, 64, dtype=torch.float16), torch.zeros(len(TS), 64, 16, dtype=torch.float16))    # another channel width
    with pytest.raises(ValueError, match=r"put: does not fit"):
        small.put(0, GarmentCache(G=1, timesteps=TS, h=8, w=8, gh=8, gw=6, dtype=torch.float16, attn_fp8=False, f8_exp=(2, 2, 2), weights_id="w0",
                                  kv=wide.kv))
    with pytest.raises(ValueError, match=r"put: weights_id mismatch"):         # every other field still has to agree
        small.put(0, _cache((4, 4), wid="w1"))
    with pytest.raises(ValueError, match=r"put: timesteps mismatch"):
        small.put(0, _cache((4, 4), ts=TS[:4]))
    with pytest.raises(ValueError, match=r"put: G mismatch"):
        small.put(0, _cache((4, 4), G=2))
    assert small.sizes == [(8, 6)] * 2
    assert all(torch.equal(k, bk) and torch.equal(vt, bvt) for (k, vt), (bk, bvt) in zip(small.kv, before))


def test_a_cache_without_sizes_refuses_another_size_with_the_message_it_had():
    plain = _cache(SLOT, G=2)
    assert plain.sizes is None
    with pytest.raises(ValueError, match=r"GarmentCache put: gh mismatch"):
        plain.put(0, _cache((4, 4)))
    with pytest.raises(ValueError, match=r"GarmentCache put: gw mismatch"):
        plain.put(0, _cache((8, 6)))
    from idm_vton_amd.garment_cache import GarmentCache
    with pytest.raises(ValueError, match=r"GarmentCache cat: gh mismatch"):
        GarmentCache.cat([plain, _cache((4, 4))])
    t = plain.take(1)
    assert t.sizes is None and (t.gh, t.gw) == SLOT and t.nbytes * 2 == plain.nbytes


def test_select_cat_and_to_carry_the_sizes_along():
    from idm_vton_amd.garment_cache import GarmentCache
    a, b = _slotted(2), _slotted(1, fill=2.0)
    g0, g1, g2 = _cache((4, 4), seed=1), _cache((8, 6), seed=2), _cache((4, 3), seed=3)
    a.put(0, g0), a.put(1, g1), b.put(0, g2)
    j = GarmentCache.cat([a, b])
    assert j.G == 3 and j.sizes == [(4, 4), (8, 6), (4, 3)] and (j.gh, j.gw) == SLOT
    assert [_equal(j.take(g), o) for g, o in enumerate((g0, g1, g2))] == [True] * 3
    s = j.select([2, 0, 2])
    assert s.sizes == [(4, 3), (4, 4), (4, 3)] and _equal(s.take(2), g2) and _equal(s.take(1), g0)
    assert j.to("cpu") is j
    big = j.for_person_size(16, 12)                                            # the same tensors re-declared: a put through one is seen by both
    big.put(1, g2.for_person_size(16, 12))
    assert (big.h, big.w) == (16, 12) and j.sizes == big.sizes == [(4, 4), (4, 3), (4, 3)] and _equal(j.take(1), g2)
    j.put(1, g1)
    assert j.garment_sizes([1, 1, 0, 2]) == [(8, 6), (8, 6), (4, 4), (4, 3)]
    assert _cache(SLOT, G=2).garment_sizes([1, 0]) == [SLOT, SLOT]
    with pytest.raises(ValueError, match="garment_index mismatch"):
        j.garment_sizes([3])
    with pytest.raises(ValueError, match="sizes / rows need one entry per garment"):
        _cache(SLOT, G=2, sizes=[SLOT])


def test_save_and_load_round_trip_the_sizes_and_version_1_files_still_load(tmp_path):
    import json
    from safetensors import safe_open
    from idm_vton_amd.garment_cache import GarmentCache
    pool = _slotted(2)
    one = _cache((8, 6), seed=9)
    pool.put(1, one)
    pool.save(str(tmp_path / "slotted.safetensors"))
    back = GarmentCache.load(str(tmp_path / "slotted.safetensors"))
    assert _equal(back, pool) and back.sizes == [SLOT, (8, 6)] and back.rows == pool.rows
    assert _equal(back.take(1), one)
    with safe_open(str(tmp_path / "slotted.safetensors"), framework="pt") as f:
        assert json.loads(f.metadata()["version"]) == 2
    plain = _cache(SLOT, G=2)
    plain.save(str(tmp_path / "plain.safetensors"))
    with safe_open(str(tmp_path / "plain.safetensors"), framework="pt") as f:                 # today's exact metadata: version 1, no new key
        meta = f.metadata()
        assert json.loads(meta["version"]) == 1 and sorted(meta) == sorted(
            ["format", "version", "G", "timesteps", "h", "w", "gh", "gw", "dtype", "attn_fp8", "f8_exp", "weights_id", "features"])
    back = GarmentCache.load(str(tmp_path / "plain.safetensors"))
    assert back.sizes is None and _equal(back, plain)


def test_widening_an_e4m3_feature_inverts_the_fp8_slot_order():
    """widen_f8 against the layout rule written out: position 64t + 32u + 16kb + 4g + j of the fp8 V^T holds key 64t + 32kb + 8g + 4u + j, and
    the 16-bit V^T keeps key k at k with bits 2 and 3 swapped."""
    from idm_vton_amd.garment_cache import widen_f8
    ld = 128
    key16 = torch.empty(ld)                                                    # 16-bit V^T row whose value at a key's place is the key
    for key in range(ld):
        key16[(key & ~12) | ((key & 4) << 1) | ((key & 8) >> 1)] = key % 16    # (values e4m3 holds exactly)
    v8 = torch.empty(ld)
    for pos in range(ld):
        t, u, kb, g, j = pos >> 6, (pos >> 5) & 1, (pos >> 4) & 1, (pos >> 2) & 3, pos & 3
        v8[pos] = (64 * t + 32 * kb + 8 * g + 4 * u + j) % 16
    vt8 = (v8 * 4.0).to(torch.float8_e4m3fn).view(torch.uint8).reshape(1, 1, ld)           # e4m3(v * 2^ev), ev = 2
    k8 = (torch.arange(-8, 8).float() * 0.5 * 2.0).to(torch.float8_e4m3fn).view(torch.uint8).reshape(1, 16)    # e4m3(k * 2^ek), ek = 1
    k, vt = widen_f8(k8, vt8, torch.float16, 1, 2)
    assert torch.equal(vt[0, 0].float(), key16) and torch.equal(k[0].float(), torch.arange(-8, 8).float() * 0.5)


# ------------------------------------------------------------------------------------------------------------------ GarmentPool
GARMENTS = {"a": ((4, 4), 11), "b": ((8, 6), 12), "c": ((8, 8), 13), "d": ((4, 3), 14)}


def _one(key):
    size, seed = GARMENTS[key]
    return _cache(size, seed=seed)


def test_a_mixed_size_pool_indexes_evicts_spills_compactly_and_restores_bit_for_bit():
    from idm_vton_amd.garment_cache import GarmentPool
    pool = GarmentPool(2, like=_cache(SLOT, seed=99), spill=True, mixed_sizes=True)
    assert pool.cache.sizes == [SLOT, SLOT] and (pool.cache.gh, pool.cache.gw) == SLOT
    encoded = []
    enc = lambda key: (encoded.append(key), _one(key))[1]
    assert pool.get(["a", "b", "a"], enc) == [0, 1, 0] and pool.cache.sizes == [(4, 4), (8, 6)]
    assert pool.get(["b"], enc) == [1]                                         # 'a' is now the least recently used
    assert pool.get(["c", "b"], enc) == [0, 1] and encoded == ["a", "b", "c"]  # ... and leaves for 'c', a garment of the slot's size
    assert pool.cache.sizes == [SLOT, (8, 6)] and pool.stats["evicted"] == 1
    assert _equal(pool.host["a"], _one("a")) and pool.host["a"].nbytes == _one("a").nbytes < _one("c").nbytes     # the host copy is compact
    assert pool.get(["a", "c"], enc) == [1, 0] and encoded == ["a", "b", "c"] and pool.stats["restored"] == 1
    assert pool.host["b"].nbytes == _one("b").nbytes and _equal(pool.host["b"], _one("b"))
    assert pool.cache.sizes == [SLOT, (4, 4)]
    assert _equal(pool.cache.take(1), _one("a")) and _equal(pool.cache.take(0), _one("c"))     # restored bit for bit
    for i in range(len(TS)):                                                   # 'a' came back into the slot 'b' left: no trace of 'b' in its V^T
        assert not _slot_views(pool.cache, i, 1)[0][1][:, 16:].any()
    assert pool.get(["d", "a"], enc) == [0, 1] and pool.cache.sizes == [(4, 3), (4, 4)] and _equal(pool.cache.take(0), _one("d"))


def test_a_mixed_size_pool_refuses_what_does_not_fit_and_loses_no_slot():
    from idm_vton_amd.garment_cache import GarmentPool
    pool = GarmentPool(2, like=_cache((8, 6), seed=99), mixed_sizes=True)
    with pytest.raises(ValueError, match="put: does not fit"):
        pool.get(["c"], _one)
    assert pool.get(["a", "d"], _one) == [0, 1] and pool.cache.sizes == [(4, 4), (4, 3)]
    plain = GarmentPool(2, like=_cache((8, 6), seed=99))                       # without mixed_sizes: today's pool, today's refusal
    assert plain.cache.sizes is None
    with pytest.raises(ValueError, match="put: gh mismatch"):
        plain.get(["a"], _one)
