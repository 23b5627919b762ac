"""CPU tests of the packed garment cache: the e4m3 format itself (exhaustively: 254 finite bytes x every exponent x both 16-bit dtypes),
PackedGarmentCache's primitives on CPU tensors, a GarmentPool over a packed cache, and the host side of idmvton_kv_unpack -- exported,
described by idmvton_sizeof, additive to ABI version 9, and every refusal raised before a launch (no GPU: the pointers are made up and never
dereferenced)."""
import ctypes as C
import os

import pytest
import torch

from tests.garment_support import DTYPES, FINITE, same_packed, scaled_cache


# ------------------------------------------------------------------------------------------------------------------ the format
@DTYPES
def test_every_byte_and_exponent_widens_exactly_and_packs_back(dtype):
    from idm_vton_amd.garment_cache import PACK_EXP_MAX, PACK_EXP_MIN, pack_values, unpack_values
    assert FINITE.numel() == 254 and (PACK_EXP_MIN, PACK_EXP_MAX) == (-7, 15)
    for e in range(PACK_EXP_MIN, PACK_EXP_MAX + 1):
        et = torch.tensor(e)
        x = unpack_values(FINITE, et, dtype)
        exact = FINITE.view(torch.float8_e4m3fn).double() * 2.0 ** -e
        assert torch.isfinite(x).all() and torch.equal(x.double(), exact), e
        assert torch.equal(pack_values(x, et), FINITE), e


def test_exponent_rule():
    from idm_vton_amd.garment_cache import pack_exponent
    assert pack_exponent(torch.tensor([0.0, 1e-9, 448.0, 449.0, 65504.0])).tolist() == [0, 15, 0, -1, -7]
    # against the rule as written, floor(log2(448 / amax)) in float64, on 16-bit values around every power of two
    for dtype in (torch.float16, torch.bfloat16):
        a = torch.cat([torch.tensor([2.0 ** p * f for p in range(-12, 10) for f in (0.874, 0.875, 0.876, 1.0, 1.7)]).to(dtype).float(),
                       torch.tensor([448.0, 224.0, 3.5, 7.0, 0.4375])])
        ref = torch.floor(torch.log2(448.0 / a.double())).clamp(-7, 15).to(torch.int32)
        assert torch.equal(pack_exponent(a), ref)


@DTYPES
@pytest.mark.parametrize("scale", [1e-3, 1.0, 37.0, 3000.0])
def test_error_bounds_on_random_tensors(scale, dtype):
    """|x' - x| <= 2^-4 |x| where |x| 2^e >= 2^-6 (e4m3's normal range: 3 mantissa bits, half an ulp), <= 2^-10 2^-e below (half a subnormal step)."""
    from idm_vton_amd.garment_cache import pack_exponent, pack_values, unpack_values
    x = torch.randn(64, 257, generator=torch.Generator().manual_seed(3)) * scale
    x[:8] *= 2.0 ** -15                                  # values below e4m3's normal range under the tensor's exponent
    x = x.to(dtype)
    e = pack_exponent(x.abs().amax())
    b = pack_values(x, e)
    assert not ((b & 0x7f) == 0x7f).any()                # no NaN byte
    xd, yd = x.double(), unpack_values(b, e, dtype).double()
    normal = xd.abs() * 2.0 ** int(e) >= 2.0 ** -6
    assert normal.any() and (~normal).any()
    assert ((yd - xd).abs()[normal] <= 2.0 ** -4 * xd.abs()[normal]).all()
    assert ((yd - xd).abs()[~normal] <= 2.0 ** -10 * 2.0 ** -int(e)).all()


# ------------------------------------------------------------------------------------------------------------------ the cache


@DTYPES
def test_pack_unpack_round_trip_and_nbytes(dtype):
    from idm_vton_amd.garment_cache import PackedGarmentCache
    c = scaled_cache(dtype=dtype)
    p = c.pack()
    assert isinstance(p, PackedGarmentCache) and p.packed and not c.packed and p.dtype == dtype and not p.attn_fp8
    assert "e4m3-packed" in repr(p) and "e4m3-packed" not in repr(c)
    assert tuple(p.exps.shape) == (2, 2, 2) and p.exps.dtype == torch.int32 and len(set(p.exps.flatten().tolist())) > 2
    assert p.nbytes == c.nbytes // 2 + p.exps.numel() * 4
    assert all(a.shape == b.shape and u.shape == v.shape for (a, u), (b, v) in zip(c.kv, p.kv))
    u = p.unpack()
    assert type(u) is type(c) and u.dtype == dtype and u.nbytes == c.nbytes
    n, G = len(c.timesteps), c.G
    for f, ((k, vt), (k2, vt2)) in enumerate(zip(c.kv, u.kv)):
        for j, (x, y) in enumerate(((k, k2), (vt, vt2))):
            xd, yd = x.double().reshape(n, G, -1), y.double().reshape(n, G, -1)
            sc = 2.0 ** p.exps[:, f, j].double().view(1, G, 1)
            normal = xd.abs() * sc >= 2.0 ** -6
            err = (yd - xd).abs()
            assert (err[normal] <= 2.0 ** -4 * xd.abs()[normal]).all() and (err <= torch.where(normal, err, 2.0 ** -10 / sc)).all()
    assert same_packed(u.pack(), p)                            # pack . unpack . pack reproduces bytes and exponents


def test_primitives_carry_the_exponents():
    from idm_vton_amd.garment_cache import GarmentCache
    c = scaled_cache(G=3)
    p = c.pack()
    s = p.select([2, 0, 2])
    assert s.G == 3 and torch.equal(s.exps, p.exps[[2, 0, 2]]) and same_packed(s, c.select([2, 0, 2]).pack())
    t = p.take(1)
    assert t.G == 1 and t.packed and torch.equal(t.exps, p.exps[1:2]) and same_packed(t, c.take(1).pack())
    assert same_packed(GarmentCache.cat([p.take(0), p.take(1), p.take(2)]), p)
    q = p.select([0, 1, 2])
    q.put(0, p.take(2))                                  # a packed source: bytes and exponents in place
    ptrs = [k.data_ptr() for k, _ in q.kv] + [q.exps.data_ptr()]
    q.put(1, c.take(0))                                  # a 16-bit source: packed first
    assert ptrs == [k.data_ptr() for k, _ in q.kv] + [q.exps.data_ptr()]
    assert same_packed(q, p.select([2, 0, 2]))
    shared = q.for_person_size(32, 24)
    assert shared.packed and shared.exps.data_ptr() == q.exps.data_ptr() and (shared.h, shared.w) == (32, 24)
    m = p.to("cpu", pin_memory=False)
    assert m is p
    r = p.repeat_garments(2)
    assert r.G == 6 and torch.equal(r.exps, p.exps.repeat(2, 1, 1))


def test_save_load_version_3_and_unpacked_still_version_1(tmp_path):
    import json
    from safetensors import safe_open
    from idm_vton_amd.garment_cache import GarmentCache
    c = scaled_cache()
    p = c.pack()
    p.save(str(tmp_path / "p.safetensors"))
    c.save(str(tmp_path / "c.safetensors"))
    with safe_open(str(tmp_path / "p.safetensors"), framework="pt") as f:
        meta = {k: json.loads(v) for k, v in f.metadata().items()}
        assert meta["version"] == 3 and meta["packed"] is True and "exps" in f.keys()
    with safe_open(str(tmp_path / "c.safetensors"), framework="pt") as f:
        meta = {k: json.loads(v) for k, v in f.metadata().items()}
        assert meta["version"] == 1 and "packed" not in meta and "exps" not in f.keys()
    back = GarmentCache.load(str(tmp_path / "p.safetensors"))
    assert same_packed(back, p) and back.timesteps == p.timesteps and back.dtype == p.dtype and back.weights_id == p.weights_id
    assert not GarmentCache.load(str(tmp_path / "c.safetensors")).packed


def test_refusals():
    from idm_vton_amd.garment_cache import GarmentCache
    c = scaled_cache()
    with pytest.raises(ValueError, match="already e4m3-packed"):
        c.pack().pack()
    with pytest.raises(ValueError, match="attn_fp8 cache cannot be packed"):
        scaled_cache(attn_fp8=True).pack()
    with pytest.raises(ValueError, match="`sizes`.*cannot be packed"):
        scaled_cache(sizes=[(16, 12), (16, 12)]).pack()
    with pytest.raises(ValueError, match="GarmentCache cat: packed mismatch"):
        GarmentCache.cat([c.pack(), c])
    with pytest.raises(ValueError, match="GarmentCache cat: packed mismatch"):
        GarmentCache.cat([c, c.pack()])
    with pytest.raises(ValueError, match="GarmentCache put: packed mismatch"):
        c.select([0, 1]).put(0, c.pack().take(0))        # a packed garment into a 16-bit cache: never silently
    # `check` keeps its fields: the engine's 16-bit dtype, attn_fp8 False
    p = c.pack()
    kw = dict(timesteps=p.timesteps, h=p.h, w=p.w, dtype=p.dtype, attn_fp8=False, f8_exp=p.f8_exp, weights_id=p.weights_id, persons=2)
    assert p.check(**kw) == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="GarmentCache dtype mismatch"):
        p.check(**{**kw, "dtype": torch.bfloat16})
    with pytest.raises(ValueError, match="GarmentCache attn_fp8 mismatch"):
        p.check(**{**kw, "attn_fp8": True})


def test_pool_over_a_packed_cache_spills_and_restores_bit_identically():
    from idm_vton_amd.garment_cache import GarmentPool
    ones = {key: scaled_cache(G=1, seed=s) for s, key in enumerate("abc")}
    packed = {key: one.pack() for key, one in ones.items()}
    calls = []

    def encode(key):
        calls.append(key)
        return packed[key] if key != "b" else ones[key]  # encode= may return packed or 16-bit garments
    pool = GarmentPool(2, like=packed["a"], spill=1)
    assert pool.cache.packed and pool.cache.G == 2 and pool.cache.nbytes == 2 * (packed["a"].nbytes - 16) + 32
    assert pool.get(["a", "b"], encode) == [0, 1]
    assert pool.get(["c", "b"], encode) == [0, 1]        # evicts a -> pinned-free host copy (CPU pool), packed bytes
    assert list(pool.host) == ["a"] and pool.host["a"].packed and same_packed(pool.host["a"], packed["a"])
    assert pool.host["a"].nbytes == packed["a"].nbytes
    assert pool.get(["a", "b"], encode) == [0, 1]        # evicts c, restores a from the host
    assert calls == ["a", "b", "c"] and pool.stats == dict(hits=2, encoded=3, restored=1, evicted=2)
    assert same_packed(pool.cache.take(0), packed["a"]) and same_packed(pool.cache.take(1), packed["b"])
    assert list(pool.host) == ["a"]                      # spill=1: the bound drops c's copy, never the one being restored


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_kv_unpack_is_exported_described_and_additive():
    from idm_vton_amd import ffi
    L = ffi.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "idmvton_hip.h")).read()
    assert "int idmvton_kv_unpack(const idmvton_kv_unpack_args* a, const idmvton_kv_unpack_desc* host_desc, void* stream);" in header
    assert "idmvton_kv_unpack" in ffi.SYMBOLS and hasattr(L, "idmvton_kv_unpack")
    assert L.idmvton_sizeof(b"idmvton_kv_unpack_desc") == 40 == C.sizeof(ffi.KvUnpackDesc)
    assert L.idmvton_sizeof(b"idmvton_kv_unpack_args") == 24 == C.sizeof(ffi.KvUnpackArgs)
    assert L.idmvton_abi_version() == 9 == ffi.ABI_VERSION


def _table(over=None, n=2):
    """A valid table of n runs 32 x 64 (made-up addresses) with the fields of `over` = {(index, field): value} changed."""
    from idm_vton_amd import ffi
    host = (ffi.KvUnpackDesc * n)()
    for i in range(n):
        host[i].src, host[i].dst, host[i].exp = 0x100000 + 0x10000 * i, 0x800000 + 0x10000 * i, 0x40000 + 4 * i
        host[i].rows, host[i].cols, host[i].lds, host[i].ldd = 32, 64, 64, 64
    for (i, field), v in (over or {}).items():
        setattr(host[i], field, v)
    a = ffi.KvUnpackArgs()
    a.dtype, a.n, a.desc, a.max_chunks = ffi.BF16, n, 0x200000, 1
    return a, host


REFUSALS = [
    ("src null", {(1, "src"): None}, {}, -5, "descriptor 1 has a null pointer"),
    ("dst null", {(0, "dst"): None}, {}, -5, "descriptor 0 has a null pointer"),
    ("exp null", {(0, "exp"): None}, {}, -5, "descriptor 0 has a null pointer"),
    ("src alignment", {(1, "src"): 0x100008}, {}, -3, "descriptor 1: src / dst not 16-byte aligned"),
    ("dst alignment", {(0, "dst"): 0x800002}, {}, -3, "descriptor 0: src / dst not 16-byte aligned"),
    ("rows", {(0, "rows"): 0}, {}, -1, "descriptor 0: rows=0 cols=64"),
    ("cols < 16", {(0, "cols"): 0}, {}, -1, "descriptor 0: rows=32 cols=0"),
    ("cols % 16", {(1, "cols"): 40}, {}, -1, "descriptor 1: rows=32 cols=40"),
    ("lds < cols", {(0, "lds"): 48}, {}, -1, r"descriptor 0: lds=48 \(>= cols=64"),
    ("lds % 16", {(0, "lds"): 72}, {}, -1, r"descriptor 0: lds=72 \(>= cols=64"),
    ("ldd < cols", {(1, "ldd"): 56}, {}, -1, r"descriptor 1: ldd=56 \(>= cols=64"),
    ("ldd % 8", {(1, "ldd"): 68}, {}, -1, r"descriptor 1: ldd=68 \(>= cols=64"),
    ("dtype", {}, dict(dtype=2), -2, "dtype 2"),
    ("dtype f8", {}, dict(dtype=3), -2, "dtype 3"),
    ("n", {}, dict(n=0), -5, "n=0 outside"),
    ("max_chunks small", {(0, "rows"): 600}, {}, -5, "max_chunks=1, the largest run has 3 chunks"),
    ("max_chunks large", {}, dict(max_chunks=2), -5, "max_chunks=2, the largest run has 1 chunks"),
    ("device table null", {}, dict(desc=None), -5, "null args / descriptor table"),
    ("device table alignment", {}, dict(desc=0x200008), -3, "device descriptor table is not 16-byte aligned"),
]


@pytest.mark.parametrize("over,args,code,msg", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_kv_unpack_refuses_on_the_host(over, args, code, msg):
    from idm_vton_amd import ffi
    L = ffi.lib()
    a, host = _table(over)
    for k, v in args.items():
        setattr(a, k, v)
    assert L.idmvton_kv_unpack(C.byref(a), C.cast(host, C.c_void_p), None) == code
    with pytest.raises(RuntimeError, match=msg):
        ffi.call_kv_unpack(a, host, 0)


def test_kv_unpack_refuses_null_arguments():
    from idm_vton_amd import ffi
    L = ffi.lib()
    a, host = _table()
    assert L.idmvton_kv_unpack(None, C.cast(host, C.c_void_p), None) == -5
    assert L.idmvton_kv_unpack(C.byref(a), None, None) == -5 and b"null args" in L.idmvton_last_error()


def test_fill_records_are_the_descriptors_of_the_layout_rule():
    """The table the engine uploads, against slot_run's views: (entry, garment) of the packed list -> (timestep slot, set slot) of a 16-bit
    set, one record per (timestep, garment, feature, K | V^T) in that order, each a valid idmvton_kv_unpack_desc."""
    from idm_vton_amd import ffi
    from idm_vton_amd.garment_cache import alloc_kv, fill_records, kv_shapes, slot_run
    p = scaled_cache(G=3).pack()
    n, G, k, S = 5, 3, 4, 2
    dst = alloc_kv([((a[0] // G * S,) + a[1:], (b[0] // G * S,) + b[1:], torch.float16) for a, b, _ in kv_shapes(p.kv)], n, k, "cpu")
    entries, tslots, garments, gslots = [4, 1, 2], [0, 1, 2], [2, 0], [0, 1]
    rec = fill_records(p.kv, n, G, dst, k, S, p.exps, entries, tslots, garments, gslots)
    assert rec.dtype == torch.int64 and tuple(rec.shape) == (3 * 2 * 2 * 2, 5) and rec.is_contiguous()
    descs = (ffi.KvUnpackDesc * rec.shape[0]).from_address(rec.data_ptr())
    at = 0
    for i, j in zip(entries, tslots):
        for g, u in zip(garments, gslots):
            for f, ((sk, sv), (dk, dv)) in enumerate(zip(slot_run(p.kv, n, G, i, g), slot_run(dst, k, S, j, u))):
                for t, (s, d) in enumerate(((sk, dk), (sv[0], dv[0]))):
                    x = descs[at]
                    assert (x.src, x.dst, x.exp) == (s.data_ptr(), d.data_ptr(), p.exps[g, f, t].data_ptr()), (i, g, f, t)
                    assert (x.rows, x.cols, x.lds, x.ldd) == (s.shape[0], s.shape[1], s.stride(0), d.stride(0))
                    at += 1
