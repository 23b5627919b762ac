"""CPU tests of the garment cache: the two shared-segment attention entry points exist and validate their arguments on the host (no
launch), the C ABI did not move, and GarmentCache's lookup / refusals on CPU tensors (no kernels)."""
import ctypes as C

import pytest
import torch

from tests.garment_support import ask, attn_args, attn_f8_args


def test_shared_entry_points_are_exported_and_the_abi_did_not_move():
    from idm_vton_amd import ffi
    L = ffi.lib()
    for s in ("idmvton_attn_fwd_shared", "idmvton_attn_f8_shared"):
        assert s in ffi.SYMBOLS and hasattr(L, s), s
    assert L.idmvton_abi_version() == 9
    # sizeof() of the two attention structs as built from the commit before the shared entry points: the change is additive
    assert L.idmvton_sizeof(b"idmvton_attn_args") == 144 == C.sizeof(ffi.AttnArgs)
    assert L.idmvton_sizeof(b"idmvton_attn_f8_args") == 128 == C.sizeof(ffi.AttnF8Args)


@pytest.mark.parametrize("fn,make", [("idmvton_attn_fwd_shared", lambda: attn_args(0)), ("idmvton_attn_f8_shared", attn_f8_args)],
                         ids=["attn_fwd_shared", "attn_f8_shared"])
def test_seg_nb_is_validated_on_the_host(fn, make):
    """seg_nb[s] >= 0 and, when non-zero, <= B - seg_b0[s]: refused with a message before any launch."""
    from idm_vton_amd import ffi
    L = ffi.lib()
    with pytest.raises(RuntimeError, match=r"seg_nb=-1"):
        ffi.call_shared(fn, make(), (0, -1), 0)
    with pytest.raises(RuntimeError, match=r"seg 1 seg_nb=3 outside \[0, B - seg_b0 = 2\]"):
        ffi.call_shared(fn, make(), (0, 3), 0)            # B = 4, seg_b0[1] = 2: at most 2 elements
    with pytest.raises(RuntimeError, match=r"seg 0 seg_nb=5"):
        ffi.call_shared(fn, make(), (5, 0), 0)
    rc = getattr(L, fn)(C.byref(make()), None, None)      # the C contract itself: a negative code + idmvton_last_error()
    assert rc == -5 and b"null seg_nb" in L.idmvton_last_error()
    nb = (C.c_int32 * 2)(0, 3)
    assert getattr(L, fn)(C.byref(make()), nb, None) == -1 and b"seg_nb=3" in L.idmvton_last_error()


def test_cross_mode_takes_no_shared_segment():
    from idm_vton_amd import ffi
    with pytest.raises(RuntimeError, match=r"CROSS mode takes seg_nb = \{0, 0\}"):
        ffi.call_shared("idmvton_attn_fwd_shared", attn_args(ffi.ATTN_CROSS, b0=0), (0, 2), 0)
    with pytest.raises(RuntimeError, match=r"CROSS mode takes seg_nb = \{0, 0\}"):
        ffi.call_shared("idmvton_attn_fwd_shared", attn_args(ffi.ATTN_CROSS, b0=0), (1, 0), 0)


def test_ops_segment_dicts_route_nb_to_the_shared_entry_point():
    """`nb` absent or 0 keeps the old entry point (and the tune-table key has no nb in it)."""
    from idm_vton_amd import ops
    assert ops._seg_nb([dict(nk=4), dict(nk=4, b0=2)]) is None
    assert ops._seg_nb([dict(nk=4), dict(nk=4, b0=2, nb=0)]) is None
    assert ops._seg_nb([dict(nk=4), dict(nk=4, b0=2, nb=1)]) == [0, 1]
    assert ops._seg_nb([dict(nk=4, nb=2)]) == [2, 0]
    a, b = attn_args(0), attn_args(0)
    assert ops.attn_key(a) == ops.attn_key(b) == "1,0,4,2,64,2,64,64,2"


# ------------------------------------------------------------------------------------------------------------------ GarmentCache
def _cache(G=2, ts=(900, 700, 500, 300, 100), h=16, w=12, dtype=torch.float16, attn_fp8=False, f8_exp=(2, 2, 2), wid="w0"):
    from idm_vton_amd.garment_cache import GarmentCache
    n, kv = len(ts), []
    for f, (N, Cc) in enumerate(((h * w, 64), (h * w // 4, 128))):
        k = torch.arange(n * G * N * Cc, dtype=torch.float32).reshape(n * G * N, Cc).to(dtype) + f
        vt = torch.arange(n * G * Cc * N, dtype=torch.float32).reshape(n * G, Cc, N).to(dtype) - f
        kv.append((k, vt))
    return GarmentCache(G=G, timesteps=ts, h=h, w=w, dtype=dtype, attn_fp8=attn_fp8, f8_exp=f8_exp, weights_id=wid, kv=kv)


def test_cache_lookup_is_by_timestep_value():
    c = _cache()
    assert ask(c) == [0, 1, 2, 3, 4]
    assert ask(c, timesteps=[500, 300, 100]) == [2, 3, 4]           # strength = 0.6 of the same schedule: its last three timesteps
    assert ask(c, timesteps=torch.tensor([300, 900])) == [3, 0]
    assert ask(c, persons=6) == [0, 1, 2, 3, 4]                     # P = 3 G
    G, n = c.G, len(c.timesteps)
    for f, (k, vt) in enumerate(c.kv):
        r = k.shape[0] // n
        kk, vv = c.step(3)[f]
        assert torch.equal(kk, k[3 * r:4 * r]) and torch.equal(vv, vt[3 * G:4 * G])
        assert kk.data_ptr() == k[3 * r:].data_ptr()                 # views, not copies
        kk, vv = c.run(1, 3)[f]
        assert torch.equal(kk, k[r:4 * r]) and torch.equal(vv, vt[G:4 * G])
    assert c.nbytes == sum(k.numel() * 2 + vt.numel() * 2 for k, vt in c.kv)
    with pytest.raises(IndexError):
        c.run(3, 3)


@pytest.mark.parametrize("field,over", [("timesteps", dict(timesteps=[500, 301])), ("resolution", dict(h=12, w=16)),
                                        ("dtype", dict(dtype=torch.bfloat16)), ("attn_fp8", dict(attn_fp8=True)),
                                        ("weights", dict(weights_id="w1")), ("persons", dict(persons=3))])
def test_cache_refuses_a_call_it_was_not_built_for(field, over):
    with pytest.raises(ValueError, match=f"GarmentCache {field} mismatch"):
        ask(_cache(), **over)


def test_cache_refuses_other_fp8_exponents_and_bad_construction():
    from idm_vton_amd.garment_cache import GarmentCache
    c = _cache(attn_fp8=True)
    assert ask(c) == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="GarmentCache f8_exp mismatch"):
        ask(c, f8_exp=(2, 3, 2))
    with pytest.raises(ValueError, match="distinct timesteps"):
        _cache(ts=(5, 5))
    with pytest.raises(ValueError, match="feature 0"):
        GarmentCache(G=2, timesteps=(1, 2), h=2, w=2, dtype=torch.float16, attn_fp8=False, f8_exp=(2, 2, 2), weights_id="w",
                     kv=[(torch.zeros(9, 64), torch.zeros(4, 64, 4))])


def test_repeat_garments_materialises_what_a_shared_segment_reads():
    """Person i reads garment i % G: the materialised form holds g0..gG-1 `times` times per timestep."""
    c = _cache(G=2)
    m = c.repeat_garments(2)
    assert m.G == 4 and m.timesteps == c.timesteps and m.nbytes == 2 * c.nbytes
    for i in range(len(c.timesteps)):
        for (k, vt), (km, vm) in zip(c.step(i), m.step(i)):
            N = k.shape[0] // c.G
            for person in range(4):
                g = person % c.G
                assert torch.equal(km[person * N:(person + 1) * N], k[g * N:(g + 1) * N]) and torch.equal(vm[person], vt[g])


def test_weights_fingerprint_tells_weight_sets_apart():
    from idm_vton_amd.garment_cache import weights_fingerprint
    g = torch.Generator().manual_seed(0)
    sd = {"a.weight": torch.randn(8, 8, generator=g), "b.bias": torch.randn(8, generator=g)}
    same = {k: v.clone() for k, v in reversed(list(sd.items()))}
    assert weights_fingerprint(sd) == weights_fingerprint(same)
    other = {k: v.clone() for k, v in sd.items()}
    other["b.bias"][3] += 0.5
    assert weights_fingerprint(sd) != weights_fingerprint(other)
    assert weights_fingerprint(sd) != weights_fingerprint({k: v.half() for k, v in sd.items()})
