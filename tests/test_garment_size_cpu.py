"""CPU tests of the garment running at its own resolution: GarmentCache's two sizes -- (h, w), the person latent size a cache is declared
for, and (gh, gw), the garment's own --, for_person_size, the size formula, and the keys under which the engine keeps persistent garment
sets and captured graphs (the key functions alone: no kernels, no device)."""
import pytest
import torch

from tests.garment_support import ask


def _cache(G=2, ts=(900, 500, 100), h=16, w=16, gh=8, gw=12, dtype=torch.float16, levels=((1, 64), (2, 128))):
    """A hand-built cache shaped like the engine's: per (level, channels) one feature whose token rows are round16 of the garment's token
    count at that level (the garment latent halves, rounding up, per level)."""
    from idm_vton_amd.garment_cache import GarmentCache
    from idm_vton_amd.ops import round16
    n, kv, rows = len(ts), [], []
    for level, Cc in levels:
        a, b = gh, gw
        for _ in range(level):
            a, b = (a + 1) // 2, (b + 1) // 2
        N = round16(a * b)
        rows.append((N, Cc))
        kv.append((torch.zeros(n * G * N, Cc, dtype=dtype), torch.zeros(n * G, Cc, N, dtype=dtype)))
    return GarmentCache(G=G, timesteps=ts, h=h, w=w, gh=gh, gw=gw, dtype=dtype, attn_fp8=False, f8_exp=(2, 2, 2), weights_id="w0", kv=kv), rows


def test_garment_size_defaults_to_the_person_size_and_shows_in_the_repr_only_when_it_differs():
    from idm_vton_amd.garment_cache import GarmentCache
    kv = [(torch.zeros(2 * 16, 64), torch.zeros(2, 64, 16))]
    same = GarmentCache(G=1, timesteps=(5, 1), h=4, w=4, dtype=torch.float32, attn_fp8=False, f8_exp=(2, 2, 2), weights_id="w", kv=kv)
    assert (same.gh, same.gw) == (4, 4) and "garment" not in repr(same)
    c, _ = _cache()
    assert (c.h, c.w, c.gh, c.gw) == (16, 16, 8, 12) and "garment latent=8x12" in repr(c) and "latent=16x16" in repr(c)


def test_check_is_still_the_person_size_check():
    """A cache of an 8x12 garment declared for 16x16 persons: the call's PERSON size is what `check` compares; the garment's own size is not
    a size a call may run at unless it is declared."""
    c, _ = _cache()
    assert ask(c) == [0, 1, 2]
    for h, w in ((32, 32), (8, 12), (16, 12)):
        with pytest.raises(ValueError, match="GarmentCache resolution mismatch"):
            ask(c, h=h, w=w)


def test_for_person_size_shares_storage_and_then_passes():
    c, _ = _cache()
    d = c.for_person_size(32, 32)
    assert (d.h, d.w, d.gh, d.gw, d.G, d.timesteps) == (32, 32, 8, 12, c.G, c.timesteps)
    for (k, vt), (k2, vt2) in zip(c.kv, d.kv):
        assert k.data_ptr() == k2.data_ptr() and vt.data_ptr() == vt2.data_ptr()
    assert ask(d, h=32, w=32) == [0, 1, 2]
    with pytest.raises(ValueError, match="GarmentCache resolution mismatch"):
        ask(d, h=16, w=16)                                # the re-declared cache is as strict as the first
    assert ask(c) == [0, 1, 2] and (c.h, c.w) == (16, 16)  # and the first is unchanged
    assert d.nbytes == c.nbytes


def test_repeat_garments_carries_the_garment_size():
    c, _ = _cache(G=1)
    m = c.repeat_garments(2)
    assert (m.G, m.h, m.w, m.gh, m.gw) == (2, 16, 16, 8, 12) and m.nbytes == 2 * c.nbytes


def test_nbytes_is_the_formula():
    """Per garment and timestep: sum over features of N_f * C_f elements, times 2 tensors (K, V^T), times the element size.  With the SDXL
    topology -- 10 features of 640 channels at level 1 (N1 rows), 60 of 1280 at level 2 (N2 rows) -- that is
    (10 * N1 * 640 + 60 * N2 * 1280) * 2 * 2 bytes: a 384x512 garment (latent 48x64: N1 = 768, N2 = 192) over 30 steps is 2 359 296 000 B,
    a quarter of the 768x1024 garment's 9 437 184 000 B."""
    from idm_vton_amd.ops import round16
    c, rows = _cache(G=2, ts=(900, 500, 100), gh=9, gw=5)                 # a 72x40 cloth: 15 tokens at level 1, 6 at level 2 -> 16 rows each
    assert rows == [(16, 64), (16, 128)]
    assert c.nbytes == sum(N * Cc for N, Cc in rows) * 2 * 2 * 2 * 3       # K and V^T, 2 bytes, G = 2, 3 timesteps
    sdxl = lambda gh, gw: (10 * round16((gh + 1) // 2 * ((gw + 1) // 2)) * 640 +
                           60 * round16((((gh + 1) // 2) + 1) // 2 * ((((gw + 1) // 2) + 1) // 2)) * 1280) * 2 * 2
    assert sdxl(64, 48) * 30 == 2_359_296_000 and sdxl(128, 96) * 30 == 9_437_184_000
    # the same count from a cache object of that shape, without allocating it: meta tensors
    from idm_vton_amd.garment_cache import GarmentCache
    kv = [(torch.empty(30 * 768, 640, dtype=torch.bfloat16, device="meta"), torch.empty(30, 640, 768, dtype=torch.bfloat16, device="meta"))] * 10 + \
         [(torch.empty(30 * 192, 1280, dtype=torch.bfloat16, device="meta"), torch.empty(30, 1280, 192, dtype=torch.bfloat16, device="meta"))] * 60
    big = GarmentCache(G=1, timesteps=range(30), h=128, w=96, gh=64, gw=48, dtype=torch.bfloat16, attn_fp8=False, f8_exp=(2, 2, 2),
                       weights_id="w", kv=kv)
    assert big.nbytes == 2_359_296_000


def test_set_and_graph_keys_tell_garment_sizes_apart():
    """Two calls that differ only in the garment's size must not share persistent sets (their shapes differ) nor captured graphs (the captured
    launches carry the garment geometry)."""
    from idm_vton_amd.pipeline import TryonEngine
    st = lambda gh, gw, **kw: dict(dict(B=2, h=16, w=16, gh=gh, gw=gw, k=4, steps_noise=None, gcache=None), **kw)
    a, b = st(16, 16), st(8, 12)
    assert TryonEngine._set_key(a) != TryonEngine._set_key(b)
    assert TryonEngine._graph_key(a, True) != TryonEngine._graph_key(b, True)
    assert TryonEngine._graph_key(a, True) == TryonEngine._graph_key(st(16, 16), True)
    # a set's shapes do not depend on the person's size; a graph state does (latents, cond, x_in)
    assert TryonEngine._set_key(b) == TryonEngine._set_key(st(8, 12, h=32, w=32))
    assert TryonEngine._graph_key(b, True) != TryonEngine._graph_key(st(8, 12, h=32, w=32), True)
    # on a cache: the garment size and the garment count are part of the key, and a cached state is never a live one
    c8, _ = _cache(gh=8, gw=12)
    c4, _ = _cache(gh=4, gw=12)
    ka, kb = TryonEngine._graph_key(st(8, 12, gcache=c8), False), TryonEngine._graph_key(st(4, 12, gcache=c4), False)
    assert ka != kb and ka != TryonEngine._graph_key(st(8, 12), True)


def test_garment_latent_size_needs_multiples_of_8():
    from idm_vton_amd.pipeline import TryonEngine
    assert TryonEngine._garment_latent_size(torch.zeros(1, 3, 72, 40)) == (9, 5)
    for shape in ((1, 3, 70, 40), (1, 3, 72, 44)):
        with pytest.raises(ValueError, match="divisible by 8"):
            TryonEngine._garment_latent_size(torch.zeros(shape))
