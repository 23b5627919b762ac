"""-m gpu: the packed garment cache on the GPU.  Kernel level: idmvton_kv_unpack on framed operands (tests/frames.py) against the torch
definition of the format, bit for bit.  Cache level: pack() / unpack() on the device against the CPU reference.  Engine level: a call on a
packed cache against the same call on packed.unpack() -- the same arithmetic, so EQUALITY in every execution form --, a garment swapped in
place under captured graphs, the fp32 oracle, and the boundary pipeline."""
import pytest
import torch

from tests.engine_support import (DEV, RUNS, assert_bits, base_call, boundary_inputs, boundary_pipeline, e4m3_bytes, engine_inputs, engine_reference,
                                  garment_kw, ip_states, reference_draws, run_on)
from tests.garment_support import DTYPES, FINITE, FORMS, IDX, same_packed, scaled_cache

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ kernel


def _launch(runs, dtype, framed):
    from idm_vton_amd import ops
    from tests import frames
    exps = torch.tensor([r[4] for r in runs], dtype=torch.int32, device=DEV)
    srcs, dsts, descs = [], [], []
    for i, (rows, cols, lds, ldd, _) in enumerate(runs):
        b = e4m3_bytes(rows, cols, seed=i).to(DEV)
        if framed:
            s = frames.framed(b, lds)                    # gap columns and guard bands hold 0x7f: e4m3's NaN
            d = frames.framed_out((rows, cols), dtype, DEV, ldd)
        else:
            s, d = b, torch.empty((rows, cols), dtype=dtype, device=DEV)
        srcs.append(s); dsts.append(d)
        descs.append((s, d, exps[i:i + 1]))
    table = ops.kv_unpack(descs, dtype)
    torch.cuda.synchronize()
    return srcs, dsts, table


@DTYPES
def test_kv_unpack_framed_is_bit_equal_to_the_format_and_touches_nothing_else(dtype):
    from idm_vton_amd.garment_cache import unpack_values
    from tests import frames
    srcs, dsts, table = _launch(RUNS, dtype, framed=True)
    _, tight, _ = _launch(RUNS, dtype, framed=False)
    assert table.n == 5 and int(table.items.max()) == 515 * 40 and int(table.items.min()) == 1
    seen = set()
    for i, ((rows, cols, lds, ldd, e), s, d, t) in enumerate(zip(RUNS, srcs, dsts, tight)):
        b = e4m3_bytes(rows, cols, seed=i)
        seen |= set(b.flatten().tolist())
        ref = unpack_values(b, torch.tensor(e), dtype)
        frames.assert_all_written(d, f"run {i}")
        frames.assert_frame_intact(d, f"run {i}")        # guard bands and the gap columns [cols, ldd)
        frames.assert_untouched(s, f"run {i} source")
        assert_bits(d, ref, b, f"run {i}: not the format's bits")
        assert_bits(d, t, b, f"run {i}: framed against tight")
    assert seen == set(FINITE.tolist())


@DTYPES
def test_kv_unpack_smallest_table(dtype):
    from idm_vton_amd.garment_cache import unpack_values
    from tests import frames
    srcs, dsts, table = _launch(RUNS[:1], dtype, framed=True)
    assert table.n == 1 and int(table.items.max()) == 1
    frames.assert_all_written(dsts[0])
    frames.assert_frame_intact(dsts[0])
    frames.assert_untouched(srcs[0])
    assert_bits(dsts[0], unpack_values(e4m3_bytes(1, 16, 0), torch.tensor(-7), dtype), e4m3_bytes(1, 16, 0), "1 x 16")


def test_kv_unpack_wrapper_refuses_a_malformed_run():
    from idm_vton_amd import ops
    e = torch.zeros(1, dtype=torch.int32, device=DEV)
    s, d = torch.zeros(4, 32, dtype=torch.uint8, device=DEV), torch.full((4, 32), float("nan"), dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match="kv_unpack: a run is"):
        ops.kv_unpack([(s, d.to(torch.bfloat16), e)], torch.float16)
    with pytest.raises(RuntimeError, match=r"idmvton_kv_unpack failed \(-1\).*cols=24"):
        ops.kv_unpack([(s[:, :24], d[:, :24], e)], torch.float16)
    torch.cuda.synchronize()
    assert torch.isnan(d).all()                          # nothing was launched


# ------------------------------------------------------------------------------------------------------------------ pack / unpack
@DTYPES
def test_pack_and_unpack_on_the_device_equal_the_cpu_reference(dtype):
    """Synthetic values whose scales differ per garment, feature and tensor (exponents from -7 up, values below e4m3's normal range), and a
    tiny-model cache: bytes, exponents and the widened values, against plain torch on the host."""
    eng, inp, _ = engine_inputs(dtype, 2, 3)
    for c in (scaled_cache(G=3, dtype=dtype).to(DEV), eng.encode_garment(num_inference_steps=3, **garment_kw(inp))):
        p, ref = c.pack(), c.to("cpu").pack()
        assert p.packed and p.exps.is_cuda and all(k.is_cuda and k.dtype == torch.uint8 for k, _ in p.kv)
        assert same_packed(p.to("cpu"), ref) and p.to("cpu").exps.device.type == "cpu"
        assert p.nbytes == c.nbytes // 2 + p.exps.numel() * 4
        u, uref = p.unpack(), ref.unpack()
        assert all(k.is_cuda and k.dtype == dtype for k, _ in u.kv)
        assert all(torch.equal(a.cpu(), b) and torch.equal(x.cpu(), y) for (a, x), (b, y) in zip(u.kv, uref.kv))
        back = ref.to(DEV)                               # `to` moves the exponents with the bytes, pinned or not
        assert back.exps.is_cuda and same_packed(back.to("cpu", pin_memory=True), ref)


# ------------------------------------------------------------------------------------------------------------------ engine


@pytest.mark.parametrize("scheduler", ["ddpm", "ddim"])
@DTYPES
def test_packed_indexed_call_equals_the_call_on_the_unpacked_cache(dtype, scheduler):
    """P = 4 persons on a G = 3 packed cache, garment_index = [2, 0, 2, 1], 4 steps: every execution form against the same call on
    packed.unpack().  Unpacking into a set and unpacking into a cache are the same arithmetic."""
    steps = 4
    eng, inp, _ = engine_inputs(dtype, 4, steps)
    packed = eng.encode_garment(num_inference_steps=steps, scheduler=scheduler, storage="e4m3", **garment_kw(inp, 3))
    wide = packed.unpack()
    assert packed.packed and packed.G == 3 and not wide.packed and wide.nbytes == 2 * (packed.nbytes - packed.exps.numel() * 4)
    base = base_call(inp, steps, scheduler)
    n0 = eng.stats["garment_set_copies"]
    for form in FORMS:
        lat_p, lat_w = run_on(eng, base, packed, form, IDX), run_on(eng, base, wide, form, IDX)
        print(f"{dtype} {scheduler} {form}: max|packed - unpacked| = {(lat_p - lat_w).abs().max().item():.3e}")
        assert torch.isfinite(lat_w).all() and torch.equal(lat_p, lat_w), (form, (lat_p - lat_w).abs().max().item())
    assert eng.stats["garment_set_copies"] > n0
    assert not torch.equal(run_on(eng, base, packed, "serial_eager", [0, 0, 1, 2]), lat_w)   # another index gives other latents


@DTYPES
def test_packed_call_without_an_index_equals_the_unpacked_one(dtype):
    """P = G = 2, 7 steps (blocks of 1, 2, 4 timesteps), and the strength-0.6 call on the same 7-step cache (its entries found by value)."""
    steps = 7
    eng, inp, _ = engine_inputs(dtype, 2, steps)
    packed = eng.encode_garment(num_inference_steps=steps, storage="e4m3", **garment_kw(inp))
    wide = packed.unpack()
    base = base_call(inp, steps)
    for form in FORMS:
        lat_p, lat_w = run_on(eng, base, packed, form), run_on(eng, base, wide, form)
        assert torch.isfinite(lat_w).all() and torch.equal(lat_p, lat_w), (form, (lat_p - lat_w).abs().max().item())
    part = dict(base, strength=0.6, noise={**base["noise"], "image": torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(77)),
                                           "steps": inp["noise"]["steps"][:4]})
    for form in FORMS:
        lat_p, lat_w = run_on(eng, part, packed, form), run_on(eng, part, wide, form)
        assert torch.isfinite(lat_w).all() and torch.equal(lat_p, lat_w), ("strength 0.6", form)
    assert not torch.equal(lat_w, run_on(eng, base, wide, "serial_eager"))


@DTYPES
def test_encode_garment_e4m3_is_the_packed_native_cache_at_half_the_bytes(dtype):
    steps = 7
    eng, inp, _ = engine_inputs(dtype, 2, steps)
    n0 = eng.stats["garment_batches"]
    native = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp))
    n1 = eng.stats["garment_batches"]
    packed = eng.encode_garment(num_inference_steps=steps, storage="e4m3", **garment_kw(inp))
    assert eng.stats["garment_batches"] - n1 == n1 - n0 == 3
    assert packed.nbytes == native.nbytes // 2 + packed.exps.numel() * 4 and tuple(packed.exps.shape) == (2, len(native.kv), 2)
    assert "e4m3-packed" in repr(packed) and packed.timesteps == native.timesteps and packed.weights_id == native.weights_id
    assert same_packed(packed.to("cpu"), native.pack().to("cpu"))
    with pytest.raises(ValueError, match="storage='fp4'"):
        eng.encode_garment(num_inference_steps=steps, storage="fp4", **garment_kw(inp))
    eng8, inp8, _ = engine_inputs(torch.float16, 2, 3, fp8=True)
    with pytest.raises(ValueError, match="attn_fp8 engine's cache cannot be packed"):
        eng8.encode_garment(num_inference_steps=3, storage="e4m3", **garment_kw(inp8))


def test_a_garment_swapped_in_place_under_captured_graphs():
    """Two graph-form calls on one packed pool cache with a `put` between them: the second equals a fresh engine's call on the swapped cache
    built apart, the first did not change, and no graph state was added (bytes and exponents moved in place)."""
    from idm_vton_amd.garment_cache import GarmentCache
    steps = 3
    eng, inp, _ = engine_inputs(torch.float16, 4, steps)
    enc = lambda e, sl: e.encode_garment(num_inference_steps=steps, storage="e4m3", cloth=inp["cloth"][sl], text_embeds_cloth=inp["text_embeds_cloth"][sl],
                                         noise_cloth=inp["noise"]["cloth"][sl])
    pool, other = enc(eng, slice(0, 3)), enc(eng, slice(3, 4))
    base = base_call(inp, steps)
    fresh, _, _ = engine_inputs(torch.float16, 4, steps)
    before = GarmentCache.cat([pool.select([0]), pool.select([1]), pool.select([2])])
    swapped = GarmentCache.cat([pool.select([0]), other, pool.select([2])])
    ref_before, ref_after = run_on(fresh, base, before, "serial_eager", IDX), run_on(fresh, base, swapped, "serial_eager", IDX)
    assert not torch.equal(ref_before, ref_after)
    for form in ("graph", "graph_overlap"):
        assert torch.equal(run_on(eng, base, pool, form, IDX), ref_before), form
    states, graphs = len(eng._graphs), sum(len(g["graphs"]) for g in eng._graphs.values())
    ptrs = [k.data_ptr() for k, _ in pool.kv] + [pool.exps.data_ptr()]
    pool.put(1, other)
    assert ptrs == [k.data_ptr() for k, _ in pool.kv] + [pool.exps.data_ptr()]
    for form in ("graph", "graph_overlap"):
        assert torch.equal(run_on(eng, base, pool, form, IDX), ref_after), form
    assert len(eng._graphs) == states and sum(len(g["graphs"]) for g in eng._graphs.values()) == graphs
    pool.put(1, before.take(1).unpack())                 # a 16-bit source is packed on the device, then moved in
    assert torch.equal(run_on(eng, base, pool, "graph_overlap", IDX), ref_before)


PACKED_ORACLE_BAR = 1.49e-3                             # 1.25 x the measured 1.193e-3 (below the variant's 8e-2: the rule for measured stages)


def test_packed_call_against_the_oracle():
    """The packed call quantises a strict subset of what attn_fp8 quantises (the garment keys and values, not the person's, not Q, not P), so
    it is held to that variant's stated bar: latents within 8e-2 of the fp32 oracle on the tiny pipeline (3 steps, B = 2, fp16;
    tests/test_parity_gpu.py::test_fp8_attention_engine_matches_oracle_within_its_stated_tolerance).  It also differs from the 16-bit cached
    call: the packed bytes are what is read.
    Measured on the MI355X, both forms: packed 1.193e-3, the 16-bit cache 1.021e-3 (the kernels are bit-reproducible, so the figure does not
    move from run to run); the bar is 1.25 x the packed figure, which is below 8e-2."""
    from oracle import pipeline as opipe
    from oracle.scheduler import Scheduler
    from tests import parity_utils as pu
    steps = 3
    eng, inp, m = engine_inputs(torch.float16, 2, steps)
    o_t, o_g, o_v = m["oracle"]
    tr = {}
    opipe.run(o_t, o_g, o_v, Scheduler("ddpm"), num_inference_steps=steps, guidance_scale=2.0, trace=tr, **inp)
    native = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp))
    packed = eng.encode_garment(num_inference_steps=steps, storage="e4m3", **garment_kw(inp))
    base = base_call(inp, steps)
    for form in ("serial_eager", "graph_overlap"):
        lat_n, lat_p = run_on(eng, base, native, form), run_on(eng, base, packed, form)
        e_n, e_p = pu.relerr(lat_n, tr["step_latents"][-1]), pu.relerr(lat_p, tr["step_latents"][-1])
        print(f"{form}: latents against the oracle: packed {e_p:.3e}, 16-bit cache {e_n:.3e}")
        assert torch.isfinite(lat_p).all() and not torch.equal(lat_p, lat_n), form
        assert e_p <= PACKED_ORACLE_BAR, (form, e_p, e_n)


def test_boundary_pipeline_encodes_and_takes_a_packed_cache():
    """pipe.encode_garment(..., storage="e4m3") and pipe(cloth=<packed>, garment_index=...) against the engine-level call on the same draws."""
    from idm_vton_amd.garment_cache import PackedGarmentCache
    DT = torch.float16
    pipe, enc, kw = boundary_pipeline(DT)
    B, H, W, steps = 2, 128, 128, 3
    inp, clip_pix, call = boundary_inputs(kw, B, H, W, steps, DT)
    cache = pipe.encode_garment(inp["cloth"], inp["text_embeds_cloth"], steps, H, W, generator=torch.Generator(DEV).manual_seed(11), storage="e4m3")
    assert isinstance(cache, PackedGarmentCache) and cache.G == B and len(cache.timesteps) == steps
    index = [1, 1]
    torch.manual_seed(123)                                                         # the pose posterior uses the GLOBAL generator
    img_c = pipe(generator=torch.Generator(DEV).manual_seed(7), cloth=cache, text_embeds_cloth=None, garment_index=index, **call)[0]
    eng = pipe.hip_engine()
    _, noise = reference_draws(7, 123, B, H, W, steps, DT)
    ip = ip_states(enc, clip_pix)
    ref = engine_reference(eng, inp, noise, ip, steps, cloth=cache, garment_index=index)
    assert torch.isfinite(img_c).all() and torch.equal(img_c, ref)
    other = engine_reference(eng, inp, noise, ip, steps, cloth=cache, garment_index=[0, 1])
    assert not torch.equal(other, ref)
