"""-m gpu: the FEATURE cache on the GPU.  encode_garment(storage="features") keeps GarmentNet's features F in place of their K / V^T; a
call on it fills a staging list per block and projects it with the launches an uncached call makes, so EQUALITY (torch.equal) with the
uncached call and with the K / V^T-cached call is the bar everywhere but the packed form's oracle test.  Tiny engines: latent 16x16, 3 steps
(blocks of 1 and 2 timesteps), the helpers of tests/engine_support.py."""
import pytest
import torch

from tests.engine_support import (DEV, base_call, boundary_inputs, boundary_pipeline, engine_inputs, engine_reference, garment_kw, inputs, ip_states, pair,
                                  reference_draws, run_on, to_host)
from tests.garment_support import DTYPES, FORMS, IDX, TRANSPORTS

pytestmark = pytest.mark.gpu

STEPS, NBLOCKS = 3, 2


def _kv_equal(a, b):
    assert (a.G, a.timesteps, a.h, a.w, a.gh, a.gw, a.dtype, a.weights_id, a.features, len(a.kv)) == \
           (b.G, b.timesteps, b.h, b.w, b.gh, b.gw, b.dtype, b.weights_id, b.features, len(b.kv))
    for f, (ea, eb) in enumerate(zip(a.kv, b.kv)):
        assert len(ea) == len(eb)
        for x, y in zip(ea, eb):
            assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), f


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheduler", ["ddpm", "ddim"])
@DTYPES
def test_feature_cached_call_equals_the_uncached_and_the_kv_cached_call(dtype, scheduler):
    """B = G = 2: the four execution forms and on_step.  No GarmentNet batch, one projection per block."""
    eng, inp, _ = engine_inputs(dtype, 2, STEPS)
    kw = dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler=scheduler, **inp)
    feats = eng.encode_garment(num_inference_steps=STEPS, scheduler=scheduler, storage="features", **garment_kw(inp))
    native = eng.encode_garment(num_inference_steps=STEPS, scheduler=scheduler, **garment_kw(inp))
    assert feats.features and not native.features and feats.G == 2 and 2 * feats.nbytes == native.nbytes
    assert len(eng._block_schedule(STEPS)[1]) == NBLOCKS
    base = base_call(inp, STEPS, scheduler)
    for form in FORMS:
        # pair's two calls, with the counters read around the feature-cached one (start latents and conditioning copied over: the person-side
        # VAE encodes of a cached prepare() run at another encoder batch size, which is not what is under test)
        st = eng.prepare(**kw)
        st_f = eng.prepare(**{**base, "cloth": feats})
        st_f["latents"].copy_(st["latents"])
        st_f["cond"].copy_(st["cond"])
        lat_u = eng.denoise(st, **FORMS[form]).clone()
        b0, p0 = eng.stats["garment_batches"], eng.stats["garment_projections"]
        lat_f = eng.denoise(st_f, **FORMS[form]).clone()
        assert (eng.stats["garment_batches"], eng.stats["garment_projections"]) == (b0, p0 + NBLOCKS), form
        lat_k = run_on(eng, base, native, form)
        b1, p1 = eng.stats["garment_batches"], eng.stats["garment_projections"]
        lat_f2 = run_on(eng, base, feats, form)                            # (through the state the K / V^T call left, where there is one)
        assert (eng.stats["garment_batches"], eng.stats["garment_projections"]) == (b1, p1 + NBLOCKS), form
        print(f"{dtype} {scheduler} {form}: max|features - uncached| = {(lat_u - lat_f).abs().max().item():.3e}")
        assert torch.isfinite(lat_u).all() and torch.equal(lat_f, lat_u), (form, (lat_u - lat_f).abs().max().item())
        assert torch.equal(lat_f2, lat_k), (form, (lat_f2 - lat_k).abs().max().item())


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [1, 2])
@DTYPES
def test_project_garment_gives_the_native_cache_bit_for_bit(dtype, G):
    eng, inp, _ = engine_inputs(dtype, 2, STEPS)
    feats = eng.encode_garment(num_inference_steps=STEPS, storage="features", **garment_kw(inp, G))
    native = eng.encode_garment(num_inference_steps=STEPS, **garment_kw(inp, G))
    p0 = eng.stats["garment_batches"]
    proj = eng.project_garment(feats)
    assert eng.stats["garment_batches"] == p0 and not proj.features and not proj.packed
    _kv_equal(proj, native)
    assert native.nbytes == 2 * feats.nbytes and proj.nbytes == native.nbytes
    # the layout: N_f = round16(feature_tokens) rows per garment and timestep, the engine's dtype, timestep-major
    tokens = eng.unet.feature_tokens(feats.gh, feats.gw)
    assert [e[0].shape[0] for e in feats.kv] == [STEPS * G * ((n + 15) // 16 * 16) for n in tokens]
    assert all(len(e) == 1 and e[0].dtype == dtype for e in feats.kv)
    assert all(torch.isfinite(e[0]).all() for e in feats.kv)             # the pad rows' filler is finite


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
def test_shared_segment_of_four_persons_on_two_feature_garments():
    eng, inp, _ = engine_inputs(torch.float16, 4, STEPS)
    feats = eng.encode_garment(num_inference_steps=STEPS, storage="features", **garment_kw(inp, 2))
    native = eng.encode_garment(num_inference_steps=STEPS, **garment_kw(inp, 2))
    base = base_call(inp, STEPS)
    for form in FORMS:
        lat_k, lat_f = run_on(eng, base, native, form), run_on(eng, base, feats, form)
        assert torch.isfinite(lat_k).all() and torch.equal(lat_f, lat_k), form


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def _ones(eng, inp, storage, which=(0, 1, 2)):
    return [eng.encode_garment(num_inference_steps=STEPS, storage=storage, cloth=inp["cloth"][g:g + 1], text_embeds_cloth=inp["text_embeds_cloth"][g:g + 1],
                               noise_cloth=inp["noise"]["cloth"][g:g + 1]) for g in which]


@DTYPES
def test_indexed_call_on_a_pool_of_feature_garments(dtype):
    """A pool cat of three G = 1 feature caches, index [2, 0, 2, 1] (P = 4, U = 3 garments in first-use order into slots 0..2 of 4-slot
    staging lists), against the call on cat of the three native G = 1 caches.  The projection then runs over M = c * 4 * N_f rows where
    the native garments were projected over c * N_f: equality rests on a GEMM row not depending on M, which is measured here, not implied."""
    from idm_vton_amd.garment_cache import GarmentCache
    eng, inp, _ = engine_inputs(dtype, 4, STEPS)
    pool, ref = GarmentCache.cat(_ones(eng, inp, "features")), GarmentCache.cat(_ones(eng, inp, "native"))
    assert pool.features and pool.G == 3 and 2 * pool.nbytes == ref.nbytes
    base = base_call(inp, STEPS)
    for form in FORMS:
        lat_k, lat_f = run_on(eng, base, ref, form, IDX), run_on(eng, base, pool, form, IDX)
        print(f"{dtype} {form}: max|features - kv| = {(lat_k - lat_f).abs().max().item():.3e}")
        assert torch.isfinite(lat_k).all() and torch.equal(lat_f, lat_k), (form, (lat_k - lat_f).abs().max().item())
    assert not torch.equal(run_on(eng, base, pool, "serial_eager", [0, 0, 0, 0]), lat_k)     # the index is read


def test_one_graph_state_serves_two_indices_and_a_put_in_place():
    from idm_vton_amd.garment_cache import GarmentCache
    eng, inp, _ = engine_inputs(torch.float16, 4, STEPS)
    f_ones, k_ones = _ones(eng, inp, "features", (0, 1, 2, 3)), _ones(eng, inp, "native", (0, 1, 2, 3))
    pool, ref = GarmentCache.cat(f_ones[:3]), GarmentCache.cat(k_ones[:3])
    swapped = GarmentCache.cat([k_ones[0], k_ones[3], k_ones[2]])
    base = base_call(inp, STEPS)
    a, b = [2, 0, 2, 1], [1, 1, 0, 2]
    want = {(name, tuple(i)): run_on(eng, base, c, "serial_eager", i) for name, c in (("before", ref), ("after", swapped)) for i in (a, b)}
    assert len({tuple(v.flatten().tolist()) for v in want.values()}) == 4
    run_on(eng, base, ref, "graph_overlap", a)                             # the state is captured on the K / V^T cache ...
    states, n_garm = len(eng._graphs), eng.stats["garment_batches"]
    captured = sum(len(g["graphs"]) for g in eng._graphs.values())
    for form in ("graph", "graph_overlap"):                              # ... and serves the feature pool
        for i in (a, b, a):
            assert torch.equal(run_on(eng, base, pool, form, i), want[("before", tuple(i))]), (form, i)
    ptr = pool.kv[0][0].data_ptr()
    pool.put(1, f_ones[3])
    assert pool.kv[0][0].data_ptr() == ptr
    for form in ("graph", "graph_overlap", "serial_eager"):
        for i in (a, b):
            assert torch.equal(run_on(eng, base, pool, form, i), want[("after", tuple(i))]), (form, i)
    assert torch.equal(run_on(eng, base, swapped, "graph_overlap", b), want[("after", tuple(b))])      # and the reverse: K / V^T through it again
    assert len(eng._graphs) == states == 1 and eng.stats["garment_batches"] == n_garm
    assert sum(len(g["graphs"]) for g in eng._graphs.values()) >= captured


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_feature_cache_built_at_full_strength_serves_strength_0_6(dtype):
    """7 steps at strength 1; the 0.6 call runs the last 4 timesteps, found by value, in blocks of 1, 2, 1: the projections run at the
    uncached 0.6 call's own M, on features that GarmentNet made in batches of 1, 2, 4 timesteps -- a measured equality, like its precedent
    tests/test_garment_cache_gpu.py::test_cache_built_at_full_strength_serves_strength_0_6."""
    steps = 7
    eng, inp, _ = engine_inputs(dtype, 2, steps)
    inp["noise"]["image"] = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(77))
    inp["noise"]["steps"] = inp["noise"]["steps"][:4]
    kw = dict(num_inference_steps=steps, guidance_scale=2.0, scheduler="ddpm", strength=0.6, **inp)
    feats = eng.encode_garment(num_inference_steps=steps, storage="features", **garment_kw(inp))
    for form in ("serial_eager", "graph_overlap"):
        lat_u, lat_f = pair(eng, kw, feats, form)
        assert torch.isfinite(lat_u).all() and torch.equal(lat_u, lat_f), (form, (lat_u - lat_f).abs().max().item())


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cloth", [(64, 96), (72, 40)], ids=["cloth64x96", "cloth72x40"])
def test_a_garment_at_its_own_size(cloth):
    """A 128x128 person; 72x40 is the odd latent 9x5: 15 and 6 tokens in 16 rows (64x96: 24 in 32, and 6), so the features carry pad rows,
    whose filler is the live call's."""
    dtype = torch.float16
    eng, _, m = engine_inputs(dtype, 2, STEPS)
    inp = inputs(m, 2, 128, 128, *cloth, STEPS, dtype)
    kw = dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler="ddpm", **inp)
    feats = eng.encode_garment(num_inference_steps=STEPS, storage="features", height=128, width=128, **garment_kw(inp))
    assert (feats.h, feats.w, feats.gh, feats.gw) == (16, 16, cloth[0] // 8, cloth[1] // 8)
    tokens = eng.unet.feature_tokens(feats.gh, feats.gw)
    assert [e[0].shape[0] // (STEPS * 2) for e in feats.kv] == [(n + 15) // 16 * 16 for n in tokens]
    assert any(n % 16 for n in tokens)                                   # 24 and 6 tokens (8x12), 15 and 6 (9x5): pad rows either way
    for form in FORMS:
        lat_u, lat_f = pair(eng, kw, feats, form)
        assert torch.isfinite(lat_u).all() and torch.equal(lat_u, lat_f), (form, (lat_u - lat_f).abs().max().item())
    _kv_equal(eng.project_garment(feats), eng.encode_garment(num_inference_steps=STEPS, height=128, width=128, **garment_kw(inp)))


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_packed_feature_call_equals_the_call_on_the_unpacked_cache(dtype):
    from idm_vton_amd.garment_cache import GarmentCache
    eng, inp, _ = engine_inputs(dtype, 4, STEPS)
    feats = eng.encode_garment(num_inference_steps=STEPS, storage="features", **garment_kw(inp, 3))
    packed = eng.encode_garment(num_inference_steps=STEPS, storage="features-e4m3", **garment_kw(inp, 3))
    assert packed.features and packed.packed and tuple(packed.exps.shape) == (3, len(feats.kv), 1)
    assert packed.nbytes == feats.nbytes // 2 + 4 * 3 * len(feats.kv)
    again = feats.pack()
    _kv_equal(packed, again)
    assert torch.equal(packed.exps, again.exps)
    unpacked = packed.unpack()
    assert unpacked.features and not unpacked.packed and not all(torch.equal(a[0], b[0]) for a, b in zip(unpacked.kv, feats.kv))   # lossy
    base = base_call(inp, STEPS)
    two, two_u = packed.select([0, 1]), unpacked.select([0, 1])
    for form in FORMS:
        c0, p0 = eng.stats["garment_set_copies"], eng.stats["garment_projections"]
        lat_p = run_on(eng, base, packed, form, IDX)
        # one unpack launch and one projection per block (a graph state's first call adds its warm-up fill to garment_set_copies, as ever)
        assert eng.stats["garment_set_copies"] - c0 in (NBLOCKS, NBLOCKS + 1) and eng.stats["garment_projections"] - p0 == NBLOCKS, form
        lat_u = run_on(eng, base, unpacked, form, IDX)
        assert torch.isfinite(lat_u).all() and torch.equal(lat_p, lat_u), ("index", form)
        lat_p, lat_u = run_on(eng, base, two, form), run_on(eng, base, two_u, form)              # P = 4 on G = 2, no index
        assert torch.isfinite(lat_u).all() and torch.equal(lat_p, lat_u), ("no index", form)
    _kv_equal(eng.project_garment(packed), eng.project_garment(unpacked))
    assert isinstance(again, GarmentCache)


# ---- 8 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [False, True], ids=["16bit", "packed"])
def test_host_resident_feature_cache_equals_the_device_resident_call(packed):
    """Page-locked host memory, both transports, every form, with an index (P = 4 on G = 3) and without (P = 4 on G = 2): one
    idmvton_kv_stream launch per block ("kernel"), one idmvton_kv_place launch per block ("copy"), one projection per block either way."""
    dtype = torch.float16
    eng, inp, _ = engine_inputs(dtype, 4, STEPS)
    device = eng.encode_garment(num_inference_steps=STEPS, storage="features-e4m3" if packed else "features", **garment_kw(inp, 3))
    base = base_call(inp, STEPS)
    for dev_c, index in ((device, IDX), (device.select([0, 1]), None)):
        host = to_host(dev_c, features=True)
        for form in FORMS:
            lat_d = run_on(eng, base, dev_c, form, index)
            states = len(eng._graphs)
            for transport in TRANSPORTS:
                s0 = dict(eng.stats)
                lat_h = run_on(eng, base, host, form, index, transport)
                assert torch.isfinite(lat_d).all() and torch.equal(lat_h, lat_d), (form, transport, index, (lat_h - lat_d).abs().max().item())
                delta = {key: eng.stats[key] - s0.get(key, 0) for key in eng.stats if key != "garment_stage_copies"}
                assert delta == dict(garment_batches=0, garment_set_copies=0, garment_projections=NBLOCKS,
                                     garment_stream_launches=NBLOCKS if transport == "kernel" else 0,
                                     garment_stage_launches=NBLOCKS if transport == "copy" else 0), (form, transport, delta)
                assert len(eng._graphs) == states, (form, transport)
    torch.cuda.synchronize()
    eng._release_streamed()
    assert eng._streaming == []
    stats = dict(eng.stats)
    with pytest.raises(ValueError, match="kv mismatch.*pageable.*pin_memory"):
        eng.prepare(**{**base, "cloth": device.to("cpu"), "garment_index": IDX})
    assert eng.stats == stats


# ---- 9 ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_anything_is_launched():
    from idm_vton_amd import ops
    from idm_vton_amd.garment_cache import GarmentPool, GarmentShelf
    dtype = torch.float16
    eng, inp, _ = engine_inputs(dtype, 2, STEPS)
    eng8, _, _ = engine_inputs(dtype, 2, STEPS, fp8=True)
    feats = eng.encode_garment(num_inference_steps=STEPS, storage="features", **garment_kw(inp, 1))
    native = eng.encode_garment(num_inference_steps=STEPS, **garment_kw(inp, 1))
    slotted = eng.empty_garment_cache(2, garment_height=128, garment_width=128, num_inference_steps=STEPS)
    base = base_call(inp, STEPS)
    torch.cuda.synchronize()
    stats, stats8, launched = dict(eng.stats), dict(eng8.stats), []
    real = ops._call
    ops._call = lambda *a, **kw: (launched.append(a[0]), real(*a, **kw))[1]
    try:
        for storage in ("features", "features-e4m3"):                    # an attn_fp8 engine neither encodes ...
            with pytest.raises(ValueError, match="attn_fp8"):
                eng8.encode_garment(num_inference_steps=STEPS, storage=storage, **garment_kw(inp, 1))
        with pytest.raises(ValueError, match="attn_fp8"):                # ... nor takes ...
            eng8.prepare(**{**base, "cloth": feats.repeat_garments(2)})
        with pytest.raises(ValueError, match="attn_fp8"):                # ... nor projects a feature cache
            eng8.project_garment(feats)
        with pytest.raises(ValueError, match="features"):                # a shelf add
            GarmentShelf(native).add("a", feats)
        with pytest.raises(ValueError, match="features"):                # a slotted cache: put, and as a pool
            slotted.put(0, feats)
        with pytest.raises(ValueError, match="features"):
            GarmentPool(2, like=feats, mixed_sizes=True)
        with pytest.raises(ValueError, match="features"):                # kinds do not mix
            native.put(0, feats)
        with pytest.raises(ValueError, match="storage"):
            eng.encode_garment(num_inference_steps=STEPS, storage="feature", **garment_kw(inp, 1))
    finally:
        ops._call = real
    assert launched == [] and eng.stats == stats and eng8.stats == stats8 and not eng._graphs and not eng8._graphs


# ---- 10 -----------------------------------------------------------------------------------------------------------------------------------
def test_boundary_pipeline_encodes_and_takes_a_feature_cache():
    DT = torch.float16
    pipe, enc, kw = boundary_pipeline(DT)
    B, H, W, steps = 2, 128, 128, STEPS
    inp, clip_pix, call = boundary_inputs(kw, B, H, W, steps, DT)
    feats = pipe.encode_garment(inp["cloth"], inp["text_embeds_cloth"], steps, H, W, generator=torch.Generator(DEV).manual_seed(11), storage="features")
    native = pipe.encode_garment(inp["cloth"], inp["text_embeds_cloth"], steps, H, W, generator=torch.Generator(DEV).manual_seed(11))
    assert feats.features and feats.G == B and 2 * feats.nbytes == native.nbytes
    eng = pipe.hip_engine()
    _kv_equal(eng.project_garment(feats), native)
    n_garm, n_proj = eng.stats["garment_batches"], eng.stats["garment_projections"]
    gen_c = torch.Generator(DEV).manual_seed(7)
    torch.manual_seed(123)                                                         # the pose posterior uses the GLOBAL generator
    img_c = pipe(generator=gen_c, cloth=feats, text_embeds_cloth=None, **call)[0]
    assert eng.stats["garment_batches"] == n_garm and eng.stats["garment_projections"] > n_proj
    # the engine-level call on the draws of the reference's order: the cloth draw is made and dropped
    gen, noise = reference_draws(7, 123, B, H, W, steps, DT)
    ip = ip_states(enc, clip_pix)
    ref = engine_reference(eng, inp, noise, ip, steps, cloth=native)
    assert torch.isfinite(img_c).all() and torch.equal(img_c, ref)
    gen_u = torch.Generator(DEV).manual_seed(7)
    torch.manual_seed(123)
    pipe(generator=gen_u, cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"], **call)
    assert torch.equal(gen_c.get_state(), gen_u.get_state()) and torch.equal(gen_c.get_state(), gen.get_state())


# ---- 11 -----------------------------------------------------------------------------------------------------------------------------------
PACKED_FEATURES_ORACLE_BAR = 1.52e-3                     # 1.25 x the measured 1.217e-3 (below the attn_fp8 variant's 8e-2: the rule for measured stages)


def test_packed_feature_call_against_the_oracle():
    """tests/test_garment_packed_gpu.py::test_packed_call_against_the_oracle for packed FEATURES: tiny pipeline, 3 steps, B = 2, fp16, the
    latents' max-rel error against the fp32 oracle.  The 16-bit feature call needs no bar of its own: its bits are the K / V^T-cached call's.
    Measured on the MI355X: packed features 1.217e-3, 16-bit features 1.021e-3 (the K / V^T cache's figure; the packed K / V^T cache has
    1.193e-3); the kernels are bit-reproducible, so the figure does not move from run to run.  The bar is 1.25 x the packed figure."""
    from oracle import pipeline as opipe
    from oracle.scheduler import Scheduler
    from tests import parity_utils as pu
    eng, inp, m = engine_inputs(torch.float16, 2, STEPS)
    o_t, o_g, o_v = m["oracle"]
    tr = {}
    opipe.run(o_t, o_g, o_v, Scheduler("ddpm"), num_inference_steps=STEPS, guidance_scale=2.0, trace=tr, **inp)
    feats = eng.encode_garment(num_inference_steps=STEPS, storage="features", **garment_kw(inp))
    packed = eng.encode_garment(num_inference_steps=STEPS, storage="features-e4m3", **garment_kw(inp))
    base = base_call(inp, STEPS)
    for form in ("serial_eager", "graph_overlap"):
        lat_n, lat_p = run_on(eng, base, feats, form), run_on(eng, base, packed, form)
        e_n, e_p = pu.relerr(lat_n, tr["step_latents"][-1]), pu.relerr(lat_p, tr["step_latents"][-1])
        print(f"{form}: latents against the oracle: packed features {e_p:.3e}, 16-bit features {e_n:.3e}")
        assert torch.isfinite(lat_p).all() and not torch.equal(lat_p, lat_n), form
        assert PACKED_FEATURES_ORACLE_BAR < 8e-2 and e_p <= PACKED_FEATURES_ORACLE_BAR, (form, e_p, e_n)
