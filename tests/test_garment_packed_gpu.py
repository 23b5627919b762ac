"""-m gpu: the packed garment cache on the GPU.  Kernel level: idmvton_kv_unpack on framed operands (tests/frames.py) against the torch
definition of the format, bit for bit.  Cache level: pack() / unpack() on the device against the CPU reference.  Engine level: a call on a
packed cache against the same call on packed.unpack() -- the same arithmetic, so EQUALITY in every execution form --, a garment swapped in
place under captured graphs, the fp32 oracle, and the boundary pipeline."""
import pytest
import torch

from tests.test_garment_cache_gpu import FORMS, _engine, _garment_kw
from tests.test_garment_index_gpu import _base, _run

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
FINITE = torch.tensor([b for b in range(256) if b & 0x7f != 0x7f], dtype=torch.uint8)


# ------------------------------------------------------------------------------------------------------------------ kernel
# (rows, cols, source row stride, destination row stride, exponent): unequal work -- 1 to 20600 16-byte items, so most blocks of the grid's
# x extent find nothing to do for most descriptors --, a gap in the source rows, in the destination rows, in both, and a V^T-shaped run
RUNS = [(1, 16, 16, 16, -7), (37, 80, 96, 88, -1), (200, 1280, 1280, 1280, 0), (3 * 128, 208, 208, 224, 6), (515, 640, 640, 640, 15)]


def _bytes(rows, cols, seed):
    """Random finite e4m3 bytes; the first 254 of a run that has room for them are all 254 finite values."""
    b = FINITE[torch.randint(0, 254, (rows * cols,), generator=torch.Generator().manual_seed(seed))]
    if rows * cols >= 254:
        b[:254] = FINITE
    return b.reshape(rows, cols)


def _assert_bits(got, ref, b, what):
    """torch.equal on the bit patterns, naming the first elements that differ: (row, column), source byte, bits written, bits expected."""
    from tests import frames
    g, r = frames.ints(got.cpu().contiguous()), frames.ints(ref.cpu().contiguous())
    bad = torch.nonzero(g != r)
    first = [(int(i), int(j), hex(int(b[i, j])), hex(int(g[i, j]) & 0xffff), hex(int(r[i, j]) & 0xffff)) for i, j in bad[:8].tolist()]
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} element(s) differ; (row, column, byte, got, expected) of the first: {first}"


def _launch(runs, dtype, framed):
    from idm_vton_amd import ops
    from tests import frames
    exps = torch.tensor([r[4] for r in runs], dtype=torch.int32, device=DEV)
    srcs, dsts, descs = [], [], []
    for i, (rows, cols, lds, ldd, _) in enumerate(runs):
        b = _bytes(rows, cols, seed=i).to(DEV)
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
        b = _bytes(rows, cols, seed=i)
        seen |= set(b.flatten().tolist())
        ref = unpack_values(b, torch.tensor(e), dtype)
        frames.assert_all_written(d, f"run {i}")
        frames.assert_frame_intact(d, f"run {i}")        # guard bands and the gap columns [cols, ldd)
        frames.assert_untouched(s, f"run {i} source")
        _assert_bits(d, ref, b, f"run {i}: not the format's bits")
        _assert_bits(d, t, b, f"run {i}: framed against tight")
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
    _assert_bits(dsts[0], unpack_values(_bytes(1, 16, 0), torch.tensor(-7), dtype), _bytes(1, 16, 0), "1 x 16")


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
    from tests.test_garment_packed_cpu import _cache, _same
    eng, inp, _ = _engine(dtype, 2, 3)
    for c in (_cache(G=3, dtype=dtype).to(DEV), eng.encode_garment(num_inference_steps=3, **_garment_kw(inp))):
        p, ref = c.pack(), c.to("cpu").pack()
        assert p.packed and p.exps.is_cuda and all(k.is_cuda and k.dtype == torch.uint8 for k, _ in p.kv)
        assert _same(p.to("cpu"), ref) and p.to("cpu").exps.device.type == "cpu"
        assert p.nbytes == c.nbytes // 2 + p.exps.numel() * 4
        u, uref = p.unpack(), ref.unpack()
        assert all(k.is_cuda and k.dtype == dtype for k, _ in u.kv)
        assert all(torch.equal(a.cpu(), b) and torch.equal(x.cpu(), y) for (a, x), (b, y) in zip(u.kv, uref.kv))
        back = ref.to(DEV)                               # `to` moves the exponents with the bytes, pinned or not
        assert back.exps.is_cuda and _same(back.to("cpu", pin_memory=True), ref)


# ------------------------------------------------------------------------------------------------------------------ engine
IDX = [2, 0, 2, 1]


@pytest.mark.parametrize("scheduler", ["ddpm", "ddim"])
@DTYPES
def test_packed_indexed_call_equals_the_call_on_the_unpacked_cache(dtype, scheduler):
    """P = 4 persons on a G = 3 packed cache, garment_index = [2, 0, 2, 1], 4 steps: every execution form against the same call on
    packed.unpack().  Unpacking into a set and unpacking into a cache are the same arithmetic."""
    steps = 4
    eng, inp, _ = _engine(dtype, 4, steps)
    packed = eng.encode_garment(num_inference_steps=steps, scheduler=scheduler, storage="e4m3", **_garment_kw(inp, 3))
    wide = packed.unpack()
    assert packed.packed and packed.G == 3 and not wide.packed and wide.nbytes == 2 * (packed.nbytes - packed.exps.numel() * 4)
    base = _base(inp, steps, scheduler)
    n0 = eng.stats["garment_set_copies"]
    for form in FORMS:
        lat_p, lat_w = _run(eng, base, packed, form, IDX), _run(eng, base, wide, form, IDX)
        print(f"{dtype} {scheduler} {form}: max|packed - unpacked| = {(lat_p - lat_w).abs().max().item():.3e}")
        assert torch.isfinite(lat_w).all() and torch.equal(lat_p, lat_w), (form, (lat_p - lat_w).abs().max().item())
    assert eng.stats["garment_set_copies"] > n0
    assert not torch.equal(_run(eng, base, packed, "serial_eager", [0, 0, 1, 2]), lat_w)   # another index gives other latents


@DTYPES
def test_packed_call_without_an_index_equals_the_unpacked_one(dtype):
    """P = G = 2, 7 steps (blocks of 1, 2, 4 timesteps), and the strength-0.6 call on the same 7-step cache (its entries found by value)."""
    steps = 7
    eng, inp, _ = _engine(dtype, 2, steps)
    packed = eng.encode_garment(num_inference_steps=steps, storage="e4m3", **_garment_kw(inp))
    wide = packed.unpack()
    base = _base(inp, steps)
    for form in FORMS:
        lat_p, lat_w = _run(eng, base, packed, form), _run(eng, base, wide, form)
        assert torch.isfinite(lat_w).all() and torch.equal(lat_p, lat_w), (form, (lat_p - lat_w).abs().max().item())
    part = dict(base, strength=0.6, noise={**base["noise"], "image": torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(77)),
                                           "steps": inp["noise"]["steps"][:4]})
    for form in FORMS:
        lat_p, lat_w = _run(eng, part, packed, form), _run(eng, part, wide, form)
        assert torch.isfinite(lat_w).all() and torch.equal(lat_p, lat_w), ("strength 0.6", form)
    assert not torch.equal(lat_w, _run(eng, base, wide, "serial_eager"))


@DTYPES
def test_encode_garment_e4m3_is_the_packed_native_cache_at_half_the_bytes(dtype):
    from tests.test_garment_packed_cpu import _same
    steps = 7
    eng, inp, _ = _engine(dtype, 2, steps)
    n0 = eng.stats["garment_batches"]
    native = eng.encode_garment(num_inference_steps=steps, **_garment_kw(inp))
    n1 = eng.stats["garment_batches"]
    packed = eng.encode_garment(num_inference_steps=steps, storage="e4m3", **_garment_kw(inp))
    assert eng.stats["garment_batches"] - n1 == n1 - n0 == 3
    assert packed.nbytes == native.nbytes // 2 + packed.exps.numel() * 4 and tuple(packed.exps.shape) == (2, len(native.kv), 2)
    assert "e4m3-packed" in repr(packed) and packed.timesteps == native.timesteps and packed.weights_id == native.weights_id
    assert _same(packed.to("cpu"), native.pack().to("cpu"))
    with pytest.raises(ValueError, match="storage='fp4'"):
        eng.encode_garment(num_inference_steps=steps, storage="fp4", **_garment_kw(inp))
    eng8, inp8, _ = _engine(torch.float16, 2, 3, unet_kw=dict(attn_fp8=True))
    with pytest.raises(ValueError, match="attn_fp8 engine's cache cannot be packed"):
        eng8.encode_garment(num_inference_steps=3, storage="e4m3", **_garment_kw(inp8))


def test_a_garment_swapped_in_place_under_captured_graphs():
    """Two graph-form calls on one packed pool cache with a `put` between them: the second equals a fresh engine's call on the swapped cache
    built apart, the first did not change, and no graph state was added (bytes and exponents moved in place)."""
    from idm_vton_amd.garment_cache import GarmentCache
    steps = 3
    eng, inp, _ = _engine(torch.float16, 4, steps)
    enc = lambda e, sl: e.encode_garment(num_inference_steps=steps, storage="e4m3", cloth=inp["cloth"][sl], text_embeds_cloth=inp["text_embeds_cloth"][sl],
                                         noise_cloth=inp["noise"]["cloth"][sl])
    pool, other = enc(eng, slice(0, 3)), enc(eng, slice(3, 4))
    base = _base(inp, steps)
    fresh, _, _ = _engine(torch.float16, 4, steps)
    before = GarmentCache.cat([pool.select([0]), pool.select([1]), pool.select([2])])
    swapped = GarmentCache.cat([pool.select([0]), other, pool.select([2])])
    ref_before, ref_after = _run(fresh, base, before, "serial_eager", IDX), _run(fresh, base, swapped, "serial_eager", IDX)
    assert not torch.equal(ref_before, ref_after)
    for form in ("graph", "graph_overlap"):
        assert torch.equal(_run(eng, base, pool, form, IDX), ref_before), form
    states, graphs = len(eng._graphs), sum(len(g["graphs"]) for g in eng._graphs.values())
    ptrs = [k.data_ptr() for k, _ in pool.kv] + [pool.exps.data_ptr()]
    pool.put(1, other)
    assert ptrs == [k.data_ptr() for k, _ in pool.kv] + [pool.exps.data_ptr()]
    for form in ("graph", "graph_overlap"):
        assert torch.equal(_run(eng, base, pool, form, IDX), ref_after), form
    assert len(eng._graphs) == states and sum(len(g["graphs"]) for g in eng._graphs.values()) == graphs
    pool.put(1, before.take(1).unpack())                 # a 16-bit source is packed on the device, then moved in
    assert torch.equal(_run(eng, base, pool, "graph_overlap", IDX), ref_before)


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
    eng, inp, m = _engine(torch.float16, 2, steps)
    o_t, o_g, o_v = m["oracle"]
    tr = {}
    opipe.run(o_t, o_g, o_v, Scheduler("ddpm"), num_inference_steps=steps, guidance_scale=2.0, trace=tr, **inp)
    native = eng.encode_garment(num_inference_steps=steps, **_garment_kw(inp))
    packed = eng.encode_garment(num_inference_steps=steps, storage="e4m3", **_garment_kw(inp))
    base = _base(inp, steps)
    for form in ("serial_eager", "graph_overlap"):
        lat_n, lat_p = _run(eng, base, native, form), _run(eng, base, packed, form)
        e_n, e_p = pu.relerr(lat_n, tr["step_latents"][-1]), pu.relerr(lat_p, tr["step_latents"][-1])
        print(f"{form}: latents against the oracle: packed {e_p:.3e}, 16-bit cache {e_n:.3e}")
        assert torch.isfinite(lat_p).all() and not torch.equal(lat_p, lat_n), form
        assert e_p <= PACKED_ORACLE_BAR, (form, e_p, e_n)


def test_boundary_pipeline_encodes_and_takes_a_packed_cache():
    """pipe.encode_garment(..., storage="e4m3") and pipe(cloth=<packed>, garment_index=...) against the engine-level call on the same draws."""
    import torch.nn.functional as F  # noqa: F401
    from idm_vton_amd import config as pc
    from idm_vton_amd.boundary.scheduler import DDPMScheduler
    from idm_vton_amd.boundary.vae import AutoencoderKL
    from idm_vton_amd.garment_cache import PackedGarmentCache
    from src.tryon_pipeline import StableDiffusionXLInpaintPipeline
    from src.unet_hacked_garmnet import UNet2DConditionModel as G
    from src.unet_hacked_tryon import UNet2DConditionModel as T
    from tests import parity_utils as pu
    from tests.test_garment_cache_gpu import _FakeCLIPVision
    DT = torch.float16
    kw = dict(pu.TINY)
    tcfg = pc.UNetConfig(mode="tryon", in_channels=13, sample_size=16, **kw)
    gcfg = pc.UNetConfig(mode="garmnet", in_channels=4, addition_embed_type=None, encoder_hid_dim_type=None, sample_size=16, **kw)
    vcfg = pc.VAEConfig(**pu.TINY_VAE)
    rnd = lambda sd: {k: v.to(DT) for k, v in sd.items()}
    t = T(tcfg, torch_dtype=DT); t.load_state_dict(rnd(pc.random_state_dict(pc.unet_param_shapes(tcfg), 1, torch.float32, "cpu")))
    g = G(gcfg, torch_dtype=DT); g.load_state_dict(rnd(pc.random_state_dict(pc.unet_param_shapes(gcfg), 2, torch.float32, "cpu")))
    v = AutoencoderKL(vcfg, torch_dtype=DT); v.load_state_dict(rnd(pc.random_state_dict(pc.vae_param_shapes(vcfg), 3, torch.float32, "cpu", std=0.05)))
    torch.manual_seed(5)
    enc = _FakeCLIPVision(kw["encoder_hid_dim"]).to(DT)
    pipe = StableDiffusionXLInpaintPipeline(vae=v, text_encoder=None, text_encoder_2=None, tokenizer=None, tokenizer_2=None, unet=t,
                                            unet_encoder=g, scheduler=DDPMScheduler(), image_encoder=enc).to(DEV)
    B, H, W, steps = 2, 128, 128, 3
    inp = pu.make_inputs(B, H, W, kw["cross_attention_dim"], 64, kw["encoder_hid_dim"], steps, DT)
    clip_pix = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(9))
    call = dict(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"],
                pooled_prompt_embeds=inp["pooled_prompt_embeds"], negative_pooled_prompt_embeds=inp["negative_pooled_prompt_embeds"],
                num_inference_steps=steps, strength=1.0, pose_img=inp["pose_img"], mask_image=inp["mask_image"], image=inp["image"],
                height=H, width=W, guidance_scale=2.0, ip_adapter_image=clip_pix, output_type="pt")
    cache = pipe.encode_garment(inp["cloth"], inp["text_embeds_cloth"], steps, H, W, generator=torch.Generator(DEV).manual_seed(11), storage="e4m3")
    assert isinstance(cache, PackedGarmentCache) and cache.G == B and len(cache.timesteps) == steps
    index = [1, 1]
    torch.manual_seed(123)                                                         # the pose posterior uses the GLOBAL generator
    img_c = pipe(generator=torch.Generator(DEV).manual_seed(7), cloth=cache, text_embeds_cloth=None, garment_index=index, **call)[0]
    eng = pipe.hip_engine()
    gen = torch.Generator(DEV).manual_seed(7)
    torch.manual_seed(123)
    draw = lambda gg, dt_: torch.randn((B, 4, H // 8, W // 8), generator=gg, device=DEV, dtype=dt_).float()
    n_lat, n_masked, n_pose, _dropped = draw(gen, DT), draw(gen, torch.float32), draw(None, torch.float32), draw(gen, torch.float32)
    n_steps = torch.stack([draw(gen, DT) for _ in range(steps)])
    with torch.no_grad():
        pos = enc(clip_pix.to(DEV, DT), output_hidden_states=True).hidden_states[-2]
        neg = enc(torch.zeros_like(clip_pix).to(DEV, DT), output_hidden_states=True).hidden_states[-2]
    ref = eng(image=inp["image"], mask_image=inp["mask_image"], pose_img=inp["pose_img"], cloth=cache, garment_index=index,
              prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"],
              pooled_prompt_embeds=inp["pooled_prompt_embeds"], negative_pooled_prompt_embeds=inp["negative_pooled_prompt_embeds"],
              text_embeds_cloth=None, noise=dict(latents=n_lat, masked=n_masked, pose=n_pose, cloth=None, steps=n_steps),
              num_inference_steps=steps, guidance_scale=2.0, ip_hidden_states=torch.cat([neg, pos]), scheduler="ddpm")
    assert torch.isfinite(img_c).all() and torch.equal(img_c, ref)
    other = eng(image=inp["image"], mask_image=inp["mask_image"], pose_img=inp["pose_img"], cloth=cache, garment_index=[0, 1],
                prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"],
                pooled_prompt_embeds=inp["pooled_prompt_embeds"], negative_pooled_prompt_embeds=inp["negative_pooled_prompt_embeds"],
                text_embeds_cloth=None, noise=dict(latents=n_lat, masked=n_masked, pose=n_pose, cloth=None, steps=n_steps),
                num_inference_steps=steps, guidance_scale=2.0, ip_hidden_states=torch.cat([neg, pos]), scheduler="ddpm")
    assert not torch.equal(other, ref)
