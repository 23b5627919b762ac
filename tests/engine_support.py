"""What the GPU tests share: the cached tiny model and the engine / input / call builders of the garment tests, the attention and kv-kernel
operand builders, the garments of three sizes with their per-person oracle, and the boundary pipeline (`StableDiffusionXLInpaintPipeline`
on the tiny weights, the reference's draw order, the CLIP stand-ins).  Importing this module touches no GPU: collection works without one.
The host side (marks, constants, synthetic caches, comparisons) is tests/garment_support.py."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from tests.garment_support import FINITE, FORMS, HEADS

DEV = "cuda"


def no_tune_table(monkeypatch):
    """tune = 0 reaches the library's own rule, whatever the committed table holds for a shape, and every other tune value is passed
    explicitly.  (The table's key carries nk, which differs between a ragged launch -- the capacity -- and its reference -- a person's count.)"""
    from idm_vton_amd import ops
    monkeypatch.setattr(ops, "_TUNE", {"gemm": {}, "attn": {}})


# ------------------------------------------------------------------------------------------------------------------ attention operands
def randn(*shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dtype).to(DEV)


def int_table(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def nan_out(B, Nq, Cc, dtype):
    return torch.full((B, Nq, Cc), float("nan"), dtype=dtype, device=DEV)


def self_attn_operands(P, G, Nq, nkg, dtype, seed):
    """Two-segment SELF launch of B = 2P query batches: own tokens + a garment segment from batch P on, held for G garments."""
    from tests.kernel_checks import _key_order_padded
    B, Cc = 2 * P, HEADS * 64
    q = randn(B, Nq, Cc, dtype=dtype, seed=seed)
    k1, v1 = randn(B, Nq, Cc, dtype=dtype, seed=seed + 1), randn(B, Nq, Cc, dtype=dtype, seed=seed + 2)
    k2, v2 = randn(G, nkg, Cc, dtype=dtype, seed=seed + 3), randn(G, nkg, Cc, dtype=dtype, seed=seed + 4)
    return q, k1, v1, k2, v2, _key_order_padded


def f8_operands(P, G, Nq, nkg, dtype, seed):
    from idm_vton_amd import ops
    q, k1, v1, k2, v2, ko = self_attn_operands(P, G, Nq, nkg, dtype, seed)
    B, Cc = 2 * P, HEADS * 64
    q8 = ops.quant_f8((q.float() * ops.QSCALE).to(dtype).view(B * Nq, Cc), 4.0)

    def seg(kx, vx, nk):
        Bx = kx.shape[0]
        k8 = ops.quant_f8(kx.view(Bx * nk, Cc), 4.0)
        vt16, ld16 = ko(vx, nk)
        vt8 = ops.quant_f8(vt16.view(Bx * Cc, ld16)[:, :ops.round16(nk)], 4.0, mode=1)
        return k8, vt8
    return q8, seg(k1, v1, Nq), seg(k2, v2, nkg)


# ------------------------------------------------------------------------------------------------------------------ kv kernel operands
# (rows, cols, source row stride, destination row stride, exponent): unequal work -- 1 to 20600 16-byte items, so most blocks of the grid's
# x extent find nothing to do for most descriptors --, a gap in the source rows, in the destination rows, in both, and a V^T-shaped run
RUNS = [(1, 16, 16, 16, -7), (37, 80, 96, 88, -1), (200, 1280, 1280, 1280, 0), (3 * 128, 208, 208, 224, 6), (515, 640, 640, 640, 15)]
# destinations: (rows, width, row stride) in 16-bit elements; runs: ("d", rows, cols, source row stride, exponent, destination, first column)
# or ("z", rows, cols, destination, first column), cols in elements
MIXED_DSTS = [(5, 112, 128), (70, 256, 256), (33, 512, 520)]
MIXED_RUNS = [("d", 5, 48, 64, -3, 0, 0),                # a compact run into the front of a wider destination ...
              ("z", 5, 64, 0, 48),                       # ... and the zero tail behind it: together they cover its 112 columns
              ("d", 70, 256, 256, 5, 1, 0),              # 1120 items when widening: one full chunk and one partial chunk
              ("z", 33, 512, 2, 0)]                      # 1056 items when widening


def e4m3_bytes(rows, cols, seed):
    """Random finite e4m3 bytes; the first 254 of a run that has room for them are all 254 finite values."""
    b = FINITE[torch.randint(0, 254, (rows * cols,), generator=torch.Generator().manual_seed(seed))]
    if rows * cols >= 254:
        b[:254] = FINITE
    return b.reshape(rows, cols)


def assert_bits(got, ref, b, what):
    """torch.equal on the bit patterns, naming the first elements that differ: (row, column), source byte, bits written, bits expected."""
    from tests import frames
    g, r = frames.ints(got.cpu().contiguous()), frames.ints(ref.cpu().contiguous())
    bad = torch.nonzero(g != r)
    first = [(int(i), int(j), hex(int(b[i, j])), hex(int(g[i, j]) & 0xffff), hex(int(r[i, j]) & 0xffff)) for i, j in bad[:8].tolist()]
    assert bad.numel() == 0, f"{what}: {bad.shape[0]} element(s) differ; (row, column, byte, got, expected) of the first: {first}"


def pin_frame(view):
    """A framed CPU view (tests/frames.py) -> the same frame in page-locked memory."""
    from tests import frames
    fr = view._frame
    buf = fr.buf.pin_memory()
    v = buf.as_strided(view.shape, view.stride(), view.storage_offset())
    v._frame = frames._Frame(buf, fr.start, fr.shape, fr.ld, fr.interior_bits)
    assert v.is_pinned()
    return v


def check_fill(dsts, runs, outs, srcs, vals, dtype, copy=False):
    """The destinations of one idmvton_kv_fill / idmvton_kv_place table of data and zero runs: all written, frames intact, sources untouched,
    data runs the format's bits (widening) or the source's (copying), zero runs 0x0000."""
    from idm_vton_amd.garment_cache import unpack_values
    from tests import frames
    for d, o in enumerate(outs):
        frames.assert_all_written(o, f"destination {d}")
        frames.assert_frame_intact(o, f"destination {d}")    # guard bands and the gap columns [width, ld)
    for i, run in enumerate(runs):
        if run[0] == "z":
            _, rows, cols, d, c0 = run
            got = frames.ints(outs[d][:rows, c0:c0 + cols].cpu().contiguous())
            assert (got == 0).all(), f"run {i}: a zero run's bits are 0x0000, got {sorted(set(got.flatten().tolist()))[:4]}"
            continue
        _, rows, cols, lds, e, d, c0 = run
        frames.assert_untouched(srcs[i], f"run {i} source")
        got = outs[d][:rows, c0:c0 + cols]
        if copy:
            assert torch.equal(frames.ints(got.cpu().contiguous()), frames.ints(vals[i])), f"run {i}: not the source's bits"
        else:
            assert_bits(got, unpack_values(vals[i], torch.tensor(e), dtype), vals[i], f"run {i}: not the format's bits")


# ------------------------------------------------------------------------------------------------------------------ model, engine, calls
@functools.lru_cache(maxsize=None)
def _built(dtype, fp8):
    from tests import parity_utils as pu
    return pu.build("tiny", dtype, DEV, unet_kw=dict(attn_fp8=True) if fp8 else None)


def model(dtype, fp8=False):
    """One tiny model (oracle + product) per storage dtype and attention variant, shared by every test that does not alter it: parity_utils.build
    is fully seeded and a call changes no weight.  Engines are made per test (`engine`)."""
    return _built(dtype, bool(fp8))


def engine(m, dtype):
    from idm_vton_amd.pipeline import TryonEngine
    return TryonEngine(*m["product"], dtype, DEV)


def inputs(m, B, H, W, Hg, Wg, steps, dtype):
    """parity_utils.make_inputs with a cloth image (and its posterior draw) of another size."""
    from tests import parity_utils as pu
    inp = pu.make_inputs(B, H, W, m["xd"], m["pooled"], m["enc_dim"], steps, dtype)
    if (Hg, Wg) != (H, W):
        g = torch.Generator().manual_seed(1000 + Hg + Wg)
        inp["cloth"] = torch.randn(B, 3, Hg, Wg, generator=g).clamp(-1, 1)
        inp["noise"]["cloth"] = torch.randn(B, 4, Hg // 8, Wg // 8, generator=g)
    return inp


def engine_inputs(dtype, B, steps, fp8=False, H=128, W=128):
    """-> (a new engine on the cached model, fresh inputs of B persons, the model)."""
    m = model(dtype, fp8)
    return engine(m, dtype), inputs(m, B, H, W, H, W, steps, dtype), m


def garment_kw(inp, G=None):
    return dict(cloth=inp["cloth"][:G], text_embeds_cloth=inp["text_embeds_cloth"][:G], noise_cloth=inp["noise"]["cloth"][:G])


def base_call(inp, steps, scheduler="ddpm"):
    """The keywords of a call on a cache: the garment's own inputs dropped."""
    return dict(num_inference_steps=steps, guidance_scale=2.0, scheduler=scheduler, **{**inp, "text_embeds_cloth": None, "noise": {**inp["noise"], "cloth": None}})


def run_on(eng, base, cache, form, index=None, transport="kernel"):
    return eng.denoise(eng.prepare(**{**base, "cloth": cache, "garment_index": index}), host_transport=transport, **FORMS[form]).clone()


def pair(eng, kw, cache, form):
    """Uncached and cached denoise of one call in one execution form.  The person-side VAE encodes of the cached prepare() ran at another
    encoder batch size (2B images instead of 3B), which is not what is under test: start latents and conditioning are copied over."""
    st = eng.prepare(**kw)
    st_c = eng.prepare(**{**kw, "cloth": cache, "text_embeds_cloth": None, "noise": {**kw["noise"], "cloth": None}})
    st_c["latents"].copy_(st["latents"])
    st_c["cond"].copy_(st["cond"])
    assert st_c["timesteps"] is not None and len(st_c["timesteps"]) == len(st["timesteps"])
    return eng.denoise(st, **FORMS[form]).clone(), eng.denoise(st_c, **FORMS[form]).clone()


def to_host(cache, features=False):
    """A device-resident cache -> its copy in page-locked host memory."""
    h = cache.to("cpu", pin_memory=True)
    assert h.host_resident and not cache.host_resident and all(t.is_pinned() for e in h.kv for t in e)
    assert h.features == features and (not h.packed or h.exps.is_pinned())
    return h


# ------------------------------------------------------------------------------------------------------------------ garments of three sizes
STEPS, H, W, P = 3, 128, 128, 3
GARMENT_HW = [(64, 96), (128, 128), (72, 40)]            # A, B, C: latent 8x12, 16x16 (the slot's), 9x5 (odd: padded token rows)
WEARS = [2, 0, 1]                                        # person i wears garment WEARS[i]
KEYS = ["g0", "g1", "g2"]                                # the three garments as a shelf names them


@functools.lru_cache(maxsize=None)
def three_garments(dtype):
    """Persons' inputs (the garment keys dropped: every call on them is on a cache) and the three garments' own inputs."""
    from tests import parity_utils as pu
    m = model(dtype)
    inp = pu.make_inputs(P, H, W, m["xd"], m["pooled"], m["enc_dim"], STEPS, dtype)
    g = torch.Generator().manual_seed(77)
    garments = [dict(cloth=torch.randn(1, 3, hg, wg, generator=g).clamp(-1, 1), noise_cloth=torch.randn(1, 4, hg // 8, wg // 8, generator=g),
                     text_embeds_cloth=inp["text_embeds_cloth"][j:j + 1]) for j, (hg, wg) in enumerate(GARMENT_HW)]
    return inp, garments


def encode_three(eng, garments, which=(0, 1, 2), storage="native"):
    return [eng.encode_garment(num_inference_steps=STEPS, height=H, width=W, storage=storage, **garments[j]) for j in which]


def slotted_pool(eng, ones, hw=(H, W)):
    pool = eng.empty_garment_cache(len(ones), hw[0], hw[1], STEPS, height=H, width=W)
    for s, one in enumerate(ones):
        pool.put(s, one)
    return pool


def gpu_shelf(eng, ones, storage, keys=KEYS):
    from idm_vton_amd.garment_cache import GarmentShelf
    made = GarmentShelf(eng.empty_garment_cache(1, H, W, STEPS, height=H, width=W), storage=storage)
    for key, one in zip(keys, ones):
        made.add(key, one)
    assert all(t.is_pinned() for p in made._parts.values() for e in p.kv for t in e)
    if storage.startswith("features"):
        assert all(p.features and p.packed == storage.endswith("e4m3") and (not p.packed or p.exps.is_pinned()) for p in made._parts.values())
    return made


@functools.lru_cache(maxsize=None)
def oracle_latents(dtype):
    """oracle.pipeline.run on each person alone (B = 1) with the cloth that person wears: the final latents, computed once per dtype."""
    from oracle import pipeline as opipe
    from oracle.scheduler import Scheduler
    o_t, o_g, o_v = model(dtype)["oracle"]
    inp, garments = three_garments(dtype)
    out = []
    for i, j in enumerate(WEARS):
        one = {k: v[i:i + 1] for k, v in inp.items() if k not in ("noise", "ip_hidden_states", "cloth", "text_embeds_cloth")}
        one["ip_hidden_states"] = torch.cat([inp["ip_hidden_states"][i:i + 1], inp["ip_hidden_states"][P + i:P + i + 1]])
        one["noise"] = {k: (v[:, i:i + 1] if k == "steps" else v[i:i + 1]) for k, v in inp["noise"].items() if k != "cloth"}
        one["noise"]["cloth"] = garments[j]["noise_cloth"]
        one.update(cloth=garments[j]["cloth"], text_embeds_cloth=garments[j]["text_embeds_cloth"])
        tr = {}
        with torch.no_grad():
            opipe.run(o_t, o_g, o_v, Scheduler("ddpm"), num_inference_steps=STEPS, guidance_scale=2.0, trace=tr, **one)
        out.append(tr["step_latents"][-1])
    return out


# ------------------------------------------------------------------------------------------------------------------ boundary
class FakeCLIPVision(torch.nn.Module):
    """Stand-in for CLIPVisionModelWithProjection: deterministic 257-token hidden states from the pixels."""

    def __init__(self, dim):
        super().__init__()
        self.proj = torch.nn.Linear(3, dim)

    def forward(self, pixel_values, output_hidden_states=False):
        p = F.adaptive_avg_pool2d(pixel_values.float(), (16, 16)).flatten(2).transpose(1, 2)            # [B,256,3]
        t = torch.cat([p.mean(1, keepdim=True), p], dim=1)
        h = self.proj(t.to(self.proj.weight.dtype))
        return SimpleNamespace(hidden_states=[h * 0.5, h, h * 2.0], image_embeds=h[:, 0])


def boundary_pipeline(dtype, image_encoder=True):
    """-> (pipe, enc, kw): StableDiffusionXLInpaintPipeline on "cuda" over the three boundary models with the tiny weights of
    parity_utils.build (state-dict seeds 1, 2, 3, rounded to `dtype`), the CLIP stand-in drawn under torch.manual_seed(5) (None without
    `image_encoder`), and the tiny configuration's keywords."""
    from idm_vton_amd import config as pc
    from idm_vton_amd.boundary.scheduler import DDPMScheduler
    from idm_vton_amd.boundary.vae import AutoencoderKL
    from src.tryon_pipeline import StableDiffusionXLInpaintPipeline
    from src.unet_hacked_garmnet import UNet2DConditionModel as G
    from src.unet_hacked_tryon import UNet2DConditionModel as T
    from tests import parity_utils as pu
    kw = dict(pu.TINY)
    tcfg = pc.UNetConfig(mode="tryon", in_channels=13, sample_size=16, **kw)
    gcfg = pc.UNetConfig(mode="garmnet", in_channels=4, addition_embed_type=None, encoder_hid_dim_type=None, sample_size=16, **kw)
    vcfg = pc.VAEConfig(**pu.TINY_VAE)
    rnd = lambda sd: {k: v.to(dtype) for k, v in sd.items()}
    t = T(tcfg, torch_dtype=dtype); t.load_state_dict(rnd(pc.random_state_dict(pc.unet_param_shapes(tcfg), 1, torch.float32, "cpu")))
    g = G(gcfg, torch_dtype=dtype); g.load_state_dict(rnd(pc.random_state_dict(pc.unet_param_shapes(gcfg), 2, torch.float32, "cpu")))
    v = AutoencoderKL(vcfg, torch_dtype=dtype); v.load_state_dict(rnd(pc.random_state_dict(pc.vae_param_shapes(vcfg), 3, torch.float32, "cpu", std=0.05)))
    enc = None
    if image_encoder:
        torch.manual_seed(5)
        enc = FakeCLIPVision(kw["encoder_hid_dim"]).to(dtype)
    pipe = StableDiffusionXLInpaintPipeline(vae=v, text_encoder=None, text_encoder_2=None, tokenizer=None, tokenizer_2=None, unet=t,
                                            unet_encoder=g, scheduler=DDPMScheduler(), image_encoder=enc).to(DEV)
    return pipe, enc, kw


def boundary_inputs(kw, B, H, W, steps, dtype, inp=None):
    """-> (inp, clip_pix, call): parity_utils.make_inputs for the tiny configuration `kw` (or the caller's `inp`), the CLIP pixels (seed 9)
    and the keywords of a pipe(...) call without its garment (`cloth`, `text_embeds_cloth`) and its generator."""
    from tests import parity_utils as pu
    if inp is None:
        inp = pu.make_inputs(B, H, W, kw["cross_attention_dim"], 64, kw["encoder_hid_dim"], steps, dtype)
    clip_pix = torch.randn(B, 3, 224, 224, generator=torch.Generator().manual_seed(9))
    call = dict(prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"],
                pooled_prompt_embeds=inp["pooled_prompt_embeds"], negative_pooled_prompt_embeds=inp["negative_pooled_prompt_embeds"],
                num_inference_steps=steps, strength=1.0, pose_img=inp["pose_img"], mask_image=inp["mask_image"], image=inp["image"],
                height=H, width=W, guidance_scale=2.0, ip_adapter_image=clip_pix, output_type="pt")
    return inp, clip_pix, call


def reference_draws(gen_seed, global_seed, B, H, W, steps, dtype):
    """The noise of a pipe(...) call at strength 1 in the reference's draw order -> (the generator after the draws, the
    engine's `noise` dict).  Dtypes as the reference draws them (randn_tensor): latents in the prompt dtype, VAE posterior samples in fp32
    (upcast VAE; the pose posterior from the GLOBAL generator), DDPM variance noise in the model-output dtype.  `cloth` is the cloth
    posterior's draw at the person's latent size: a call on a cache makes and drops it."""
    gen = torch.Generator(DEV).manual_seed(gen_seed)
    torch.manual_seed(global_seed)
    draw = lambda gg, dt_: torch.randn((B, 4, H // 8, W // 8), generator=gg, device=DEV, dtype=dt_).float()
    n_lat, n_masked, n_pose, n_cloth = draw(gen, dtype), draw(gen, torch.float32), draw(None, torch.float32), draw(gen, torch.float32)
    n_steps = torch.stack([draw(gen, dtype) for _ in range(steps)])
    return gen, dict(latents=n_lat, masked=n_masked, pose=n_pose, cloth=n_cloth, steps=n_steps)


def ip_states(enc, clip_pix):
    """The penultimate hidden states of the CLIP stand-in -> (unconditional: of zero pixels, conditional)."""
    dtype = enc.proj.weight.dtype
    with torch.no_grad():
        pos = enc(clip_pix.to(DEV, dtype), output_hidden_states=True).hidden_states[-2]
        neg = enc(torch.zeros_like(clip_pix).to(DEV, dtype), output_hidden_states=True).hidden_states[-2]
    return neg, pos


def engine_reference(eng, inp, noise, ip, steps, **kw):
    """The engine-level call of the boundary tests on a cache: the persons' inputs of `inp`, the reference's draws with the cloth draw
    dropped, `ip` = (unconditional, conditional) hidden states; `kw`: cloth=<cache> and, where the test has one, garment_index."""
    return eng(image=inp["image"], mask_image=inp["mask_image"], pose_img=inp["pose_img"],
               prompt_embeds=inp["prompt_embeds"], negative_prompt_embeds=inp["negative_prompt_embeds"],
               pooled_prompt_embeds=inp["pooled_prompt_embeds"], negative_pooled_prompt_embeds=inp["negative_pooled_prompt_embeds"],
               text_embeds_cloth=None, noise={**noise, "cloth": None},
               num_inference_steps=steps, guidance_scale=2.0, ip_hidden_states=torch.cat(ip), scheduler="ddpm", **kw)


def mk_attn(query_dim, cross_dim, heads, processor, seed, dtype=torch.float16):
    from idm_vton_amd.boundary.modules import Attention
    torch.manual_seed(seed)
    a = Attention(query_dim, cross_dim, heads, 64, processor=processor).to(DEV, dtype)
    return a


# ------------------------------------------------------------------------------------------------------------------ CLIP
def clip_text(hidden, heads, layers, act, proj, vocab=1000, eos=999, seed=0):
    from transformers import CLIPTextConfig, CLIPTextModel, CLIPTextModelWithProjection
    torch.manual_seed(seed)
    cfg = CLIPTextConfig(vocab_size=vocab, hidden_size=hidden, intermediate_size=4 * hidden, num_hidden_layers=layers, num_attention_heads=heads,
                         max_position_embeddings=77, projection_dim=proj or 64, hidden_act=act, bos_token_id=vocab - 2, eos_token_id=eos, pad_token_id=eos)
    m = (CLIPTextModelWithProjection if proj else CLIPTextModel)(cfg).eval()
    with torch.no_grad():                                  # default init is tiny (std 0.02): widen so every op matters numerically
        for n, p in m.named_parameters():
            if p.dim() == 2 and "embedding" not in n:
                p.mul_(3.0)
            if n.endswith("bias"):
                p.normal_(0, 0.1)
    return m


def clip_ids(B, L, vocab, eos, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, vocab - 2, (B, L), generator=g)
    ids[:, 0] = vocab - 2
    for b in range(B):                                      # EOS at a different place per row, padding (== EOS id) after it
        ids[b, 5 + 7 * b:] = eos
    return ids
