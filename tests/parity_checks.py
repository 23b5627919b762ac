"""Model-level parity: HIP engine (GPU) vs oracle (CPU fp32) on identical weights / inputs / noise.
`run` returns a dict of max-rel errors per stage; used by tests/test_parity_gpu.py and tools/gpu_parity.py.  `reference` is its oracle half
alone (no GPU): tests/test_parity_audit_cpu.py runs it on mutated oracles to show that the bars in `TOL` can hear a wiring defect."""
import torch

from tests import parity_utils as pu


# Bars for err = max|x - ref| / max|ref| per storage dtype (tests/test_parity_gpu.py states where they come from).  `BAR_OF` names the bar each
# compared quantity of `reference()` is held to.
TOL = {torch.float16: dict(stage=4e-3, latents=5e-3, image=1e-2, decode=2e-4),
       torch.bfloat16: dict(stage=3e-2, latents=4e-2, image=6e-2, decode=2e-4)}
BAR_OF = dict(resampler="stage", vae_encode="stage", vae_decode="decode", garment_feats="stage", tryon_eps="stage",
              masked_lat="stage", pose_lat="stage", step_latents="latents", image="image")
T_STAGE = 481                                                  # the timestep of the single-call stages C and D


@torch.no_grad()
def reference(m, inp, B, H, W, steps, scheduler="ddpm", guidance_scale=2.0):
    """The oracle half of `run()`: every tensor a stage compares, from the fp32 CPU oracle alone.
    -> dict(resampler, vae_encode, vae_decode, garment_feats [list], tryon_eps, masked_lat, pose_lat, step_latents [list], image) plus
    `stage_d`: the inputs of the TryonNet stage (lmi, pe, add_text, time_ids), so that the engine can be given the same ones."""
    from oracle import pipeline as opipe
    from oracle.scheduler import Scheduler

    o_t, o_g, o_v = m["oracle"]
    h, w = H // 8, W // 8
    ref = {}
    # ---- A: Resampler (plugin API: unet.encoder_hid_proj) ----
    ie_o = ref["resampler"] = o_t.encoder_hid_proj(inp["ip_hidden_states"])
    # ---- B: VAE encode / decode ----
    z_o = ref["vae_encode"] = o_v.encode_sample(inp["cloth"], inp["noise"]["cloth"]) * o_v.cfg.scaling_factor
    ref["vae_decode"] = o_v.decode(z_o / o_v.cfg.scaling_factor)
    # ---- C: GarmentNet features (same latent in) ----
    _, f_o = o_g(z_o, T_STAGE, inp["text_embeds_cloth"])
    ref["garment_feats"] = f_o
    # ---- D: TryonNet noise prediction (oracle's features in, CFG batch) ----
    g = torch.Generator().manual_seed(7)
    lmi = torch.randn(2 * B, 13, h, w, generator=g)
    pe = torch.cat([inp["negative_prompt_embeds"], inp["prompt_embeds"]])
    add_text = torch.cat([inp["negative_pooled_prompt_embeds"], inp["pooled_prompt_embeds"]])
    time_ids = torch.tensor([[H, W, 0, 0, H, W]], dtype=torch.float32).repeat(2 * B, 1)
    added = dict(text_embeds=add_text, time_ids=time_ids, image_embeds=ie_o)
    feats_cfg = [torch.cat([torch.zeros_like(d), d]) for d in f_o]
    ref["tryon_eps"] = o_t(lmi, T_STAGE, pe, added_cond_kwargs=added, garment_features=feats_cfg)[0]
    ref["stage_d"] = dict(lmi=lmi, pe=pe, add_text=add_text, time_ids=time_ids, feats_cfg=feats_cfg)
    # ---- E: whole pipeline, injected noise ----
    tr = {}
    ref["image"] = opipe.run(o_t, o_g, o_v, Scheduler(scheduler), num_inference_steps=steps, guidance_scale=guidance_scale, trace=tr,
                             **inp)
    ref["masked_lat"], ref["pose_lat"], ref["step_latents"] = tr["masked_lat"][:B], tr["pose_lat"][:B], tr["step_latents"]
    return ref


@torch.no_grad()
def run(kind="tiny", dtype=torch.float16, B=1, H=128, W=128, steps=4, scheduler="ddpm", use_graph=False, device="cuda",
        overlap=False, unet_kw=None, weights="quiet"):
    from idm_vton_amd import ops
    from idm_vton_amd.pipeline import TryonEngine

    m = pu.build(kind, dtype, device, unet_kw=unet_kw, weights=weights)
    p_t, p_g, p_v, p_r = m["product"]
    inp = pu.make_inputs(B, H, W, m["xd"], m["pooled"], m["enc_dim"], steps, dtype)
    h, w = H // 8, W // 8
    ref = reference(m, inp, B, H, W, steps, scheduler)
    o_v = m["oracle"][2]
    res = {}

    # ---- A: Resampler (plugin API: unet.encoder_hid_proj) ----
    ie_o = ref["resampler"]
    ie_p = p_r(inp["ip_hidden_states"])
    res["resampler"] = pu.relerr(ie_p, ie_o)

    # ---- B: VAE encode / decode ----
    img = inp["cloth"]
    z_o = ref["vae_encode"]
    z_p = p_v.encode_sample(img.to(device), inp["noise"]["cloth"].to(device))
    res["vae_encode"] = pu.relerr(z_p, z_o)
    d_p = p_v.decode(z_o.to(device) / o_v.cfg.scaling_factor)
    res["vae_decode"] = pu.relerr(d_p, ref["vae_decode"])

    # ---- C: GarmentNet features (same latent in) ----
    t = T_STAGE
    f_o = ref["garment_feats"]
    ctx_g = p_g.encode_context(inp["text_embeds_cloth"].to(device))
    temb_g = p_g.time_embeddings([t], B)[0]
    x_g = ops.to_nhwc(z_o.to(device).float().contiguous(), dtype, cpad=p_g.cin_pad)
    _, f_p = p_g.forward(x_g, temb_g, ctx_g, B, h, w)
    assert len(f_o) == len(f_p) == p_g.num_features()
    f_p = [f[:, :n] for f, n in zip(f_p, p_g.feature_tokens(h, w))]        # the engine keeps round16(H*W) token rows per image
    errs = [pu.relerr(a, b) for a, b in zip(f_p, f_o)]
    res["garment_feat_first"], res["garment_feat_last"], res["garment_feat_max"] = errs[0], errs[-1], max(errs)

    # ---- D: TryonNet noise prediction (oracle's features in, CFG batch) ----
    sd = ref["stage_d"]
    lmi, pe, add_text, time_ids, feats_cfg = sd["lmi"], sd["pe"], sd["add_text"], sd["time_ids"], sd["feats_cfg"]
    eps_o = ref["tryon_eps"]
    ctx_t = p_t.encode_context(pe.to(device), ie_o.to(device))
    temb_t = p_t.time_embeddings([t], 2 * B, dict(text_embeds=add_text.to(device), time_ids=time_ids.to(device)))[0]
    x_t = ops.to_nhwc(lmi.to(device).contiguous(), dtype, cpad=p_t.cin_pad)
    feats_dev = [d.to(device, dtype).contiguous() for d in f_o]
    eps_p, _ = p_t.forward(x_t, temb_t, ctx_t, 2 * B, h, w, garment_feats=feats_dev)
    eps_p = eps_p.view(2 * B, h, w, -1)[..., :4].permute(0, 3, 1, 2)
    res["tryon_eps"] = pu.relerr(eps_p, eps_o)
    # the same with the zero half materialised (general garment_features= API path, no closed form)
    feats_full = [d.to(device, dtype).contiguous() for d in feats_cfg]
    eps_p2, _ = p_t.forward(x_t, temb_t, ctx_t, 2 * B, h, w, garment_feats=feats_full)
    eps_p2 = eps_p2.view(2 * B, h, w, -1)[..., :4].permute(0, 3, 1, 2)
    res["tryon_eps_materialised_zeros"] = pu.relerr(eps_p2, eps_o)
    res["closed_form_vs_materialised"] = pu.relerr(eps_p, eps_p2)

    # ---- E: whole pipeline, injected noise ----
    tr = dict(masked_lat=ref["masked_lat"], pose_lat=ref["pose_lat"], step_latents=ref["step_latents"])
    img_o = ref["image"]
    eng = TryonEngine(p_t, p_g, p_v, p_r, dtype, device)
    st = eng.prepare(num_inference_steps=steps, guidance_scale=2.0, scheduler=scheduler, **inp)
    res["prep_masked_lat"] = pu.relerr(st["trace"]["masked_lat"], tr["masked_lat"][:B])
    res["prep_pose_lat"] = pu.relerr(st["trace"]["pose_lat"], tr["pose_lat"][:B])
    ptr = {}
    traced = not (use_graph or overlap)
    lat = eng.denoise(st, use_graph=use_graph, trace=ptr if traced else None, overlap=overlap)
    if traced:
        for i, (a, b) in enumerate(zip(ptr["step_latents"], tr["step_latents"])):
            res[f"latents_step{i + 1}"] = pu.relerr(a, b)
    res["latents_final"] = pu.relerr(lat, tr["step_latents"][-1])
    res["image"] = pu.relerr(eng.decode(lat), img_o)
    if overlap:
        # the two-stream form must reproduce the serial form bit for bit (same kernels, same order per stream); run the
        # pipeline a second time through the already-captured graphs as well (persistent-buffer refresh path)
        st2 = eng.prepare(num_inference_steps=steps, guidance_scale=2.0, scheduler=scheduler, **inp)
        lat_serial = eng.denoise(st2, use_graph=False, overlap=False).clone()
        res["overlap_vs_serial"] = pu.relerr(lat, lat_serial)
        st3 = eng.prepare(num_inference_steps=steps, guidance_scale=2.0, scheduler=scheduler, **inp)
        lat_again = eng.denoise(st3, use_graph=use_graph, overlap=True)
        res["overlap_second_call"] = pu.relerr(lat_again, lat_serial)
    return res
