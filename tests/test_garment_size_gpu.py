"""-m gpu: the garment at its own resolution.  The reference encodes the cloth image as it is (src/tryon_pipeline.py:1654), runs GarmentNet
on that latent (:1787) and joins the garment tokens to the person's along the token axis only (src/attentionhacked_tryon.py:334,348), so the
garment's token count need not be the person's.  Kernel level: two-segment self-attention whose garment segment is shorter or longer than
the own segment and no multiple of 16, on every kernel `tune` selects, against fp32 SDPA.  Engine level: against the oracle (the bars of
tests/parity_checks.py and tests/kernel_checks.py, imported), cached against uncached (bit for bit), graph states per garment size,
GarmentCache.for_person_size, the fp8 attention variant, and the boundary pipeline."""
import pytest
import torch
import torch.nn.functional as F

from tests.engine_support import DEV, boundary_inputs, boundary_pipeline, engine, garment_kw, inputs, model, pair, randn
from tests.garment_support import DTYPES, FORMS, HEADS
from tests.kernel_checks import TUNES

pytestmark = pytest.mark.gpu

# (Nq, garment keys): the level-1 / level-2 launches of the engine tests below -- 256 query rows x 15 keys (person 256x256, cloth 72x40),
# 64 x 6 (person 128x128, cloth 72x40 at level 1 ... and 64x96 at level 2), 64 x 192 (cloth 256x192: more garment keys than own), 320 x 48
# (query rows that are no multiple of any kernel's workgroup rows)
SHAPES = [(256, 15), (64, 6), (64, 192), (320, 48)]


# ------------------------------------------------------------------------------------------------------------------ kernels
def _garment_segment(G, nkg, dtype, seed):
    """K [G][round16(nkg)][C] and V^T [G][C][round16(nkg)] (key order) as the engine holds them: nkg real tokens, the rows / positions up
    to round16 FINITE FILLER, not zeros (GarmentNet's padded token rows go through the same projections) -- nk must be what masks them."""
    from idm_vton_amd import ops
    Cc, ld = HEADS * 64, ops.round16(nkg)
    k, v = randn(G, ld, Cc, dtype=dtype, seed=seed), randn(G, ld, Cc, dtype=dtype, seed=seed + 1)
    return k, v, ops.key_order(v.transpose(1, 2).contiguous()), ld


@DTYPES
@pytest.mark.parametrize("tune", list(TUNES), ids=list(TUNES))
def test_self_attention_with_a_garment_segment_of_its_own_length(tune, dtype):
    from idm_vton_amd import ops
    from tests.kernel_checks import TOL as KTOL, _key_order_padded
    P = 2
    B, Cc = 2 * P, HEADS * 64
    sp = lambda t: t.float().view(t.shape[0], t.shape[1], HEADS, 64).transpose(1, 2)
    for Nq, nkg in SHAPES:
        q = randn(B, Nq, Cc, dtype=dtype, seed=Nq + nkg)
        k1, v1 = randn(B, Nq, Cc, dtype=dtype, seed=Nq + nkg + 1), randn(B, Nq, Cc, dtype=dtype, seed=Nq + nkg + 2)
        vt1, ld1 = _key_order_padded(v1, Nq)
        pres = tune != "auto"                            # kernels 3, 7, 8, 16 need a pre-multiplied q; `auto` runs the library's rule for a raw q
        qq = (q.float() * ops.QSCALE).to(dtype) if pres else q
        own = dict(k=k1, vt=vt1, nk=Nq, ldk=Cc, ldvt=ld1)
        for G in (P, 1):                                 # b0 = P > 0 with one garment per conditional batch; one shared garment (nb = 1)
            k2, v2, vt2, ld2 = _garment_segment(G, nkg, dtype, seed=3 * Nq + G)
            seg = dict(k=k2, vt=vt2, nk=nkg, ldk=Cc, ldvt=ld2, k_rows=ld2, b0=P)
            if G < P:
                seg["nb"] = G
            out = torch.full((B, Nq, Cc), float("nan"), dtype=dtype, device=DEV)
            ops.attention(qq, out, [own, seg], HEADS, tune=TUNES[tune], q_prescaled=pres)
            # fp32 SDPA over [own ; garment] with the unconditional batches' all-zero garment keys / values materialised
            z = torch.zeros(P, HEADS, nkg, 64, device=DEV)
            kg, vg = sp(k2[:, :nkg]).expand(P, -1, -1, -1), sp(v2[:, :nkg]).expand(P, -1, -1, -1)
            kk, vv = torch.cat([sp(k1), torch.cat([z, kg])], dim=2), torch.cat([sp(v1), torch.cat([z, vg])], dim=2)
            ref = F.scaled_dot_product_attention(sp(qq) / (ops.QSCALE if pres else 1.0), kk, vv).transpose(1, 2).reshape(B, Nq, Cc)
            assert torch.isfinite(out).all(), (tune, Nq, nkg, G)
            err = ((out.float() - ref).abs().max() / ref.abs().max()).item()
            print(f"{dtype} {tune} Nq={Nq} garment keys={nkg} G={G}: {err:.3e}")
            assert err <= KTOL[dtype], (tune, Nq, nkg, G, err)


@DTYPES
@pytest.mark.parametrize("Nq,nkg", [(256, 15), (64, 192)])
def test_fp8_self_attention_with_a_garment_segment_of_its_own_length(Nq, nkg, dtype):
    """idmvton_attn_f8 on the same shape class, held to check_attn_f8's stated tolerances (tests/kernel_checks.py::all_checks: 1.2e-1 against
    fp32 SDPA on the unquantised operands, 3e-2 on the dequantised ones)."""
    from tests.kernel_checks import check_attn_f8
    e_full, e_kernel = check_attn_f8(4, HEADS, Nq, dtype, DEV, n_garm=nkg, b0=2)
    print(f"{dtype} Nq={Nq} garment keys={nkg}: {e_full:.3e} (unquantised) {e_kernel:.3e} (kernel only)")
    assert e_full <= 1.2e-1 and e_kernel <= 3e-2, (e_full, e_kernel)


# ------------------------------------------------------------------------------------------------------------------ engine


@torch.no_grad()
def _parity(m, dtype, B, H, W, Hg, Wg, steps, forms=(dict(),)):
    """tests/parity_checks.run's stages C, D, E with the garment at (Hg, Wg): GarmentNet's features at the garment's latent size, TryonNet's
    noise prediction on the oracle's features (the garment_feats= route: reference-shaped [B][Ng][C] of another token count), and the call."""
    from idm_vton_amd import ops
    from oracle import pipeline as opipe
    from oracle.scheduler import Scheduler
    from tests import parity_utils as pu
    o_t, o_g, o_v = m["oracle"]
    p_t, p_g, p_v, p_r = m["product"]
    inp = inputs(m, B, H, W, Hg, Wg, steps, dtype)
    h, w, gh, gw = H // 8, W // 8, Hg // 8, Wg // 8
    res, t = {}, 481
    z_o = o_v.encode_sample(inp["cloth"], inp["noise"]["cloth"]) * o_v.cfg.scaling_factor
    _, f_o = o_g(z_o, t, inp["text_embeds_cloth"])
    tokens = p_g.feature_tokens(gh, gw)
    assert [f.shape[1] for f in f_o] == tokens
    x_g = ops.to_nhwc(z_o.to(DEV).float().contiguous(), dtype, cpad=p_g.cin_pad)
    _, f_p = p_g.forward(x_g, p_g.time_embeddings([t], B)[0], p_g.encode_context(inp["text_embeds_cloth"].to(DEV)), B, gh, gw)
    res["garment_feat_max"] = max(pu.relerr(a[:, :n], b) for a, b, n in zip(f_p, f_o, tokens))
    lmi = torch.randn(2 * B, 13, h, w, generator=torch.Generator().manual_seed(7))
    pe = torch.cat([inp["negative_prompt_embeds"], inp["prompt_embeds"]])
    add_text = torch.cat([inp["negative_pooled_prompt_embeds"], inp["pooled_prompt_embeds"]])
    time_ids = torch.tensor([[H, W, 0, 0, H, W]], dtype=torch.float32).repeat(2 * B, 1)
    ie_o = o_t.encoder_hid_proj(inp["ip_hidden_states"])
    eps_o = o_t(lmi, t, pe, added_cond_kwargs=dict(text_embeds=add_text, time_ids=time_ids, image_embeds=ie_o),
                garment_features=[torch.cat([torch.zeros_like(d), d]) for d in f_o])[0]
    ctx_t = p_t.encode_context(pe.to(DEV), ie_o.to(DEV))
    temb_t = p_t.time_embeddings([t], 2 * B, dict(text_embeds=add_text.to(DEV), time_ids=time_ids.to(DEV)))[0]
    x_t = ops.to_nhwc(lmi.to(DEV).contiguous(), dtype, cpad=p_t.cin_pad)
    eps_p, _ = p_t.forward(x_t, temb_t, ctx_t, 2 * B, h, w, garment_feats=[d.to(DEV, dtype).contiguous() for d in f_o])
    res["tryon_eps"] = pu.relerr(eps_p.view(2 * B, h, w, -1)[..., :4].permute(0, 3, 1, 2), eps_o)
    tr = {}
    img_o = opipe.run(o_t, o_g, o_v, Scheduler("ddpm"), num_inference_steps=steps, guidance_scale=2.0, trace=tr, **inp)
    eng = engine(m, dtype)
    for i, kw in enumerate(forms):
        st = eng.prepare(num_inference_steps=steps, guidance_scale=2.0, scheduler="ddpm", **inp)
        assert (st["gh"], st["gw"]) == (gh, gw) and tuple(st["trace"]["cloth_lat"].shape[-2:]) == (gh, gw)
        lat = eng.denoise(st, **kw)
        sfx = "" if i == 0 else f"_{i}"
        res["cloth_lat" + sfx] = pu.relerr(st["trace"]["cloth_lat"], tr["cloth_lat"])
        res["latents_final" + sfx] = pu.relerr(lat, tr["step_latents"][-1])
        res["image" + sfx] = pu.relerr(eng.decode(lat), img_o)
    return res


@DTYPES
@pytest.mark.parametrize("person,cloth", [((128, 128), (72, 40)), ((128, 128), (64, 96)), ((128, 128), (256, 192)), ((256, 256), (72, 40))],
                         ids=["128_cloth72x40", "128_cloth64x96", "128_cloth256x192", "256_cloth72x40"])
def test_garment_of_another_size_matches_the_oracle(person, cloth, dtype):
    """Garment tokens (level 1, level 2): 72x40 -> 15, 6; 64x96 -> 24, 6; 256x192 -> 192, 48 (more than the 64 / 16 own tokens of a 128x128
    person).  At 256x256 the level-1 launches have 256 query rows -- the software-pipelined kernel's workgroup -- against 15 garment keys."""
    from tests.parity_checks import TOL
    r = _parity(model(dtype), dtype, 1, *person, *cloth, steps=2)
    print(person, cloth, dtype, {k: f"{v:.3e}" for k, v in r.items()})
    t = TOL[dtype]
    assert r["garment_feat_max"] <= t["stage"] and r["tryon_eps"] <= t["stage"] and r["cloth_lat"] <= t["stage"], r
    assert r["latents_final"] <= t["latents"] and r["image"] <= t["image"], r


@pytest.mark.parametrize("scheduler", ["ddpm", "ddim"])
@DTYPES
def test_cached_loop_is_bit_identical_to_the_uncached_loop_at_another_garment_size(dtype, scheduler):
    """Person 128x128, cloth 64x96, B = 2, 7 steps (blocks of 1, 2, 4 timesteps): encode_garment makes the launches the uncached call makes
    -- the cloth's own VAE pass, the same GarmentNet batches at the garment's latent size --, so every execution form reproduces the uncached
    latents exactly; and P = 2 persons on a G = 1 cache (shared segment) equal the cache that holds the garment twice."""
    steps = 7
    m = model(dtype)
    eng, inp = engine(m, dtype), inputs(m, 2, 128, 128, 64, 96, steps, dtype)
    kw = dict(num_inference_steps=steps, guidance_scale=2.0, scheduler=scheduler, **inp)
    cache = eng.encode_garment(num_inference_steps=steps, scheduler=scheduler, height=128, width=128, **garment_kw(inp))
    assert (cache.h, cache.w, cache.gh, cache.gw, cache.G) == (16, 16, 8, 12, 2)
    tokens = m["product"][0].feature_tokens(8, 12)
    assert [vt.shape[2] for _, vt in cache.kv] == [(n + 15) // 16 * 16 for n in tokens]      # round16 rows of the GARMENT's token counts
    for form in FORMS:
        lat_u, lat_c = pair(eng, kw, cache, form)
        print(f"{dtype} {scheduler} {form}: max|cached - uncached| = {(lat_u - lat_c).abs().max().item():.3e}")
        assert torch.isfinite(lat_u).all() and torch.equal(lat_u, lat_c), (form, (lat_u - lat_c).abs().max().item())
    cache1 = eng.encode_garment(num_inference_steps=steps, scheduler=scheduler, height=128, width=128, **garment_kw(inp, 1))
    cache2 = cache1.repeat_garments(2)
    assert (cache2.G, cache2.gh, cache2.gw) == (2, 8, 12)
    base = {**kw, "text_embeds_cloth": None}
    for form in ("serial_eager", "graph_overlap"):
        lats = [eng.denoise(eng.prepare(**{**base, "cloth": c}), **FORMS[form]).clone() for c in (cache1, cache2)]
        assert torch.isfinite(lats[0]).all() and torch.equal(lats[0], lats[1]), form


def test_graph_state_is_kept_per_garment_size():
    """One engine, hipGraph + two-stream overlap, four calls in turn: same-size cloth, 64x96, 256x192, same-size again.  Persistent sets and
    captured graphs are keyed by the garment's size, so each call gives the serial eager result of its own inputs and the last call -- back
    on the first call's state -- its bits."""
    dtype, steps = torch.float16, 5
    m = model(dtype)
    eng = engine(m, dtype)
    sizes = [(128, 128), (64, 96), (256, 192), (128, 128)]
    calls = [dict(num_inference_steps=steps, guidance_scale=2.0, scheduler="ddpm", **inputs(m, 2, 128, 128, Hg, Wg, steps, dtype)) for Hg, Wg in sizes]
    graph = [eng.denoise(eng.prepare(**kw), **FORMS["graph_overlap"]).clone() for kw in calls]
    assert len(eng._graphs) == 3 and len(eng._set_shapes) == 3
    serial = [eng.denoise(eng.prepare(**kw), **FORMS["serial_eager"]).clone() for kw in calls]
    for (Hg, Wg), g, s in zip(sizes, graph, serial):
        assert torch.isfinite(s).all() and torch.equal(g, s), (Hg, Wg, (g - s).abs().max().item())
    assert torch.equal(graph[0], graph[3])
    assert not torch.equal(graph[0], graph[1]) and not torch.equal(graph[1], graph[2])


def test_one_encoded_garment_serves_another_person_size_once_declared():
    """The garment K / V^T do not depend on the person's resolution: a cache encoded from a 64x96 cloth and declared for 128x128 serves a
    256x256 call through for_person_size(32, 32), with the latents of the uncached 256x256 call on that cloth (whole call: both encode
    the two person-side images in one 2B pass); undeclared, it is refused."""
    dtype, steps = torch.float16, 3
    m = model(dtype)
    eng = engine(m, dtype)
    small, big = inputs(m, 1, 128, 128, 64, 96, steps, dtype), inputs(m, 1, 256, 256, 64, 96, steps, dtype)
    small["text_embeds_cloth"] = big["text_embeds_cloth"]                          # one garment: the same image, posterior draw and caption
    assert torch.equal(small["cloth"], big["cloth"]) and torch.equal(small["noise"]["cloth"], big["noise"]["cloth"])
    cache = eng.encode_garment(num_inference_steps=steps, height=128, width=128, **garment_kw(small))
    kw = dict(num_inference_steps=steps, guidance_scale=2.0, scheduler="ddpm", return_latents=True)
    with pytest.raises(ValueError, match="GarmentCache resolution mismatch"):
        eng(**kw, **{**big, "cloth": cache, "text_embeds_cloth": None})
    for form in ("serial_eager", "graph_overlap"):
        fk = {k: v for k, v in FORMS[form].items()}
        lat_u = eng(**kw, **fk, **big).clone()
        lat_c = eng(**kw, **fk, **{**big, "cloth": cache.for_person_size(32, 32), "text_embeds_cloth": None}).clone()
        assert torch.isfinite(lat_u).all() and torch.equal(lat_u, lat_c), (form, (lat_u - lat_c).abs().max().item())
    # and it still serves the size it was encoded for
    lat_s = eng(**kw, **{**small, "cloth": cache, "text_embeds_cloth": None})
    assert torch.equal(lat_s, eng(**kw, **small))


def test_fp8_attention_engine_with_a_larger_garment_matches_the_oracle_within_its_stated_tolerance():
    """Cloth 256x192 on a 128x128 person with HipUNet(attn_fp8=True): 192 garment keys at level 1 (whole 64-key tiles: e4m3 straight from
    the projection) against 64 own, 48 at level 2 (projected in 16 bits, quantised per launch) against 16 own.  The bar of
    tests/test_parity_gpu.py::test_fp8_attention_engine_matches_oracle_within_its_stated_tolerance."""
    dtype = torch.float16
    r = _parity(model(dtype, fp8=True), dtype, 2, 128, 128, 256, 192, steps=3, forms=(dict(), dict(use_graph=True, overlap=True)))
    print({k: f"{v:.3e}" for k, v in r.items()})
    assert r["garment_feat_max"] <= 8e-2 and r["tryon_eps"] <= 8e-2 and r["latents_final"] <= 8e-2 and r["latents_final_1"] <= 8e-2, r


# ------------------------------------------------------------------------------------------------------------------ boundary
def test_boundary_pipeline_takes_a_cloth_of_another_size():
    from oracle import pipeline as opipe
    from oracle.scheduler import Scheduler
    from tests import parity_utils as pu
    from tests.parity_checks import TOL
    DT = torch.float16
    pipe, _, kw = boundary_pipeline(DT)
    B, H, W, Hg, Wg, steps = 2, 128, 128, 64, 96, 3
    m = model(DT)                                       # the same seeds and rounding as above: the oracle holds the pipeline's weights
    inp, clip_pix, call = boundary_inputs(kw, B, H, W, steps, DT, inp=inputs(m, B, H, W, Hg, Wg, steps, DT))
    o_t, o_g, o_v = m["oracle"]

    def oracle_of(traced, cloth_lat_noise):
        """The oracle on what crossed the engine boundary in a pipeline call (pipe.trace_call), with the given cloth posterior draw."""
        on_cpu = lambda x: x.detach().float().cpu() if torch.is_tensor(x) else x
        a = {k: on_cpu(traced[k]) for k in ("image", "mask_image", "pose_img", "prompt_embeds", "negative_prompt_embeds", "pooled_prompt_embeds",
                                            "negative_pooled_prompt_embeds", "ip_hidden_states")}
        nz = {k: on_cpu(x) for k, x in traced["noise"].items() if k in ("latents", "masked", "pose", "steps")}
        nz["cloth"] = on_cpu(cloth_lat_noise)
        return opipe.run(o_t, o_g, o_v, Scheduler("ddpm"), cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"], noise=nz,
                         num_inference_steps=steps, guidance_scale=2.0, **a)

    def run(gen_seed, **over):
        gen = torch.Generator(DEV).manual_seed(gen_seed)
        torch.manual_seed(123)                                                     # the pose posterior uses the GLOBAL generator
        pipe.trace_call = {}
        img = pipe(generator=gen, **{**call, **over})[0]
        traced, pipe.trace_call = pipe.trace_call, None
        return img, gen, traced

    # uncached: cloth tensor of another size; its posterior draw has the garment latent's shape
    uncached = dict(cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"])
    img_u, gen_u, tr_u = run(7, **uncached)
    assert tuple(tr_u["noise"]["cloth"].shape) == (B, 4, Hg // 8, Wg // 8) and tuple(img_u.shape) == (B, 3, H, W)
    img_u2, _, _ = run(7, **uncached)
    assert torch.isfinite(img_u).all() and torch.equal(img_u, img_u2)             # reproducible with a seeded generator
    e_u = pu.relerr(img_u, oracle_of(tr_u, tr_u["noise"]["cloth"]))
    # cached: encode_garment (one draw of the garment latent's shape from its own generator), then the cache as `cloth=`
    enc_gen = lambda: torch.Generator(DEV).manual_seed(11)
    cache = pipe.encode_garment(inp["cloth"], inp["text_embeds_cloth"], steps, H, W, generator=enc_gen())
    assert (cache.h, cache.w, cache.gh, cache.gw, cache.G) == (H // 8, W // 8, Hg // 8, Wg // 8, B)
    n_garm = pipe.hip_engine().stats["garment_batches"]
    cached = dict(cloth=cache, text_embeds_cloth=None)
    img_c, gen_c, tr_c = run(7, **cached)
    assert pipe.hip_engine().stats["garment_batches"] == n_garm and tr_c["noise"]["cloth"] is None
    cache2 = pipe.encode_garment(inp["cloth"], inp["text_embeds_cloth"], steps, H, W, generator=enc_gen())
    img_c2, _, _ = run(7, cloth=cache2, text_embeds_cloth=None)
    assert torch.isfinite(img_c).all() and torch.equal(img_c, img_c2)
    n_cloth = torch.randn((B, 4, Hg // 8, Wg // 8), generator=enc_gen(), device=DEV, dtype=torch.float32)     # encode_garment's draw
    e_c = pu.relerr(img_c, oracle_of(tr_c, n_cloth))
    print(f"boundary, cloth {Hg}x{Wg} on {H}x{W}: image vs oracle uncached {e_u:.3e} cached {e_c:.3e}")
    assert e_u <= TOL[DT]["image"] and e_c <= TOL[DT]["image"], (e_u, e_c)
    # the cached call made (and dropped) the cloth draw at the garment latent's shape: same later draws, same final generator state
    assert torch.equal(gen_c.get_state(), gen_u.get_state())
    for k in ("latents", "masked", "steps"):
        assert torch.equal(tr_c["noise"][k], tr_u["noise"][k]), k
    # pose_img is concatenated with the image's latents along channels: another size is still refused; so is a cloth size no multiple of 8
    with pytest.raises(ValueError, match="`pose_img` is"):
        run(7, **uncached, pose_img=inp["pose_img"][..., :Hg, :Wg])
    with pytest.raises(ValueError, match="divisible by 8"):
        run(7, **{**uncached, "cloth": inp["cloth"][..., :60, :]})
