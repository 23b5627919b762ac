"""-m gpu: per-person guidance.  idmvton_guided_step against the fp64 restatement of its formula (tests/guidance_support.formula) on the
same 16-bit eps values -- the bar is MARGIN x the error of a float32 torch evaluation of that formula, measured in the same test, no number
fixed in advance --, its off case and batch invariance bit for bit, its operands in poisoned frames; the attention launches of a call
without unconditional rows (the garment segment from batch 0 on) against fp32 SDPA; and the engine: a mixed batch in the four execution
forms, every step replayed against the formula, uncond="skip" on every cache form a call can take, and the call surface.
Tiny engines: latent 16 x 16, 3 DDPM steps (blocks of 1 and 2 timesteps), B = 3."""
import pytest
import torch
import torch.nn.functional as F

from tests.engine_support import (DEV, H, KEYS, STEPS, W, WEARS, base_call, boundary_inputs, boundary_pipeline, encode_three, engine, engine_inputs,
                                  f8_operands, garment_kw, gpu_shelf, int_table, ip_states, model, nan_out, no_tune_table, reference_draws,
                                  self_attn_operands, slotted_pool, three_garments, to_host)
from tests.frames import Framed, Tight
from tests.garment_support import DTYPES, F8_SDPA_BAR, FORMS, HEADS, TRANSPORTS
from tests.guidance_support import G3, HWS, MARGIN, PHI3, coef_row, emulate_cond_step, errors, operands, replay_eps

pytestmark = pytest.mark.gpu
B = 3
LDCS = pytest.mark.parametrize("ldc", [64, 4], ids=["ldc64_nan", "ldc4"])
HW = pytest.mark.parametrize("hw", HWS)
NOISE = pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "null_noise"])


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _launch(eps, lat, noise, coef, branches=2, al=None):
    """One guided_step on device copies of the CPU operands (through the allocation policy `al`) -> the updated latents."""
    from idm_vton_amd import ops
    al = al or Tight()
    n = lat.shape[0]
    e = al.inp("eps", eps.to(DEV), contig=True)
    x = al.inout("latents", lat.to(DEV).clone(), contig=True)
    nz = al.inp("noise", noise.to(DEV), contig=True) if noise is not None else None
    c = al.inp("coef", coef.to(DEV), contig=True)
    work = al.out("work", (ops.guided_step_work_floats(n, lat.shape[-1]),), torch.float32, DEV, contig=True, scratch=True) if branches == 2 else None
    ops.guided_step(e, x, nz, c, work, branches)
    return x


@DTYPES
@HW
@LDCS
@NOISE
def test_guided_step_against_the_fp64_formula(with_noise, ldc, hw, dtype):
    eps, lat, noise = operands(B, hw, ldc, dtype)
    noise = noise if with_noise else None
    coef = coef_row(G3, PHI3)
    got = _launch(eps, lat, noise, coef)
    assert torch.isfinite(got).all()                      # channels 4.. of an ldc = 64 row are NaN: none was read
    e_k, e_32 = errors(got, eps, lat, noise, coef, 2)
    print(f"guided_step {dtype} hw={hw} ldc={ldc} noise={with_noise}: kernel {e_k:.3e}, float32 torch {e_32:.3e} (bar {MARGIN:g} x = {MARGIN * e_32:.3e})")
    assert e_32 > 0 and e_k <= MARGIN * e_32, (e_k, e_32)


@DTYPES
@HW
@NOISE
def test_conditional_branch_alone(with_noise, hw, dtype):
    """branches 1: e = t whatever g and phi hold, no work buffer; within the bar, and the bits of the fp32 emulation of its arithmetic."""
    eps, lat, noise = operands(B, hw, 64, dtype, branches=1)
    noise = noise if with_noise else None
    coef = coef_row(G3, PHI3)
    got = _launch(eps, lat, noise, coef, branches=1)
    e_k, e_32 = errors(got, eps, lat, noise, coef, 1)
    print(f"guided_step branches=1 {dtype} hw={hw} noise={with_noise}: kernel {e_k:.3e}, float32 torch {e_32:.3e}")
    assert torch.isfinite(got).all() and e_32 > 0 and e_k <= MARGIN * e_32, (e_k, e_32)
    assert torch.equal(got.cpu(), emulate_cond_step(eps, lat, noise, coef))


@DTYPES
@HW
@LDCS
def test_a_person_without_rescale_gets_cfg_steps_bits(ldc, hw, dtype):
    """phi = 0: person 0 of the mixed launch (g = 7.5) and every person of an all-zero-phi launch are bit-equal to ops.cfg_step with that g,
    with and without the noise term."""
    from idm_vton_amd import ops
    eps, lat, noise = operands(B, hw, ldc, dtype)
    for nz in (noise, None):
        mixed = _launch(eps, lat, nz, coef_row(G3, PHI3))
        plain = _launch(eps, lat, nz, coef_row(G3, (0.0, 0.0, 0.0)))
        for b, g in enumerate(G3):
            one = lat[b:b + 1].to(DEV).clone()
            ops.cfg_step(torch.stack([eps[b], eps[B + b]]).to(DEV), one, nz[b:b + 1].to(DEV) if nz is not None else None,
                         torch.tensor([*coef_row(G3, PHI3)[:3].tolist(), g], dtype=torch.float32, device=DEV))
            assert torch.equal(plain[b:b + 1], one), (b, nz is None)
            if PHI3[b] == 0:
                assert torch.equal(mixed[b:b + 1], one), (b, nz is None)
            elif b == 1:
                assert not torch.equal(mixed[b:b + 1], one)      # (and the rescale does something: g = 2, phi = 0.7)


@DTYPES
@HW
def test_a_persons_bits_do_not_depend_on_the_batch(hw, dtype):
    """Person 1 (g = 2, phi = 0.7) of the B = 3 launch, launched alone, and as the last of a batch of 2 in another order."""
    eps, lat, noise = operands(B, hw, 64, dtype)
    full = _launch(eps, lat, noise, coef_row(G3, PHI3))
    alone = _launch(torch.stack([eps[1], eps[B + 1]]), lat[1:2], noise[1:2], coef_row(G3[1:2], PHI3[1:2]))
    assert torch.equal(full[1:2], alone)
    order = [2, 1]
    two = _launch(torch.cat([eps[order], eps[[B + i for i in order]]]), lat[order], noise[order], coef_row([G3[i] for i in order], [PHI3[i] for i in order]))
    assert torch.equal(two[1:2], full[1:2]) and torch.equal(two[0:1], full[2:3])


@DTYPES
@HW
@pytest.mark.parametrize("branches", [2, 1])
def test_guided_step_in_poisoned_frames(branches, hw, dtype):
    """Every operand inside a frame (tests/frames.py): guard bands of latents and `work` intact -- `work` has exactly its stated size --, the
    inputs (eps with NaN in channels 4.., noise, coef) untouched, and the bits of the tight launch."""
    eps, lat, noise = operands(B, hw, 64, dtype, branches=branches)
    coef = coef_row(G3, PHI3)
    framed = Framed()
    got = _launch(eps, lat, noise, coef, branches, framed)
    framed.verify()
    assert torch.isfinite(got).all() and torch.equal(got, _launch(eps, lat, noise, coef, branches))
    if branches == 2:
        from tests import frames
        work = framed.outs["work"]
        written = frames.ints(work) != work._frame.interior_bits
        per = work.numel() // B                              # person 0 has phi = 0: its part of `work` is never written, the others' is, whole
        assert not written[:per].any() and written[per:].all()


def test_pack_input_cond_is_the_conditional_half_of_pack_input():
    from idm_vton_amd import ops
    for dtype in (torch.float16, torch.bfloat16):
        g = torch.Generator().manual_seed(3)
        lat, cond = torch.randn(B, 4, 15, 13, generator=g).to(DEV), torch.randn(2 * B, 195, 9, generator=g).to(dtype).to(DEV)
        framed = Framed()
        both = ops.pack_input(lat, cond, torch.empty(2 * B, 195, 64, dtype=dtype, device=DEV))
        one = ops.pack_input_cond(framed.inp("latents", lat, contig=True), framed.inp("cond", cond[B:].contiguous(), contig=True),
                                  framed.out("packed", (B, 195, 64), dtype, DEV, contig=True))
        framed.verify()
        assert torch.equal(one, both[B:])


# ------------------------------------------------------------------------------------------------------------------ attention at b0 = 0
P, G, NQ, GK, GROWS = 3, 2, 80, 72, 80                    # 72 garment keys in slots of 80 rows
INDEX = [1, 0, 1]


def _sdpa_b0(q, k1, v1, k2, v2):
    """fp32 SDPA of P query batches, each on its own tokens and the GK real keys of garment INDEX[b]."""
    sp = lambda t: t.float().view(t.shape[0], t.shape[1], HEADS, 64).transpose(1, 2)
    kk = torch.cat([sp(k1), sp(k2[INDEX][:, :GK])], dim=2)
    vv = torch.cat([sp(v1), sp(v2[INDEX][:, :GK])], dim=2)
    return F.scaled_dot_product_attention(sp(q), kk, vv).transpose(1, 2).reshape(P, NQ, HEADS * 64)


@DTYPES
@pytest.mark.parametrize("table", ["index", "key_count"])
def test_self_attention_with_the_garment_segment_from_batch_0(table, dtype, monkeypatch):
    """idmvton_attn: B = P query batches and seg_b0 = {0, 0} -- no batch takes the closed form.  With an index table the launch-wide key
    count is 72 in rows of 80; with a key-count table the capacity is 80 and every batch counts 72 (K rows from 72 on NaN)."""
    from idm_vton_amd import ops
    from tests.kernel_checks import TOL as KTOL
    no_tune_table(monkeypatch)
    q, k1, v1, k2, v2, ko = self_attn_operands(P, G, NQ, GROWS, dtype, seed=21)
    q, k1, v1 = q[:P].contiguous(), k1[:P].contiguous(), v1[:P].contiguous()
    k2, v2 = k2.clone(), v2.clone()
    v2[:, GK:] = 0                                        # V^T positions of keys >= nk: finite
    vt1, ld1 = ko(v1, NQ)
    vt2, ld2 = ko(v2, GROWS)
    k2[:, GK:] = float("nan")                             # K rows >= nk: masked, never a finite logit
    Cc = HEADS * 64
    own = dict(k=k1, vt=vt1, nk=NQ, ldk=Cc, ldvt=ld1)
    gseg = dict(k=k2, vt=vt2, ldk=Cc, ldvt=ld2, k_rows=GROWS, b0=0, nb=G, index=int_table(INDEX))
    gseg.update(dict(nk=GK) if table == "index" else dict(nk=GROWS, nk_table=int_table([GK] * P)))
    qq = (q.float() * ops.QSCALE).to(dtype)
    ref = _sdpa_b0(qq.float() / ops.QSCALE, k1, v1, k2.nan_to_num(0.0), v2)
    for pres, qx in ((True, qq), (False, q)):
        out = nan_out(P, NQ, Cc, dtype)
        ops.attention(qx, out, [own, gseg], HEADS, q_prescaled=pres)
        r = ref if pres else _sdpa_b0(q, k1, v1, k2.nan_to_num(0.0), v2)
        err = ((out.float() - r).abs().max() / r.abs().max()).item()
        print(f"attn b0=0 {table} {dtype} prescaled={pres}: against fp32 SDPA {err:.3e} (bar {KTOL[dtype]:.1e})")
        assert torch.isfinite(out).all() and err <= KTOL[dtype], (table, pres, err)


@DTYPES
@pytest.mark.parametrize("table", ["index", "key_count"])
def test_fp8_self_attention_with_the_garment_segment_from_batch_0(table, dtype):
    """idmvton_attn_f8, the same launch forms; held to the bar include/idmvton_hip.h states for this kernel (tests/garment_support.py)."""
    from idm_vton_amd import ops
    q8, (k8a, vt8a), (k8b, vt8b) = f8_operands(P, G, NQ, GROWS, dtype, seed=21)
    Cc, ld = HEADS * 64, vt8b.shape[1]
    q8, k8a, vt8a = q8[:P * NQ].contiguous(), k8a[:P * NQ].contiguous(), vt8a[:P * Cc].contiguous()
    k8b, vt8b = k8b.clone().view(G, GROWS, Cc), vt8b.clone().view(G, Cc, ld)
    pos = torch.arange(ld, device=DEV)
    key = (pos & ~63) | (((pos >> 4) & 1) << 5) | (((pos >> 2) & 3) << 3) | (((pos >> 5) & 1) << 2) | (pos & 3)      # the key a V^T position holds
    vt8b[:, :, key >= GK] = 0                             # zero from key nk on
    k8b[:, GK:] = 0x7f                                    # e4m3 NaN: K rows >= nk are masked
    own = dict(k8=k8a, vt8=vt8a, nk=NQ, ldk=Cc, ldvt=vt8a.shape[1])
    gseg = dict(k8=k8b.view(G * GROWS, Cc), vt8=vt8b.view(G * Cc, ld), ldk=Cc, ldvt=ld, k_rows=GROWS, b0=0, nb=G, index=int_table(INDEX))
    gseg.update(dict(nk=GK) if table == "index" else dict(nk=GROWS, nk_table=int_table([GK] * P)))
    out = nan_out(P, NQ, Cc, dtype)
    ops.attention_f8(q8, out, [own, gseg], HEADS, qk_scale_exp=-4, v_scale_exp=-2, B=P, Nq=NQ, ldq=Cc, ldo=Cc)
    q, k1, v1, k2, v2, _ = self_attn_operands(P, G, NQ, GROWS, dtype, seed=21)
    ref = _sdpa_b0(q[:P], k1[:P], v1[:P], k2, v2)
    err = ((out.float() - ref).abs().max() / ref.abs().max()).item()
    print(f"attn_f8 b0=0 {table} {dtype}: against fp32 SDPA {err:.3e} (fp8 bar {F8_SDPA_BAR:.1e})")
    assert torch.isfinite(out).all() and err <= F8_SDPA_BAR, (table, err)


# ------------------------------------------------------------------------------------------------------------------ the engine
def _kw(inp, **over):
    return {**dict(num_inference_steps=STEPS, guidance_scale=list(G3), guidance_rescale=list(PHI3), scheduler="ddpm", **inp), **over}


def _denoise(eng, kw, form, trace=None):
    st = eng.prepare(**kw)
    return st, eng.denoise(st, trace=trace, **FORMS[form]).clone()


@DTYPES
def test_a_mixed_batch_is_bit_identical_in_every_execution_form(dtype):
    """guidance_scale = [7.5, 2, 1], guidance_rescale = [0, 0.7, 1]: the guided state (a coef row of 3 + 2B, a work buffer, a graph state of
    its own), the four execution forms and on_step."""
    eng, inp, _ = engine_inputs(dtype, B, STEPS)
    st, ref = _denoise(eng, _kw(inp), "serial_eager")
    assert st["guided"] and st["branches"] == 2 and tuple(st["coef"].shape) == (STEPS, 3 + 2 * B) and st["x_in"].shape[0] == 2 * B
    assert st["coef"][0, 3:].tolist() == [7.5, 2.0, 1.0, 0.0, torch.tensor(0.7).item(), 0.0]      # g <= 1: guidance 1, no rescale
    assert st["work"].numel() == 8 * B and torch.isfinite(ref).all()
    for form in FORMS:
        assert torch.equal(_denoise(eng, _kw(inp), form)[1], ref), form
    assert torch.equal(_denoise(eng, _kw(inp), "graph_overlap")[1], ref)                          # a second call through the captured state
    assert [k for k in eng._graphs if ("guided", 2) in k] == list(eng._graphs) and len(eng._graphs) == 1
    _, plain = _denoise(eng, _kw(inp, guidance_scale=2.0, guidance_rescale=0.0), "graph_overlap")
    assert len(eng._graphs) == 2 and not torch.equal(plain, ref)                                  # the plain state is another one


@DTYPES
def test_every_step_of_a_mixed_batch_is_the_formula(dtype):
    """Step i's traced latents against the fp64 formula on step i - 1's: pack_input + unet.forward replayed as the loop launches them (on a
    device-resident cache, whose views both read), under the kernel's bar -- MARGIN x the float32 evaluation's own error."""
    eng, inp, _ = engine_inputs(dtype, B, STEPS)
    cache = eng.encode_garment(num_inference_steps=STEPS, **garment_kw(inp))
    st = eng.prepare(**{**base_call(inp, STEPS), "cloth": cache, "guidance_scale": list(G3), "guidance_rescale": list(PHI3)})
    start, trace = st["latents"].clone(), {}
    eng.denoise(st, trace=trace)
    lats = [start] + trace["step_latents"]
    assert len(lats) == STEPS + 1
    for i in range(STEPS):
        eps = replay_eps(eng, st, i, lats[i])
        e_k, e_32 = errors(lats[i + 1], eps, lats[i], st["steps_noise"][i], st["coef"][i], 2)
        print(f"{dtype} step {i}: engine against the fp64 formula {e_k:.3e}, float32 torch {e_32:.3e}")
        assert e_32 > 0 and e_k <= MARGIN * e_32, (i, e_k, e_32)


@DTYPES
def test_equal_lists_give_the_plain_calls_bits(dtype):
    eng, inp, _ = engine_inputs(dtype, B, STEPS)
    for form in ("serial_eager", "graph_overlap"):
        st_p, plain = _denoise(eng, _kw(inp, guidance_scale=2.0, guidance_rescale=0.0), form)
        st_g, lists = _denoise(eng, _kw(inp, guidance_scale=[2, 2, 2], guidance_rescale=[0, 0, 0]), form)
        assert not st_p["guided"] and st_p["work"] is None and tuple(st_p["coef"].shape) == (STEPS, 4) and st_g["guided"]
        assert torch.isfinite(plain).all() and torch.equal(lists, plain), form
    assert sorted(len(k) for k in eng._graphs) == [7, 8]                                          # the plain state's key is what it was


def _skip(inp, **over):
    return _kw(inp, guidance_scale=1.0, guidance_rescale=0.0, uncond="skip", **over)


@DTYPES
def test_skip_runs_b_rows_and_every_form_gives_the_replays_bits(dtype):
    """uncond="skip" at g = 1: B TryonNet rows in every per-call tensor; the four forms and on_step bit-identical, live and on a cache; and
    every step bit-equal to the replay -- pack_input_cond + unet.forward at B rows, e = t -- with the step's arithmetic emulated in fp32."""
    eng, inp, _ = engine_inputs(dtype, B, STEPS)
    only_cond = dict(negative_prompt_embeds=None, negative_pooled_prompt_embeds=None, ip_hidden_states=inp["ip_hidden_states"][B:])
    st, ref = _denoise(eng, _skip(inp), "serial_eager")
    assert st["x_in"].shape[0] == B and st["cond"].shape[0] == B and st["temb_t"].shape[1] == B and st["ctx_t"]["B"] == B
    assert st["branches"] == 1 and st["guided"] and st["work"] is None and tuple(st["coef"].shape) == (STEPS, 3 + 2 * B)
    assert torch.isfinite(ref).all()
    for form in FORMS:
        assert torch.equal(_denoise(eng, _skip(inp), form)[1], ref), form
    assert torch.equal(_denoise(eng, _skip({**inp, **only_cond}), "graph_overlap")[1], ref)       # B rows of image states, no negative_*
    assert all(("guided", 1) in k for k in eng._graphs) and len(eng._graphs) == 1
    cache = eng.encode_garment(num_inference_steps=STEPS, **garment_kw(inp))
    st = eng.prepare(**{**base_call(inp, STEPS), "cloth": cache, "guidance_scale": 1.0, "uncond": "skip"})
    st_u = eng.prepare(**_skip(inp))                                                              # (pair's reason: the VAE encodes' batch size)
    st["latents"].copy_(st_u["latents"])
    st["cond"].copy_(st_u["cond"])
    start, trace = st["latents"].clone(), {}
    assert torch.equal(eng.denoise(st, trace=trace), ref)                                         # cached = uncached
    lats = [start] + trace["step_latents"]
    for i in range(STEPS):
        eps = replay_eps(eng, st, i, lats[i])
        assert eps.shape[0] == B
        assert torch.equal(lats[i + 1].cpu(), emulate_cond_step(eps, lats[i], st["steps_noise"][i], st["coef"][i])), i


@DTYPES
def test_skip_against_the_oracle_and_the_batched_call(dtype):
    from oracle import pipeline as opipe
    from oracle.scheduler import Scheduler
    from tests import parity_utils as pu
    from tests.parity_checks import TOL
    eng, inp, m = engine_inputs(dtype, B, STEPS)
    _, skip = _denoise(eng, _skip(inp), "serial_eager")
    _, run = _denoise(eng, _kw(inp, guidance_scale=1.0, guidance_rescale=0.0), "serial_eager")
    tr = {}
    with torch.no_grad():                                 # the oracle runs the conditional branch alone at guidance_scale <= 1
        opipe.run(*m["oracle"], Scheduler("ddpm"), num_inference_steps=STEPS, guidance_scale=1.0, trace=tr,
                  **{**inp, "ip_hidden_states": inp["ip_hidden_states"][B:]})
    e_o, e_r = pu.relerr(skip, tr["step_latents"][-1]), pu.relerr(skip, run)
    print(f"{dtype} skip: against the oracle {e_o:.3e}, against the batched g = 1 call {e_r:.3e} (bar {TOL[dtype]['latents']:.1e})")
    assert e_o <= TOL[dtype]["latents"] and e_r <= TOL[dtype]["latents"], (e_o, e_r)


CACHE_FORMS = ("serial_eager", "graph_overlap")


def _on(eng, base, cache, form, index=None, transport="kernel"):
    st = eng.prepare(**{**base, "cloth": cache, "garment_index": index})
    assert st["x_in"].shape[0] == st["B"] and (st["gnk"] is None or st["gnk"].shape[1] == st["B"])
    return eng.denoise(st, host_transport=transport, **FORMS[form]).clone()


@pytest.mark.parametrize("form", CACHE_FORMS)
def test_skip_on_same_size_cache_forms(form):
    """plain i % G (cached = uncached), garment_index (= the call on the selected garments), slotted at equal sizes, packed (= unpacked),
    features, host-resident on both transports: each bit for bit."""
    dtype = torch.float16
    eng, inp, _ = engine_inputs(dtype, B, STEPS)
    base = {**base_call(inp, STEPS), "guidance_scale": 1.0, "uncond": "skip"}
    plain = eng.encode_garment(num_inference_steps=STEPS, **garment_kw(inp))
    feats = eng.encode_garment(num_inference_steps=STEPS, storage="features", **garment_kw(inp))
    packed = plain.pack()
    pool = slotted_pool(eng, [plain.select([g]) for g in range(B)])
    host, host_packed, host_feats = to_host(plain), to_host(packed), to_host(feats, features=True)
    st_u, st_c = eng.prepare(**_skip(inp)), eng.prepare(**{**base, "cloth": plain})
    st_c["latents"].copy_(st_u["latents"])
    st_c["cond"].copy_(st_u["cond"])
    lat_u, lat_c = eng.denoise(st_u, **FORMS[form]).clone(), eng.denoise(st_c, **FORMS[form]).clone()
    assert torch.isfinite(lat_u).all() and torch.equal(lat_c, lat_u), "plain"
    ref = _on(eng, base, plain, form)
    assert torch.equal(_on(eng, base, feats, form), ref), "features"
    ref_packed = _on(eng, base, packed, form)
    assert torch.equal(ref_packed, _on(eng, base, packed.unpack(), form)) and not torch.equal(ref_packed, ref), "packed"
    for t in TRANSPORTS:
        assert torch.equal(_on(eng, base, host, form, transport=t), ref), ("host", t)
        assert torch.equal(_on(eng, base, host_feats, form, transport=t), ref), ("host features", t)
        assert torch.equal(_on(eng, base, host_packed, form, transport=t), ref_packed), ("host packed", t)
    idx = _on(eng, base, plain, form, WEARS)
    assert torch.equal(idx, _on(eng, base, plain.select(WEARS), form)) and not torch.equal(idx, ref), "indexed"
    assert torch.equal(_on(eng, base, pool, form, WEARS), idx), "slotted"


@pytest.mark.parametrize("storage", ["native", "e4m3", "features"])
def test_skip_on_mixed_size_cache_forms(storage):
    """Garments of three sizes: the slotted pool (a key-count table of [features][B]) in both forms, and the shelf -- K / V^T, packed or
    feature parts, on both transports -- against the slotted device cache of the same garments."""
    dtype = torch.float16
    eng = engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    base = {**base_call(inp, STEPS), "guidance_scale": 1.0, "uncond": "skip"}
    ones = encode_three(eng, garments)
    keys = [KEYS[j] for j in WEARS]
    shelved, index = gpu_shelf(eng, ones, "e4m3" if storage == "e4m3" else "native").get(keys)
    device = shelved.slotted(DEV)                        # (of a packed shelf: the widened values)
    if storage == "features":
        shelved, index = gpu_shelf(eng, encode_three(eng, garments, storage="features"), "features").get(keys)
    ref = _on(eng, base, device, "serial_eager", index)
    assert torch.isfinite(ref).all() and not torch.equal(_on(eng, base, device, "serial_eager", [0, 0, 1]), ref)      # the assignment is read
    if storage == "native":                              # the pool in the garments' own order and the persons' assignment: the same bits
        assert torch.equal(_on(eng, base, slotted_pool(eng, ones), "graph_overlap", WEARS), ref)
    for form in CACHE_FORMS:
        assert torch.equal(_on(eng, base, device, form, index), ref), form
        for t in TRANSPORTS:
            assert torch.equal(_on(eng, base, shelved, form, index, t), ref), (form, t)


def test_skip_on_the_fp8_attention_engine():
    """idmvton_attn_f8 with the garment segment from batch 0 on: the forms agree, and the result is the batched g = 1 call's within the fp8
    variant's stated tolerance (8e-2, tests/test_garment_ragged_gpu.py)."""
    from tests import parity_utils as pu
    dtype = torch.float16
    eng, inp, _ = engine_inputs(dtype, B, STEPS, fp8=True)
    st, skip = _denoise(eng, _skip(inp), "serial_eager")
    assert st["x_in"].shape[0] == B and torch.isfinite(skip).all()
    assert torch.equal(_denoise(eng, _skip(inp), "graph_overlap")[1], skip)
    cache = eng.encode_garment(num_inference_steps=STEPS, **garment_kw(inp))
    assert torch.equal(_on(eng, {**base_call(inp, STEPS), "guidance_scale": 1.0, "uncond": "skip"}, cache, "graph_overlap", WEARS),
                       _on(eng, {**base_call(inp, STEPS), "guidance_scale": 1.0, "uncond": "skip"}, cache.select(WEARS), "serial_eager"))
    _, run = _denoise(eng, _kw(inp, guidance_scale=1.0, guidance_rescale=0.0), "serial_eager")
    err = pu.relerr(skip, run)
    print(f"fp8 attention, skip against the batched g = 1 call: {err:.3e} (bar 8.0e-02)")
    assert err <= 8e-2


# ------------------------------------------------------------------------------------------------------------------ the call surface
def test_boundary_pipeline_takes_lists_rescale_and_skip_uncond():
    DT = torch.float16
    pipe, enc, kw = boundary_pipeline(DT)
    inp, clip_pix, call = boundary_inputs(kw, B, H, W, STEPS, DT)
    cache = pipe.encode_garment(inp["cloth"], inp["text_embeds_cloth"], STEPS, H, W, generator=torch.Generator(DEV).manual_seed(11))
    eng = pipe.hip_engine()
    _, noise = reference_draws(7, 123, B, H, W, STEPS, DT)
    neg, pos = ip_states(enc, clip_pix)
    seen = []
    prepare = eng.prepare
    eng.prepare = lambda **k: (lambda st: (seen.append((st["x_in"].shape[0], st["guided"], st["branches"])), st)[1])(prepare(**k))

    def piped(**over):
        gen = torch.Generator(DEV).manual_seed(7)
        torch.manual_seed(123)                            # the pose posterior uses the GLOBAL generator
        return pipe(generator=gen, cloth=cache, text_embeds_cloth=None, **{**call, **over})[0]

    def direct(ip, **over):
        return eng(image=inp["image"], mask_image=inp["mask_image"], pose_img=inp["pose_img"], prompt_embeds=inp["prompt_embeds"],
                   pooled_prompt_embeds=inp["pooled_prompt_embeds"], text_embeds_cloth=None, noise={**noise, "cloth": None}, num_inference_steps=STEPS,
                   ip_hidden_states=ip, scheduler="ddpm", cloth=cache, **over)

    negs = dict(negative_prompt_embeds=inp["negative_prompt_embeds"], negative_pooled_prompt_embeds=inp["negative_pooled_prompt_embeds"])
    img = piped(guidance_scale=list(G3), guidance_rescale=0.7)
    assert pipe.guidance_scale == list(G3) and pipe.guidance_rescale == 0.7 and pipe.do_classifier_free_guidance and seen[-1] == (2 * B, True, 2)
    assert torch.isfinite(img).all() and torch.equal(img, direct(torch.cat([neg, pos]), guidance_scale=list(G3), guidance_rescale=0.7, **negs))
    assert not torch.equal(img, piped(guidance_scale=list(G3)))                                   # the rescale is applied
    img = piped(guidance_scale=list(G3), guidance_rescale=list(PHI3))
    assert torch.equal(img, direct(torch.cat([neg, pos]), guidance_scale=list(G3), guidance_rescale=list(PHI3), **negs))
    assert pipe.skip_uncond is False
    batched = piped(guidance_scale=[1.0, 0.5, 1.0])                                               # no person above 1: guidance 1, both branches
    assert not pipe.do_classifier_free_guidance and seen[-1] == (2 * B, True, 2)
    pipe.skip_uncond = True
    skipped = piped(guidance_scale=[1.0, 0.5, 1.0])
    assert seen[-1] == (B, True, 1)
    assert torch.equal(skipped, direct(pos, guidance_scale=1.0, uncond="skip", negative_prompt_embeds=None, negative_pooled_prompt_embeds=None))
    assert torch.isfinite(skipped).all() and (skipped - batched).abs().max() < 2e-2               # one fp32 rounding of eps apart, in [0, 1] pixels
    piped(guidance_scale=list(G3))                                                                # a person above 1: skip_uncond does not apply
    assert seen[-1] == (2 * B, True, 2)
