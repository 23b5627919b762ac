"""-m gpu: the row plan.  Kernel level: idmvton_pack_rows against a torch gather and idmvton_pack_input's rows; idmvton_row_step against
idmvton_person_step on the [uncond B | cond B] tensor its rows stand for and against idmvton_guided_step(branches = 1), bit for bit, a
dormant person skipped with NaN and Inf in every row nobody owns, a person's bits under two row counts and two positions.  The attention
kernels at B != 2P: 2 unconditional + 3 conditional query batches.  Engine level, on the issue's worked example (B = 3, 4 steps, strengths
[1.0, 0.5, 0.75], guidance [2, 1, 2]: 16 row-steps instead of 24): the row state and its counters, every execution form, the fp32 oracle
per person, the rows="all" call, every kind of cache, the refusals, the calls with nothing to skip, and the boundary pipeline."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.engine_support import (DEV, H, W, WEARS, base_call, boundary_inputs, boundary_pipeline, engine_inputs, garment_kw, int_table, nan_out,
                                  no_tune_table, run_on, self_attn_operands, to_host)
from tests.frames import Framed, Tight, ints
from tests.garment_support import DTYPES, FORMS, HEADS, TRANSPORTS
from tests.guidance_support import HWS, operands
from tests.rows_support import B, GUIDANCE, N_ACTIVE, SHAPES, STEP2, STEPS, STRENGTHS, TOTAL, call_kw, coef_row, plan_eps, table, with_image_noise

pytestmark = pytest.mark.gpu
LDC = 64
HW_CASES = pytest.mark.parametrize("hw", HWS)
G3 = (7.5, 2.0, 1.5)                                     # everyone with guidance: who gets e = t is the table's business


# ------------------------------------------------------------------------------------------------------------------ pack_rows
@DTYPES
@HW_CASES
def test_pack_rows_is_a_gather_of_pack_input_rows(hw, dtype):
    from idm_vton_amd import ops
    g = torch.Generator().manual_seed(hw)
    lat, cond = torch.randn(B, 4, hw, generator=g).to(DEV), torch.randn(B, hw, 9, generator=g).to(dtype).to(DEV)
    full = ops.pack_input(lat, torch.cat([cond, cond]).contiguous(), torch.empty(2 * B, hw, 16, dtype=dtype, device=DEV))
    for persons in ([1], [0, 2, 0, 2], STEP2["row_person"], [-3, 7, 1, 2 ** 31 - 1, -2 ** 31]):       # the last: entries outside [0, B) are clamped
        al = Framed()
        out = al.out("out", (len(persons), hw, 16), dtype, DEV, contig=True)
        ops.pack_rows(al.inp("latents", lat, contig=True), al.inp("cond", cond, contig=True), out, int_table(persons))
        al.verify()                                       # all written, guard bands intact, the inputs untouched
        want = [min(max(p, 0), B - 1) for p in persons]
        gather = torch.cat([lat[want].permute(0, 2, 1).to(dtype), cond[want], torch.zeros(len(want), hw, 3, dtype=dtype, device=DEV)], dim=-1)
        assert torch.equal(ints(out.contiguous()), ints(gather.contiguous())), persons
        assert torch.equal(ints(out.contiguous()), ints(full[want].contiguous())), persons           # pack_input's casts: that person's row there


# ------------------------------------------------------------------------------------------------------------------ row_step
def _launch(step, eps, lat, noise, coef, extra, al=None):
    """One person_step / guided_step / row_step on device copies of the CPU operands (through the allocation policy `al`) -> the latents."""
    from idm_vton_amd import ops
    al = al or Tight()
    e = al.inp("eps", eps.to(DEV), contig=True)
    x = al.inout("latents", lat.to(DEV).clone(), contig=True)
    nz = al.inp("noise", noise.to(DEV), contig=True) if noise is not None else None
    c = al.inp("coef", coef.to(DEV), contig=True)
    work = None
    if step == "row_step" or extra == 2:
        work = al.out("work", (ops.guided_step_work_floats(lat.shape[0], lat.shape[-1]),), torch.float32, DEV, contig=True, scratch=True)
    getattr(ops, step)(e, x, nz, c, work, extra.to(DEV) if step == "row_step" else extra)
    return x


def _person(eps, lat, noise, g, phi, active=(1, 1, 1)):
    row = torch.cat([coef_row(g, phi), torch.tensor([float(a) for a in active])])
    return _launch("person_step", eps, lat, noise, row, 2)


@DTYPES
@HW_CASES
@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "null_noise"])
@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_both_rows_are_the_person_step(phi, with_noise, hw, dtype):
    """Every person with both rows, scattered over R = 8: the bits of idmvton_person_step on the [uncond B | cond B] tensor those rows
    stand for -- with and without noise, without a rescale and with one (a statistics reduction per person)."""
    full, lat, noise = operands(B, hw, LDC, dtype)
    noise = noise if with_noise else None
    urow, crow = [6, 1, 3], [0, 7, 4]                     # neither [uncond | cond] nor ascending: rows 2 and 5 belong to nobody
    framed = Framed()
    got = _launch("row_step", plan_eps(full, urow, crow, R=8), lat, noise, coef_row(G3, [phi] * B), table(urow, crow), framed)
    framed.verify()
    assert torch.isfinite(got).all() and torch.equal(got, _person(full, lat, noise, G3, [phi] * B))
    assert not torch.equal(got.cpu(), lat)


@DTYPES
@HW_CASES
def test_without_an_unconditional_row_it_is_the_conditional_step(hw, dtype):
    """urow < 0 <= crow for person 1 (whose coef row asks for a rescale, which e = t does not take): the bits of
    idmvton_guided_step(branches = 1) on that row; persons 0 and 2 keep the person step's bits."""
    full, lat, noise = operands(B, hw, LDC, dtype)
    phi = [0.0, 0.7, 0.7]
    urow, crow = [0, -1, 1], [2, 3, 4]
    got = _launch("row_step", plan_eps(full, urow, crow), lat, noise, coef_row(G3, phi), table(urow, crow), Framed())
    cond_only = _launch("guided_step", full[B:], lat, noise, coef_row(G3, phi), 1)
    both = _person(full, lat, noise, G3, phi)
    assert torch.equal(got[1], cond_only[1]) and not torch.equal(got[1], both[1])
    assert torch.equal(got[0], both[0]) and torch.equal(got[2], both[2]) and torch.isfinite(got).all()
    none = table([-1] * B, [0, 1, 2])                     # nobody with an unconditional row: the whole conditional step
    assert torch.equal(_launch("row_step", full[B:].contiguous(), lat, noise, coef_row(G3, phi), none), cond_only)


@DTYPES
@HW_CASES
@pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "null_noise"])
def test_a_dormant_person_is_skipped(with_noise, hw, dtype):
    """crow < 0 for person 1, whose unconditional row is named all the same (it is not read): its latents and its part of `work` keep
    their bits, every row nobody owns holds NaN and Inf, its noise rows NaN; persons 0 and 2 (rescaled) the person step's bits."""
    full, lat, noise = operands(B, hw, LDC, dtype)
    phi = [0.7, 0.7, 0.7]
    ref = _person(full, lat, noise if with_noise else None, G3, phi)
    if with_noise:
        noise[1] = float("nan")
    else:
        noise = None
    urow, crow = [0, 5, 1], [2, -1, 3]                    # person 1's urow names a row nobody owns (NaN / Inf), and so are rows 4 and 6
    eps = plan_eps(full, [0, -1, 1], crow, R=7)
    framed = Framed()
    got = _launch("row_step", eps, lat, noise, coef_row(G3, phi), table(urow, crow), framed)
    framed.verify()                                       # guard bands of latents and work intact, eps / noise / coef untouched
    assert torch.equal(ints(got[1].cpu().contiguous()), ints(lat[1].contiguous()))
    assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2]) and torch.isfinite(got).all()
    work = framed.outs["work"]
    written = ints(work) != work._frame.interior_bits
    per = work.numel() // B                               # persons 0 and 2 have a rescale: their parts are written, the dormant person's is not
    assert written[:per].all() and not written[per:2 * per].any() and written[2 * per:].all()
    nobody = _launch("row_step", eps, lat, noise, coef_row(G3, phi), table([0, 1, 2], [-1, -5, -2 ** 31]))
    assert torch.equal(ints(nobody.cpu()), ints(lat))


@DTYPES
def test_row_indices_are_clamped(dtype):
    """A row index beyond R - 1 reads row R - 1 (a guard: no plan names one)."""
    full, lat, noise = operands(B, HWS[0], LDC, dtype)
    urow, crow = [0, 1, 2], [3, 4, 5]
    framed = Framed()
    got = _launch("row_step", full, lat, noise, coef_row(G3, [0.0] * B), table(urow, [3, 4, 2 ** 31 - 1]), framed)
    framed.verify()
    assert torch.equal(got, _person(full, lat, noise, G3, [0.0] * B))


@DTYPES
def test_a_persons_bits_depend_neither_on_the_rows_nor_on_its_position(dtype):
    """Person 1 alone (B = 1, R = 2), and in a batch of 3 at two positions under R = 5 and R = 9, its neighbours dormant or active."""
    hw = HWS[1]
    full, lat, noise = operands(B, hw, LDC, dtype)
    g, phi = (2.0,), (0.7,)
    alone = _launch("row_step", torch.stack([full[1], full[B + 1]]), lat[1:2], noise[1:2], coef_row(g, phi), table([0], [1]))
    assert torch.equal(alone, _person(full, lat, noise, (7.5, 2.0, 1.5), (0.0, 0.7, 0.0))[1:2])
    for pos, order, R, urow, crow in ((0, [1, 0, 2], 5, [3, -1, 0], [1, -1, 4]), (2, [0, 2, 1], 9, [0, 1, 8], [2, 6, 5])):
        pick = lambda v: [v[i] for i in order]
        sub = torch.cat([full[order], full[[B + i for i in order]]])
        got = _launch("row_step", plan_eps(sub, urow, crow, R=R), lat[order], noise[order], coef_row(pick((7.5, 2.0, 1.5)), pick((0.0, 0.7, 0.0))),
                      table(urow, crow), Framed())
        assert torch.equal(got[pos:pos + 1], alone), pos


# ------------------------------------------------------------------------------------------------------------------ attention at B != 2P
def _sp(t):
    return t.float().view(t.shape[0], t.shape[1], HEADS, 64).transpose(1, 2)


@DTYPES
def test_self_attention_with_two_unconditional_and_three_conditional_batches(dtype, monkeypatch):
    """What a plan of shape (R, a) = (5, 3) launches: 5 query batches of 80 rows, the garment segment from batch b0 = 2 on, read through
    the slot table [2, 0, 1] and a key-count table -- 96 keys in slots of 128 --, against fp32 SDPA on materialised keys (an unconditional
    batch sees that many zero keys).  K rows and V^T columns past a slot's keys hold NaN."""
    no_tune_table(monkeypatch)
    from idm_vton_amd import ops
    from tests.kernel_checks import TOL as KTOL
    P, R, b0, Nq, CAP, NK, slots = 3, 5, 2, 80, 128, 96, [2, 0, 1]
    q, k1, v1, k2, v2, ko = self_attn_operands(P, P, Nq, CAP, dtype, seed=31)
    q, k1, v1 = q[:R].contiguous(), k1[:R].contiguous(), v1[:R].contiguous()
    k2, v2 = k2.clone(), v2.clone()
    v2[:, NK:] = 0
    vt1, ld1 = ko(v1, Nq)
    vt2, ld2 = ko(v2, CAP)
    k2[:, NK:] = float("nan")
    vt2[:, :, ops.round16(NK):] = float("nan")
    Cc = HEADS * 64
    out = nan_out(R, Nq, Cc, dtype)
    ops.attention(q, out, [dict(k=k1, vt=vt1, nk=Nq, ldk=Cc, ldvt=ld1),
                           dict(k=k2, vt=vt2, nk=CAP, ldk=Cc, ldvt=ld2, k_rows=CAP, b0=b0, nb=P, index=int_table(slots), nk_table=int_table([NK] * R))], HEADS)
    assert torch.isfinite(out).all()
    ref = []
    for b in range(R):
        s = slots[max(b - b0, 0)]
        kg, vg = _sp(k2[s:s + 1, :NK]), _sp(v2[s:s + 1, :NK])
        if b < b0:
            kg, vg = torch.zeros_like(kg), torch.zeros_like(vg)
        kk, vv = torch.cat([_sp(k1[b:b + 1]), kg], dim=2), torch.cat([_sp(v1[b:b + 1]), vg], dim=2)
        ref.append(F.scaled_dot_product_attention(_sp(q[b:b + 1]), kk, vv).transpose(1, 2).reshape(1, Nq, Cc))
    ref = torch.cat(ref)
    err = ((out.float() - ref).abs().max() / ref.abs().max()).item()
    print(f"{dtype} 2 + 3 batches: against fp32 SDPA {err:.3e} (bar {KTOL[dtype]:.1e})")
    assert err <= KTOL[dtype], err                        # the bar tests/kernel_checks.py holds check_attn_self to (imported)


# ------------------------------------------------------------------------------------------------------------------ the engine
def _world(dtype):
    """-> (a new engine, the call's keywords without its cache, the cache of the B garments, the model)."""
    eng, inp, m = engine_inputs(dtype, B, STEPS)
    inp = with_image_noise(inp)
    cache = eng.encode_garment(num_inference_steps=STEPS, **garment_kw(inp))
    return eng, base_call(inp, STEPS), cache, inp, m


def _denoise(eng, kw, form="serial_eager", transport="kernel"):
    st = eng.prepare(**kw)
    return st, eng.denoise(st, host_transport=transport, **FORMS[form]).clone()


@functools.lru_cache(maxsize=None)
def _shared(dtype):
    """Computed once per dtype and left unchanged: the worked example under rows="needed" and under rows="all", the batch without
    guidance under uncond="skip" at the same strengths (serial eager, device-resident cache, garment_index = WEARS), and the fp32 oracle of
    each person alone at its own strength and guidance."""
    from oracle import pipeline as opipe
    from oracle.scheduler import Scheduler
    eng, base, cache, inp, m = _world(dtype)
    needed = _denoise(eng, call_kw(base, cache, WEARS, rows="needed"))[1]
    every = _denoise(eng, call_kw(base, cache, WEARS))[1]
    skip = _denoise(eng, call_kw(base, cache, WEARS, guidance_scale=[1.0] * B, uncond="skip"))[1]
    oracle = []
    for i, (s, n_i, g, j) in enumerate(zip(STRENGTHS, N_ACTIVE, GUIDANCE, WEARS)):
        one = {k: v[i:i + 1] for k, v in inp.items() if k not in ("noise", "ip_hidden_states", "cloth", "text_embeds_cloth")}
        ip = inp["ip_hidden_states"]
        one["ip_hidden_states"] = torch.cat([ip[i:i + 1], ip[B + i:B + i + 1]]) if g > 1 else ip[B + i:B + i + 1]
        one["noise"] = {k: (v[STEPS - n_i:, i:i + 1] if k == "steps" else v[i:i + 1]) for k, v in inp["noise"].items() if k != "cloth"}
        one["noise"]["cloth"] = inp["noise"]["cloth"][j:j + 1]
        one.update(cloth=inp["cloth"][j:j + 1], text_embeds_cloth=inp["text_embeds_cloth"][j:j + 1])
        with torch.no_grad():
            oracle.append(opipe.run(*m["oracle"], Scheduler("ddpm"), num_inference_steps=STEPS, guidance_scale=g, strength=s, return_latents=True, **one))
    return dict(needed=needed, every=every, skip=skip, oracle=oracle)


def test_the_worked_example_is_a_row_state():
    """st["rows"], the shapes of what it carries, and the counters: 16 row-steps in 4 steps.  The same call under rows="all" is the person
    state it was, with neither counter."""
    dtype = torch.float16
    eng, base, cache, _, _ = _world(dtype)
    st, got = _denoise(eng, call_kw(base, cache, WEARS, rows="needed"))
    rw = st["rows"]
    assert rw["step"] == [0, 1, 2, 2] and [(p["R"], p["a"]) for p in rw["plans"]] == SHAPES
    assert "person" not in st and st["guided"] and st["branches"] == 2 and st["gindex"] == WEARS
    assert tuple(st["cond"].shape) == (B, 256, 9) and st["x_in"].shape[0] == 5 and tuple(st["coef"].shape) == (STEPS, 3 + 2 * B)
    assert [tuple(t.shape[:1]) for t in rw["temb"]] == [(2,), (4,), (5,), (5,)]
    p = rw["plans"][2]
    assert p["table"].tolist() == STEP2["urow"] + STEP2["crow"] and p["row_person_t"].tolist() == STEP2["row_person"] and p["gix"].tolist() == WEARS
    assert all(t.shape[0] in (5, 5 * p["ctx"]["rt"], 5 * p["ctx"]["ri"]) for ent in p["ctx"]["kv"].values() for t in ent.values())
    full = st["ctx_t"]["kv"]
    for name, ent in p["ctx"]["kv"].items():              # the rows' own context, out of the full layout
        assert torch.equal(ent["vtt"], full[name]["vtt"][STEP2["full_rows"]]) and torch.equal(ent["ki"][-p["ctx"]["ri"]:], full[name]["ki"][-p["ctx"]["ri"]:])
    assert torch.isfinite(got).all()
    assert eng.stats["tryon_rows"] == TOTAL == 16 and eng.stats["row_steps"] == STEPS and eng.stats["person_steps"] == 0
    eng2, base2, cache2, _, _ = _world(dtype)
    st_all, every = _denoise(eng2, call_kw(base2, cache2, WEARS, rows="all"))
    assert "rows" not in st_all and st_all["person"] and "tryon_rows" not in eng2.stats and "row_steps" not in eng2.stats
    assert eng2.stats["person_steps"] == STEPS and torch.equal(every, _shared(dtype)["every"]) and torch.equal(got, _shared(dtype)["needed"])


def test_every_execution_form_gives_the_same_bits():
    dtype = torch.float16
    eng, base, cache, _, _ = _world(dtype)
    kw = call_kw(base, cache, WEARS, rows="needed")
    ref = _shared(dtype)["needed"]
    for form in FORMS:
        assert torch.equal(_denoise(eng, kw, form)[1], ref), form
    assert torch.equal(_denoise(eng, kw, "graph_overlap")[1], ref)                                # a second call through the captured state
    assert len(eng._graphs) == 1 and all(k[-1] == ("rows", 2) and k[-3:-1] == ("cached", "indexed") for k in eng._graphs)
    G = next(iter(eng._graphs.values()))
    assert sorted(G["rows"]) == SHAPES and all(len(gk) == 5 and gk[3:] in SHAPES for gk in G["graphs"])
    assert eng.stats["tryon_rows"] == (len(FORMS) + 1) * TOTAL and eng.stats["row_steps"] == (len(FORMS) + 1) * STEPS
    # another plan through the same state: the persons trade places ((R, a) = (1, 1), (3, 2), (5, 3): two new shapes, one known)
    other = call_kw(base, cache, WEARS, rows="needed", strength=[0.5, 1.0, 0.75], guidance_scale=[2.0, 1.0, 2.0])
    assert torch.equal(_denoise(eng, other, "graph_overlap")[1], _denoise(eng, other)[1])
    assert len(eng._graphs) == 1 and sorted(G["rows"]) == sorted(set(SHAPES) | {(1, 1), (3, 2)})
    assert torch.equal(_denoise(eng, kw, "graph")[1], ref)                                        # and the first plan again, its tables copied back


@DTYPES
def test_each_person_against_the_oracle_at_its_strength_and_guidance(dtype):
    """oracle.pipeline.run on each person alone at its own strength, guidance and garment (fp32, CPU); the bar is the tiny-pipeline
    latents bar of that dtype."""
    from tests import parity_utils as pu
    from tests.parity_checks import TOL
    sh = _shared(dtype)
    for i in range(B):
        err, err_all = pu.relerr(sh["needed"][i:i + 1], sh["oracle"][i]), pu.relerr(sh["every"][i:i + 1], sh["oracle"][i])
        print(f"{dtype} person {i} (strength {STRENGTHS[i]}, g {GUIDANCE[i]}): needed against the oracle {err:.3e}, all against the oracle {err_all:.3e} "
              f"(bar {TOL[dtype]['latents']:.1e})")
        assert err <= TOL[dtype]["latents"], (i, err)


@DTYPES
def test_against_the_call_that_runs_every_row(dtype):
    """Does a TryonNet row depend on the launch's row count?  Persons 0 and 2 (g > 1) against the rows="all" call, person 1 (g <= 1, e = t)
    against the batch without guidance under uncond="skip" at the same strengths."""
    from tests import parity_utils as pu
    sh = _shared(dtype)
    for i, other in ((0, "every"), (2, "every"), (1, "skip")):
        same = torch.equal(sh["needed"][i], sh[other][i])
        e_new, e_old = pu.relerr(sh["needed"][i:i + 1], sh[other][i:i + 1]), pu.relerr(sh[other][i:i + 1], sh["oracle"][i])
        print(f"{dtype} person {i}: needed against {other}: equal {same}, relerr {e_new:.3e}; {other} against the oracle {e_old:.3e}")
        assert same, (i, other, e_new, e_old)


@pytest.mark.parametrize("form", ["serial_eager", "graph_overlap"])
def test_on_every_kind_of_cache(form):
    """The row state on what `prepare` accepts as a cache -- features, packed (= its unpacked values), host-resident on both transports,
    garment_index on a plain and on a slotted pool, shelved --: each bit for bit what the device-resident 16-bit cache gives."""
    dtype = torch.float16
    eng, base, plain, inp, _ = _world(dtype)
    base = call_kw(base, None, None, rows="needed")
    feats = eng.encode_garment(num_inference_steps=STEPS, storage="features", **garment_kw(inp))
    packed = plain.pack()
    ref = run_on(eng, base, plain, form)                  # no garment_index: the index i % G, through the indexed sets
    assert torch.isfinite(ref).all() and torch.equal(ref, run_on(eng, base, plain, form, [0, 1, 2]))
    assert torch.equal(run_on(eng, base, feats, form), ref), "features"
    ref_packed = run_on(eng, base, packed, form)
    assert torch.equal(ref_packed, run_on(eng, base, packed.unpack(), form)) and not torch.equal(ref_packed, ref), "packed"
    for t in TRANSPORTS:
        assert torch.equal(run_on(eng, base, to_host(plain), form, transport=t), ref), ("host", t)
        assert torch.equal(run_on(eng, base, to_host(feats, features=True), form, transport=t), ref), ("host features", t)
        assert torch.equal(run_on(eng, base, to_host(packed), form, transport=t), ref_packed), ("host packed", t)
    idx = run_on(eng, base, plain, form, WEARS)
    assert torch.equal(idx, _shared(dtype)["needed"]) and torch.equal(idx, run_on(eng, base, plain.select(WEARS), form)) and not torch.equal(idx, ref), "indexed"
    pool = eng.empty_garment_cache(B, H, W, STEPS, height=H, width=W)
    for g in range(B):
        pool.put(g, plain.select([g]))
    assert torch.equal(run_on(eng, base, pool, form, WEARS), idx), "slotted"
    from idm_vton_amd.garment_cache import GarmentShelf
    shelf = GarmentShelf(eng.empty_garment_cache(1, H, W, STEPS, height=H, width=W), storage="native")
    for g in range(B):
        shelf.add(f"g{g}", plain.select([g]))
    shelved, index = shelf.get([f"g{j}" for j in WEARS])
    on_device = run_on(eng, base, shelved.slotted(DEV), form, index)
    assert torch.equal(on_device, idx), "shelved, on the device"
    for t in TRANSPORTS:
        assert torch.equal(run_on(eng, base, shelved, form, index, t), on_device), ("shelved", t)
    assert all(k[-1] == ("rows", 2) for k in eng._graphs)


def test_refusals_by_message():
    dtype = torch.float16
    eng, base, cache, inp, _ = _world(dtype)
    live = dict(num_inference_steps=STEPS, guidance_scale=list(GUIDANCE), strength=list(STRENGTHS), **inp)
    with pytest.raises(ValueError, match="rows=\"needed\" reads the garments through an index table, and an index on a live call is still out"):
        eng.prepare(**live, rows="needed")
    with pytest.raises(ValueError, match="rows='most'"):
        eng(**call_kw(base, cache, WEARS, rows="most"))
    eng8, inp8, _ = engine_inputs(dtype, B, STEPS, fp8=True)
    inp8 = with_image_noise(inp8)
    cache8 = eng8.encode_garment(num_inference_steps=STEPS, **garment_kw(inp8))
    with pytest.raises(ValueError, match="rows=\"needed\": attn_fp8 mismatch"):
        eng8.prepare(**call_kw(base_call(inp8, STEPS), cache8, WEARS, rows="needed"))
    with pytest.raises(ValueError, match="uncond=\"skip\" runs the conditional branch alone"):      # uncond="skip" keeps its own condition
        eng.prepare(**call_kw(base, cache, WEARS, rows="needed", uncond="skip"))
    assert not eng._graphs and "tryon_rows" not in eng.stats


def test_skip_and_needed_together():
    """uncond="skip" (nobody with guidance) and rows="needed" with dormant steps: conditional rows alone, 1 + 2 + 3 + 3 of them, each
    person the bits it has under rows="needed" alone."""
    dtype = torch.float16
    eng, base, cache, _, _ = _world(dtype)
    kw = call_kw(base, cache, WEARS, rows="needed", guidance_scale=[1.0, 0.5, 1.0])
    st, got = _denoise(eng, {**kw, "uncond": "skip"})
    assert [(p["R"], p["a"], p["u"]) for p in st["rows"]["plans"]] == [(1, 1, 0), (2, 2, 0), (3, 3, 0)] and eng.stats["tryon_rows"] == 9
    assert torch.isfinite(got).all() and torch.equal(got, _denoise(eng, kw)[1])
    assert torch.equal(got, _denoise(eng, {**kw, "uncond": "skip"}, "graph_overlap")[1])


def test_a_call_with_nothing_to_skip_is_the_state_it_was():
    """Under rows="needed": a scalar strength with guidance for everyone is the plain state, equal strengths the person state, nobody with
    guidance and nobody dormant the branches = 1 state of uncond="skip" -- the graph key, the kernels and the bits of the call under "all"."""
    dtype = torch.float16
    eng, base, cache, _, _ = _world(dtype)
    plain = {**base, "cloth": cache, "garment_index": WEARS, "strength": 1.0, "guidance_scale": 2.0}
    equal = {**plain, "strength": [0.75] * B, "guidance_scale": [2.0, 7.5, 1.5]}
    nobody = {**plain, "guidance_scale": [1.0, 0.5, 1.0]}
    for kw, ref_kw, last in ((plain, plain, "indexed"), (equal, equal, ("person", 2)), (nobody, {**nobody, "uncond": "skip"}, ("guided", 1))):
        before = len(eng._graphs)
        st_all, ref = _denoise(eng, ref_kw, "graph_overlap")
        st, got = _denoise(eng, {**kw, "rows": "needed"}, "graph_overlap")
        assert "rows" not in st and st.keys() == st_all.keys() and st["branches"] == st_all["branches"] and st["coef"].shape == st_all["coef"].shape
        assert len(eng._graphs) == before + 1 and list(eng._graphs)[-1][-1] == last                # one state serves both calls
        assert torch.equal(got, ref)
    assert "tryon_rows" not in eng.stats and "row_steps" not in eng.stats


# ------------------------------------------------------------------------------------------------------------------ the call surface
def test_boundary_pipeline_hands_rows_to_the_engine():
    """pipe.rows = "needed" with a strength and a guidance scale per person and one generator per person: the result of the engine call
    that crossed the boundary (trace_call), which carries rows="needed"; pipe.rows = "all" passes no such keyword."""
    DT = torch.float16
    pipe, enc, kw = boundary_pipeline(DT)
    inp, _, call = boundary_inputs(kw, B, H, W, STEPS, DT)
    cache = pipe.encode_garment(inp["cloth"], inp["text_embeds_cloth"], STEPS, H, W, generator=torch.Generator(DEV).manual_seed(11))
    call.update(cloth=cache, text_embeds_cloth=None, garment_index=WEARS, output_type="latent", strength=list(STRENGTHS), guidance_scale=list(GUIDANCE))
    seen = {}
    pipe.trace_call = seen

    def piped():
        torch.manual_seed(123)                            # the pose posterior uses the GLOBAL generator
        return pipe(generator=[torch.Generator(DEV).manual_seed(40 + i) for i in range(B)], **call)[0]

    every = piped()
    assert "rows" not in seen
    pipe.rows = "needed"
    eng = pipe.hip_engine()
    needed = piped()
    assert seen["rows"] == "needed" and seen["strength"] == STRENGTHS and seen["guidance_scale"] == GUIDANCE
    assert eng.stats["tryon_rows"] == TOTAL and eng.stats["row_steps"] == STEPS
    ref = eng(image_dtype=seen["prompt_embeds"].dtype, return_latents=True, use_graph=pipe.use_graph, overlap=pipe.overlap, **seen).clone()
    assert torch.isfinite(needed).all() and torch.equal(needed, ref) and needed.shape == every.shape
    pipe.rows = "most"
    with pytest.raises(ValueError, match="rows='most'"):
        piped()
