"""-m gpu: strength per person.  idmvton_person_step on operands framed in poisoned memory (tests/frames.py): an active person gets
idmvton_guided_step's bits, a dormant person is skipped -- its eps rows hold NaN and Inf, its latents, its part of `work` and every frame
byte keep their bits --, and a person's bits depend neither on B nor on its position.  The engine: every person of a mixed batch against
the same batch at that person's scalar strength, bit for bit, in every execution form, on a cache with garment_index, with per-person
guidance and with uncond="skip"; the scalar call's key and kernel; one oracle case; and the boundary pipeline with one generator per person.
Tiny engines: latent 16 x 16, 6 steps (blocks of 1, 2, 3 timesteps), B = 3, strengths [1.0, 0.5, 0.7] = 6, 3 and 4 steps."""
import pytest
import torch

from tests.engine_support import DEV, H, W, WEARS, base_call, boundary_inputs, boundary_pipeline, engine_inputs, garment_kw, run_on, to_host
from tests.frames import Framed, Tight, ints
from tests.garment_support import DTYPES, FORMS, TRANSPORTS
from tests.guidance_support import G3, PHI3, coef_row, operands
from tests.strength_support import HW, LDC, N_ACTIVE, STEPS, STRENGTHS, person_row, poison_person, scalar_call, with_image_noise

pytestmark = pytest.mark.gpu
B = 3
BRANCHES = pytest.mark.parametrize("branches", [2, 1], ids=["both", "cond_only"])
NOISE = pytest.mark.parametrize("with_noise", [True, False], ids=["noise", "null_noise"])
SCHEDULERS = pytest.mark.parametrize("scheduler", ["ddpm", "ddim"])


# ------------------------------------------------------------------------------------------------------------------ the kernel
def _launch(step, eps, lat, noise, coef, branches, al=None):
    """One guided_step / person_step on device copies of the CPU operands (through the allocation policy `al`) -> the updated latents."""
    from idm_vton_amd import ops
    al = al or Tight()
    e = al.inp("eps", eps.to(DEV), contig=True)
    x = al.inout("latents", lat.to(DEV).clone(), contig=True)
    nz = al.inp("noise", noise.to(DEV), contig=True) if noise is not None else None
    c = al.inp("coef", coef.to(DEV), contig=True)
    work = al.out("work", (ops.guided_step_work_floats(lat.shape[0], lat.shape[-1]),), torch.float32, DEV, contig=True, scratch=True) if branches == 2 else None
    getattr(ops, step)(e, x, nz, c, work, branches)
    return x


def _guided(eps, lat, noise, branches):
    return _launch("guided_step", eps, lat, noise, coef_row(G3, PHI3), branches)


@DTYPES
@BRANCHES
@NOISE
def test_all_active_is_the_guided_step(with_noise, branches, dtype):
    """g = (7.5, 2, 1), phi = (0, 0.7, 1): a person without rescale, two with; hw = 1100: two statistics chunks, a partial last workgroup."""
    eps, lat, noise = operands(B, HW, LDC, dtype, branches=branches)
    noise = noise if with_noise else None
    framed = Framed()
    got = _launch("person_step", eps, lat, noise, person_row(G3, PHI3, (1, 1, 1)), branches, framed)
    framed.verify()
    assert torch.isfinite(got).all() and torch.equal(got, _guided(eps, lat, noise, branches))
    assert not torch.equal(got.cpu(), lat)


@DTYPES
@BRANCHES
@NOISE
def test_a_dormant_person_is_skipped(with_noise, branches, dtype):
    """Person 1 (g = 2, phi = 0.7: the one whose statistics would be taken) dormant, its eps rows and its noise rows NaN and Inf: its
    latents and its part of `work` bit for bit what they were, every frame byte too; persons 0 and 2 the guided step's bits."""
    eps, lat, noise = operands(B, HW, LDC, dtype, branches=branches)
    ref = _guided(eps, lat, noise if with_noise else None, branches)
    eps = poison_person(eps, 1, B, branches)
    if with_noise:
        noise[1] = float("nan")
    else:
        noise = None
    framed = Framed()
    got = _launch("person_step", eps, lat, noise, person_row(G3, PHI3, (1, 0, 1)), branches, framed)
    framed.verify()                                       # guard bands of latents and work intact, eps / noise / coef untouched
    assert torch.equal(ints(got[1].cpu().contiguous()), ints(lat[1].contiguous()))
    assert torch.equal(got[0], ref[0]) and torch.equal(got[2], ref[2]) and torch.isfinite(got).all()
    if branches == 2:
        work = framed.outs["work"]
        written = ints(work) != work._frame.interior_bits
        per = work.numel() // B                           # person 0 has phi = 0 and person 1 is dormant: only person 2's part is written
        assert not written[:2 * per].any() and written[2 * per:].all()
    # NaN in the `active` column is dormant too, and so is everyone when the column is zero
    none = _launch("person_step", eps, lat, noise, person_row(G3, PHI3, (float("nan"), 0, -1.0)), branches)
    assert torch.equal(ints(none.cpu()), ints(lat))


@DTYPES
@BRANCHES
def test_a_persons_bits_depend_neither_on_b_nor_on_its_position(branches, dtype):
    """Person 1 alone (B = 1) and at each position of a batch of 3, its neighbours active or dormant."""
    eps, lat, noise = operands(B, HW, LDC, dtype, branches=branches)
    rows = lambda order: torch.cat([eps[[r * B + i for i in order]] for r in range(branches)])
    alone = _launch("person_step", rows([1]), lat[1:2], noise[1:2], person_row(G3[1:2], PHI3[1:2], (1,)), branches)
    assert torch.equal(alone, _guided(eps, lat, noise, branches)[1:2])
    for pos, order, active in ((0, [1, 0, 2], (1, 0, 1)), (1, [0, 1, 2], (0, 1, 0)), (2, [2, 0, 1], (1, 1, 1))):
        pick = lambda v: [v[i] for i in order]
        got = _launch("person_step", rows(order), lat[order], noise[order], person_row(pick(G3), pick(PHI3), active), branches, Framed())
        assert torch.equal(got[pos:pos + 1], alone), pos


# ------------------------------------------------------------------------------------------------------------------ the engine
def _kw(inp, scheduler="ddpm", **over):
    return {**dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler=scheduler, strength=list(STRENGTHS), **inp), **over}


def _denoise(eng, kw, form="serial_eager"):
    st = eng.prepare(**kw)
    return st, eng.denoise(st, **FORMS[form]).clone()


def _rows_equal_the_scalar_calls(eng, kw, form="serial_eager", **prep):
    """Row i of the per-person call == row i of the same batch at the scalar strength s_i (step noise sliced to its steps)."""
    st, mixed = _denoise(eng, kw, form)
    assert st["person"] and st["n_active"] == N_ACTIVE and len(st["timesteps"]) == max(N_ACTIVE) and tuple(st["coef"].shape) == (STEPS, 3 + 3 * B)
    assert torch.isfinite(mixed).all()
    outs = []
    for i, s in enumerate(STRENGTHS):
        st_s, one = _denoise(eng, scalar_call(kw, s, STEPS), form)
        assert "person" not in st_s and len(st_s["timesteps"]) == N_ACTIVE[i]
        assert torch.equal(mixed[i], one[i]), (i, s, (mixed[i] - one[i]).abs().max().item())
        outs.append(one)
    assert not torch.equal(mixed[1], outs[0][1]) and not torch.equal(mixed[2], outs[1][2])      # and the strengths do something
    return st, mixed


@DTYPES
@SCHEDULERS
def test_each_person_is_the_scalar_call_at_its_strength(scheduler, dtype):
    eng, inp, _ = engine_inputs(dtype, B, STEPS)
    st, _ = _rows_equal_the_scalar_calls(eng, _kw(with_image_noise(inp), scheduler))
    assert (st["steps_noise"] is not None) == (scheduler == "ddpm")
    assert eng.stats["person_steps"] == STEPS             # the three scalar calls made none


@SCHEDULERS
def test_every_execution_form_gives_the_same_bits(scheduler):
    dtype = torch.float16
    eng, inp, _ = engine_inputs(dtype, B, STEPS)
    kw = _kw(with_image_noise(inp), scheduler)
    _, ref = _denoise(eng, kw)
    assert torch.isfinite(ref).all()
    for form in FORMS:
        assert torch.equal(_denoise(eng, kw, form)[1], ref), form
    assert torch.equal(_denoise(eng, kw, "graph_overlap")[1], ref)                                # a second call through the captured state
    assert len(eng._graphs) == 1 and all(("person", 2) in k for k in eng._graphs)
    assert eng.stats["person_steps"] == (len(FORMS) + 2) * STEPS                                  # launches and replays of calls, no capture


@pytest.mark.parametrize("case", ["garment_index", "guidance_per_person", "skip_uncond"])
def test_on_a_cache_with_per_person_guidance_and_without_uncond(case):
    """A device-resident GarmentCache made at strength 1 serves every person's suffix; with garment_index, with a guidance scale and a
    rescale per person, and with uncond="skip" (B TryonNet rows, branches 1)."""
    dtype = torch.float16
    eng, inp, _ = engine_inputs(dtype, B, STEPS)
    cache = eng.encode_garment(num_inference_steps=STEPS, **garment_kw(inp))
    kw = {**base_call(with_image_noise(inp), STEPS), "cloth": cache, "strength": list(STRENGTHS)}
    if case == "garment_index":
        kw["garment_index"] = WEARS
    elif case == "guidance_per_person":
        kw.update(guidance_scale=list(G3), guidance_rescale=list(PHI3))
    else:
        kw.update(guidance_scale=1.0, uncond="skip")
    st, mixed = _rows_equal_the_scalar_calls(eng, kw)
    assert st["branches"] == (1 if case == "skip_uncond" else 2) and (st["work"] is None) == (case == "skip_uncond")
    if case == "guidance_per_person":
        assert st["coef"][0, 3:].tolist() == [7.5, 2.0, 1.0, 0.0, torch.tensor(0.7).item(), 0.0, 1.0, 0.0, 0.0]
    assert torch.equal(_denoise(eng, kw, "graph_overlap")[1], mixed)
    assert [k[-1] for k in eng._graphs] == [("person", st["branches"])]


@pytest.mark.parametrize("form", ["serial_eager", "graph_overlap"])
def test_on_every_kind_of_cache(form):
    """The person state on what `prepare` accepts as a cache -- features, packed (= its unpacked values), host-resident on both transports,
    garment_index on a plain and on a slotted pool --: each bit for bit what the device-resident 16-bit cache gives; the fills are the
    loop's (the longest timestep list), whoever is dormant."""
    dtype = torch.float16
    eng, inp, _ = engine_inputs(dtype, B, STEPS)
    base = {**base_call(with_image_noise(inp), STEPS), "strength": list(STRENGTHS)}
    plain = eng.encode_garment(num_inference_steps=STEPS, **garment_kw(inp))
    feats = eng.encode_garment(num_inference_steps=STEPS, storage="features", **garment_kw(inp))
    packed = plain.pack()
    ref = run_on(eng, base, plain, form)
    assert torch.isfinite(ref).all() and torch.equal(run_on(eng, base, feats, form), ref), "features"
    ref_packed = run_on(eng, base, packed, form)
    assert torch.equal(ref_packed, run_on(eng, base, packed.unpack(), form)) and not torch.equal(ref_packed, ref), "packed"
    for t in TRANSPORTS:
        assert torch.equal(run_on(eng, base, to_host(plain), form, transport=t), ref), ("host", t)
        assert torch.equal(run_on(eng, base, to_host(feats, features=True), form, transport=t), ref), ("host features", t)
        assert torch.equal(run_on(eng, base, to_host(packed), form, transport=t), ref_packed), ("host packed", t)
    idx = run_on(eng, base, plain, form, WEARS)
    assert torch.equal(idx, run_on(eng, base, plain.select(WEARS), form)) and not torch.equal(idx, ref), "indexed"
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
    for t in TRANSPORTS:
        assert torch.equal(run_on(eng, base, shelved, form, index, t), on_device), ("shelved", t)
    assert all(k[-1] == ("person", 2) for k in eng._graphs)


def test_on_the_fp8_attention_engine():
    """idmvton_guided_step runs behind the fp8 attention kernels as it does behind the 16-bit ones, and so does the person step: live
    and on a cache, each person the scalar call's bits."""
    dtype = torch.float16
    eng, inp, _ = engine_inputs(dtype, B, STEPS, fp8=True)
    inp = with_image_noise(inp)
    _, mixed = _rows_equal_the_scalar_calls(eng, _kw(inp))
    assert torch.equal(_denoise(eng, _kw(inp), "graph_overlap")[1], mixed)
    cache = eng.encode_garment(num_inference_steps=STEPS, **garment_kw(inp))
    _rows_equal_the_scalar_calls(eng, {**base_call(inp, STEPS), "cloth": cache, "strength": list(STRENGTHS), "garment_index": WEARS})


def test_a_scalar_strength_keeps_its_key_and_its_kernel():
    """strength = 0.5 as a float: the plain state -- no `person` entry, a [steps][4] table, the 7-element graph key of a live call with step
    noise -- and no person_step launch; the list [0.5, 0.5, 0.5] is a person state of its own with the same bits."""
    dtype = torch.float16
    eng, inp, _ = engine_inputs(dtype, B, STEPS)
    kw = _kw(with_image_noise(inp))
    st, plain = _denoise(eng, scalar_call(kw, 0.5, STEPS), "graph_overlap")
    assert "person" not in st and not st["guided"] and st["work"] is None and tuple(st["coef"].shape) == (3, 4)
    assert list(eng._graphs) == [(B, 16, 16, 16, 16, st["k"], True)]
    assert eng.stats["person_steps"] == 0 and "person_steps" not in eng.stats
    halves = {**kw, "strength": [0.5] * B, "noise": scalar_call(kw, 0.5, STEPS)["noise"]}        # n_max = 3: the loop's steps are the scalar call's
    st_p, lists = _denoise(eng, halves, "graph_overlap")
    assert st_p["person"] and len(st_p["timesteps"]) == 3 and torch.equal(lists, plain)
    assert list(eng._graphs)[1:] == [(B, 16, 16, 16, 16, st["k"], True, ("person", 2))] and eng.stats["person_steps"] == 3


def test_each_person_against_the_oracle_at_its_strength():
    """oracle.pipeline.run on each person alone at its own strength (fp32, CPU); the bar is the tiny-pipeline latents bar of that dtype."""
    from oracle import pipeline as opipe
    from oracle.scheduler import Scheduler
    from tests import parity_utils as pu
    from tests.parity_checks import TOL
    dtype = torch.float16
    eng, inp, m = engine_inputs(dtype, B, STEPS)
    inp = with_image_noise(inp)
    _, mixed = _denoise(eng, _kw(inp))
    for i, (s, n_i) in enumerate(zip(STRENGTHS, N_ACTIVE)):
        one = {k: v[i:i + 1] for k, v in inp.items() if k not in ("noise", "ip_hidden_states")}
        one["ip_hidden_states"] = torch.cat([inp["ip_hidden_states"][i:i + 1], inp["ip_hidden_states"][B + i:B + i + 1]])
        one["noise"] = {k: (v[STEPS - n_i:, i:i + 1] if k == "steps" else v[i:i + 1]) for k, v in inp["noise"].items()}
        with torch.no_grad():
            lat_o = opipe.run(*m["oracle"], Scheduler("ddpm"), num_inference_steps=STEPS, guidance_scale=2.0, strength=s, return_latents=True, **one)
        err = pu.relerr(mixed[i:i + 1], lat_o)
        print(f"{dtype} person {i} at strength {s}: against the oracle {err:.3e} (bar {TOL[dtype]['latents']:.1e})")
        assert err <= TOL[dtype]["latents"], (i, err)


# ------------------------------------------------------------------------------------------------------------------ the call surface
def test_boundary_pipeline_takes_a_strength_per_person():
    """pipe(strength=[...], generator=[g0, g1, g2]): row i is row i of pipe(strength=s_i) with fresh generators of the same seeds -- with
    one generator per person, person i gets the draws its scalar call makes."""
    DT = torch.float16
    pipe, enc, kw = boundary_pipeline(DT)
    inp, _, call = boundary_inputs(kw, B, H, W, STEPS, DT)
    call.update(cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"], output_type="latent")
    seen = {}
    pipe.trace_call = seen

    def piped(strength):
        torch.manual_seed(123)                            # the pose posterior uses the GLOBAL generator
        gens = [torch.Generator(DEV).manual_seed(40 + i) for i in range(B)]
        return pipe(generator=gens, **{**call, "strength": strength})[0]

    mixed = piped(list(STRENGTHS))
    assert seen["strength"] == STRENGTHS and tuple(seen["noise"]["steps"].shape[:2]) == (max(N_ACTIVE), B) and seen["noise"]["image"] is not None
    assert torch.isfinite(mixed).all()
    for i, s in enumerate(STRENGTHS):
        one = piped(s)
        assert seen["strength"] == s and seen["noise"]["steps"].shape[0] == N_ACTIVE[i]            # a float crosses the boundary as ever
        assert torch.equal(mixed[i], one[i]), (i, s, (mixed[i] - one[i]).abs().max().item())
    for bad, match in (([1.0, 0.5], "`strength` has 2 values for 3 persons"), ([1.0, 1.5, 0.5], "`strength` lies in \\(0, 1\\]"),
                       ([1.0, 0.1, 0.5], "number of pipeline")):
        with pytest.raises(ValueError, match=match):
            piped(bad)
