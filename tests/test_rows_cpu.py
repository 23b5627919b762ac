"""The row plan on the host (no GPU): TryonEngine._row_plans on the issue's worked example and its properties over drawn step counts and
guidance scales; the calls it leaves alone; the two kernels' place in the C ABI -- exported, their structs described by idmvton_sizeof,
additive to ABI version 9, every refusal raised before a launch (the pointers are made up and never dereferenced) --; the engine's
refusals on a CPU engine with the stand-in UNet of tests/garment_support.py; the graph key; and the boundary pipeline's `rows` attribute."""
import ctypes as C
import itertools
import os
import random

import pytest
import torch

from tests.garment_support import DTYPE, pool_cache, standin_unet
from tests.rows_support import B, GUIDANCE, N_ACTIVE, R_PER_STEP, SHAPES, STEP2, STEPS, TOTAL, pack_args, plans_of, row_args, table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the plan builder
def test_the_worked_example():
    index, plans = plans_of()
    assert [plans[i]["R"] for i in index] == R_PER_STEP and sum(plans[i]["R"] for i in index) == TOTAL < STEPS * 2 * B
    assert [(p["R"], p["a"]) for p in plans] == SHAPES and index == [0, 1, 2, 2]
    p = plans[index[2]]
    assert (p["full_rows"], p["urow"], p["crow"], p["row_person"]) == (STEP2["full_rows"], STEP2["urow"], STEP2["crow"], STEP2["row_person"])
    assert p["persons"] == [0, 1, 2] and p["uncond"] == [0, 2] and (p["u"], p["a"]) == (2, 3)
    first = plans[index[0]]                               # person 0 alone, with guidance: its two rows
    assert (first["full_rows"], first["urow"], first["crow"], first["row_person"]) == ([0, 3], [0, -1, -1], [1, -1, -1], [0, 0])
    second = plans[index[1]]                              # persons 0 and 2
    assert (second["full_rows"], second["urow"], second["crow"], second["row_person"]) == ([0, 2, 3, 5], [0, -1, 1], [2, -1, 3], [0, 2, 0, 2])


@pytest.mark.parametrize("n_b, g_b, persons", [
    (None, [2.0, 7.5, 1.5], 3),                           # a scalar strength, everyone with guidance: the plain / guided state
    ([3, 3, 3], [2.0, 7.5, 1.5], 3),                      # all strengths equal (n_max = 3): the person state
    (None, [1.0, 1.0, 0.5], 3), ([4, 4, 4], [1.0, 1.0, 1.0], 3),    # nobody with guidance, nobody dormant: today's branches = 1 state
    (None, [2.0], 1), (None, [1.0], 1), ([4], [2.0], 1)])           # B = 1
def test_nothing_to_skip_is_no_plan(n_b, g_b, persons):
    assert plans_of(n_b, g_b, max(n_b) if n_b else STEPS, persons) is None


def test_a_mixed_guidance_or_a_dormant_step_is_a_plan():
    index, plans = plans_of(None, [7.5, 2.0, 1.0])        # the guidance feature's mixed batch: person 2's unconditional row goes
    assert index == [0] * STEPS and [(p["R"], p["a"]) for p in plans] == [(5, 3)] and plans[0]["urow"] == [0, 1, -1]
    index, plans = plans_of([4, 2], [2.0, 2.0], 4, 2)     # the strength feature's [1.0, 0.5] batch: 2 + 2 + 4 + 4 of 16 row-steps
    assert [plans[i]["R"] for i in index] == [2, 2, 4, 4]
    index, plans = plans_of([4, 2, 3], [1.0, 0.5, 1.0])   # nobody with guidance, but dormant steps: conditional rows alone
    assert [plans[i]["R"] for i in index] == [1, 2, 3, 3] and all(p["u"] == 0 and p["urow"] == [-1] * 3 for p in plans)


def test_properties_over_drawn_step_counts_and_guidance():
    rng = random.Random(5)
    cases = [(nb, n_max, [rng.choice([1, n_max, rng.randint(1, n_max)]) for _ in range(nb)], [rng.choice([0.0, 1.0, 1.5, 7.5]) for _ in range(nb)])
             for nb in (1, 2, 3, 4) for n_max in (1, 2, 5, 8) for _ in range(12)]
    cases += [(nb, 3, list(n), list(g)) for nb in (2, 3) for n in itertools.product((1, 2, 3), repeat=nb) for g in itertools.product((1.0, 2.0), repeat=nb)]
    seen = 0
    for nb, n_max, n_b, g_b in cases:
        n_b[0] = n_max                                    # the loop runs the longest list: somebody has it
        got = plans_of(n_b, g_b, n_max, nb)
        full = all(n == n_max for n in n_b)
        if got is None:
            assert full and len({g > 1 for g in g_b}) == 1, (n_b, g_b)
            continue
        seen += 1
        index, plans = got
        assert len(index) == n_max and len(plans) <= nb and len({(p["R"], p["a"]) for p in plans}) == len(plans)
        before = set()
        for j, pi in enumerate(index):
            p = plans[pi]
            active = [i for i in range(nb) if j >= n_max - n_b[i]]
            assert p["persons"] == active and before <= set(active)                               # nested over the loop
            before = set(active)
            assert [i for i in range(nb) if p["crow"][i] >= 0] == active
            assert [i for i in range(nb) if p["urow"][i] >= 0] == [i for i in active if g_b[i] > 1] == p["uncond"]
            assert sorted(p["crow"][i] for i in active) == list(range(p["R"] - p["a"], p["R"]))   # the conditional rows are the last a
            assert [p["crow"][i] for i in active] == sorted(p["crow"][i] for i in active)         # ... in ascending person order
            assert sorted(p["urow"][i] for i in p["uncond"]) == list(range(p["u"])) and p["R"] == p["u"] + p["a"] <= 2 * nb
            assert p["row_person"] == p["uncond"] + active
            assert p["full_rows"] == p["uncond"] + [nb + i for i in active]
            assert all(p["row_person"][p["crow"][i]] == i for i in active) and all(p["row_person"][p["urow"][i]] == i for i in p["uncond"])
        assert any(plans[pi]["R"] < 2 * nb for pi in index)
    assert seen > 100


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_the_two_kernels_are_additive_to_abi_9():
    from idm_vton_amd import ffi
    L = ffi.lib()
    header = open(os.path.join(ROOT, "include", "idmvton_hip.h")).read()
    for name in ("idmvton_pack_rows", "idmvton_row_step"):
        assert name in ffi.SYMBOLS and hasattr(L, name)
        assert f"int {name}(const {name}_args* a, void* stream);" in header
    assert L.idmvton_sizeof(b"idmvton_pack_rows_args") == C.sizeof(ffi.PackRowsArgs) == 56
    assert L.idmvton_sizeof(b"idmvton_row_step_args") == C.sizeof(ffi.RowStepArgs) == 72
    assert L.idmvton_abi_version() == ffi.ABI_VERSION == 9
    assert L.idmvton_sizeof(b"idmvton_person_step_args") == 64 and L.idmvton_sizeof(b"idmvton_guided_step_args") == 64
    assert L.idmvton_sizeof(b"idmvton_pack_input_args") == C.sizeof(ffi.PackInputArgs) == 40


@pytest.mark.parametrize("change, match", [
    (dict(eps_nhwc=None), "null pointer"), (dict(latents=None), "null pointer"), (dict(coef=None), "null pointer"), (dict(work=None), "null pointer"),
    (dict(rows=None), "null pointer"), (dict(B=0), "B=0"), (dict(B=65536), "B=65536"), (dict(R=0), "R=0"), (dict(R=-1), "R=-1"), (dict(R=65536), "R=65536"),
    (dict(hw=0), "hw=0"), (dict(ldc=3), "ldc=3"), (dict(dtype=2), "dtype 2"), (dict(work=0x50004), "8-byte aligned"), (dict(work_floats=23), "needs 24")])
def test_row_step_refuses_without_gpu(change, match):
    from idm_vton_amd import ffi
    a = row_args()
    for k, v in change.items():
        setattr(a, k, v)
    with pytest.raises(RuntimeError, match="row_step: .*" + match):
        ffi.call("idmvton_row_step", a, 0)


@pytest.mark.parametrize("change, match", [
    (dict(latents=None), "null pointer"), (dict(cond=None), "null pointer"), (dict(out=None), "null pointer"), (dict(row_person=None), "null pointer"),
    (dict(B=0), "B=0"), (dict(R=0), "R=0"), (dict(hw=0), "hw=0"), (dict(cpad=12), "cpad=12"), (dict(R=40000, hw=60000), "R=40000"), (dict(dtype=3), "dtype 3")])
def test_pack_rows_refuses_without_gpu(change, match):
    from idm_vton_amd import ffi
    a = pack_args()
    for k, v in change.items():
        setattr(a, k, v)
    with pytest.raises(RuntimeError, match="pack_rows: .*" + match):
        ffi.call("idmvton_pack_rows", a, 0)


def test_refusal_codes():
    from idm_vton_amd import ffi
    L = ffi.lib()
    code = lambda fn, a, **ch: ([setattr(a, k, v) for k, v in ch.items()], getattr(L, fn)(C.byref(a), None))[1]
    assert code("idmvton_row_step", row_args(), rows=None) == -5 and code("idmvton_row_step", row_args(), R=0) == -1
    assert code("idmvton_row_step", row_args(), dtype=2) == -2 and code("idmvton_row_step", row_args(), work=0x50004) == -3
    assert code("idmvton_pack_rows", pack_args(), row_person=None) == -5 and code("idmvton_pack_rows", pack_args(), R=0) == -1
    assert L.idmvton_row_step(None, None) == -5 and L.idmvton_pack_rows(None, None) == -5


def test_wrappers_check_their_tensors_before_the_library(monkeypatch):
    from idm_vton_amd import ops
    monkeypatch.setattr(ops, "_call", lambda *a, **k: pytest.fail("launched"))
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else 0x1000)
    eps, lat = torch.zeros(5, 195, 4, dtype=torch.float16), torch.zeros(3, 4, 195)
    row, tab = torch.zeros(9), table(STEP2["urow"], STEP2["crow"])
    with pytest.raises(ValueError, match="3 \\+ 2B = 9"):                        # a person row (3 + 3B) is not what row_step reads
        ops.row_step(eps, lat, None, torch.zeros(12), torch.zeros(24), tab)
    with pytest.raises(ValueError, match="needs 6 contiguous int32"):
        ops.row_step(eps, lat, None, row, torch.zeros(24), tab[:5])
    with pytest.raises(ValueError, match="needs 6 contiguous int32"):
        ops.row_step(eps, lat, None, row, torch.zeros(24), tab.long())
    with pytest.raises(ValueError, match="work must be a float32 tensor"):
        ops.row_step(eps, lat, None, row, None, tab)
    cond, out = torch.zeros(3, 195, 9, dtype=torch.float16), torch.zeros(5, 195, 16, dtype=torch.float16)
    with pytest.raises(ValueError, match="needs 5 contiguous int32"):
        ops.pack_rows(lat, cond, out, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(ValueError, match="one per person"):                      # the duplicated [2B] buffer of pack_input is not taken
        ops.pack_rows(lat, torch.cat([cond, cond]), out, torch.zeros(5, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------------------ engine arguments, keys
def _cpu_engine(monkeypatch, fp8=False):
    from idm_vton_amd import ffi
    from idm_vton_amd.pipeline import TryonEngine
    for name in ("call", "call_shared", "call_indexed", "call_ragged"):
        monkeypatch.setattr(ffi, name, lambda *a, **k: pytest.fail("a launch before the refusal"))
    unet = standin_unet([])
    unet.attn_fp8 = fp8
    return TryonEngine(unet, None, None, dtype=DTYPE, device="cpu")


def _kw(**over):
    z = lambda c: torch.zeros(3, c, 16, 16)
    kw = dict(image=z(3), mask_image=z(1), pose_img=z(3), cloth=z(3), prompt_embeds=None, negative_prompt_embeds=None,
              pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, text_embeds_cloth=None, noise={}, num_inference_steps=STEPS,
              guidance_scale=list(GUIDANCE))
    kw.update(over)
    return kw


def test_prepare_and_call_refuse_before_anything_is_launched(monkeypatch):
    eng = _cpu_engine(monkeypatch)
    for run in (eng.prepare, lambda **kw: eng(use_graph=True, overlap=True, **kw)):
        with pytest.raises(ValueError, match="rows='some'"):
            run(**_kw(rows="some"))
        with pytest.raises(ValueError, match="rows=None"):
            run(**_kw(rows=None))
        with pytest.raises(ValueError, match="rows=\"needed\".* an index on a live call is still out"):
            run(**_kw(rows="needed"))
    with pytest.raises(ValueError, match="rows=\"needed\": attn_fp8"):
        _cpu_engine(monkeypatch, fp8=True).prepare(**_kw(rows="needed", cloth=pool_cache(G=3)))


def test_the_graph_key_of_a_row_state():
    from idm_vton_amd.pipeline import TryonEngine
    st = dict(B=3, h=16, w=16, gh=16, gw=16, k=2, steps_noise=None, gindex=[2, 0, 1], gcache=None)
    key = TryonEngine._graph_key
    cached = (3, 16, 16, 16, 16, 2, False, "cached", "indexed")
    assert key(st, False) == cached                                               # what it was on the parent commit
    assert key(dict(st, guided=True, branches=2), False) == cached + (("guided", 2),)
    assert key(dict(st, guided=True, branches=2, rows=dict(step=[0], plans=[{}])), False) == cached + (("rows", 2),)
    assert key(dict(st, guided=True, branches=2, rows=None), False) == cached + (("guided", 2),)
    assert TryonEngine.ROWS == ("all", "needed")
    assert N_ACTIVE == [min(int(STEPS * s), STEPS) for s in (1.0, 0.5, 0.75)]


# ------------------------------------------------------------------------------------------------------------------ the boundary pipeline
def _pipe():
    from idm_vton_amd.boundary.tryon_pipeline import StableDiffusionXLInpaintPipeline
    from types import SimpleNamespace
    vae = SimpleNamespace(config=SimpleNamespace(block_out_channels=(32, 32, 32, 32)))   # the constructor reads the VAE's depth, nothing else
    return StableDiffusionXLInpaintPipeline(vae, None, None, None, None, None, None, None)


def test_boundary_pipeline_passes_rows_only_when_it_says_something():
    pipe = _pipe()
    assert pipe.rows == "all" and pipe._rows_keyword() == {}                      # the engine call is, keyword for keyword, what it was
    pipe.rows = "needed"
    assert pipe._rows_keyword() == {"rows": "needed"}
    for bad in ("some", None, True):
        pipe.rows = bad
        with pytest.raises(ValueError, match="rows="):
            pipe._rows_keyword()
        with pytest.raises(ValueError, match="rows="):                            # the call refuses it before it looks at any argument
            pipe()
