"""Strength per person on the host (no GPU): idmvton_person_step's place in the C ABI -- exported, its struct described by idmvton_sizeof,
additive to ABI version 9, every refusal raised before a launch (the pointers are made up and never dereferenced) --, the coef-table
builder, the step counts against the scalar timestep lists, the argument errors of TryonEngine.prepare on a CPU engine with the stand-in
UNet of tests/garment_support.py, and the keys: a scalar strength is the call it always was."""
import ctypes as C
import os

import pytest
import torch

from tests.garment_support import DTYPE, standin_unet
from tests.guidance_support import G3, PHI3
from tests.strength_support import N_ACTIVE, STEPS, STRENGTHS, person_args, person_row, steps_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_person_step_is_additive_to_abi_9():
    from idm_vton_amd import ffi
    L = ffi.lib()
    header = open(os.path.join(ROOT, "include", "idmvton_hip.h")).read()
    assert "idmvton_person_step" in ffi.SYMBOLS and hasattr(L, "idmvton_person_step")
    assert "int idmvton_person_step(const idmvton_person_step_args* a, void* stream);" in header
    assert L.idmvton_sizeof(b"idmvton_person_step_args") == C.sizeof(ffi.PersonStepArgs) == 64
    assert ffi.STRUCTS["idmvton_person_step_args"] is ffi.PersonStepArgs and ffi.PersonStepArgs is not ffi.GuidedStepArgs
    assert L.idmvton_abi_version() == ffi.ABI_VERSION == 9
    assert L.idmvton_sizeof(b"idmvton_guided_step_args") == C.sizeof(ffi.GuidedStepArgs) == 64      # the guided step's struct is what it was
    assert L.idmvton_sizeof(b"idmvton_cfg_step_args") == C.sizeof(ffi.CfgStepArgs) == 48


@pytest.mark.parametrize("change, match", [
    (dict(eps_nhwc=None), "null pointer"), (dict(latents=None), "null pointer"), (dict(coef=None), "null pointer"), (dict(work=None), "null pointer"),
    (dict(B=0), "B=0"), (dict(B=-2), "B=-2"), (dict(B=65536), "B=65536"), (dict(hw=0), "hw=0"), (dict(ldc=3), "ldc=3"), (dict(dtype=2), "dtype 2"),
    (dict(dtype=3), "dtype 3"), (dict(branches=0), "branches=0"), (dict(branches=3), "branches=3"), (dict(work=0x50004), "8-byte aligned"),
    (dict(work_floats=23), "needs 24")])
def test_arg_validation_without_gpu(change, match):
    """Each as RuntimeError with the message of idmvton_last_error(), which names person_step; a launch on these pointers would not return
    an error code."""
    from idm_vton_amd import ffi
    a = person_args()
    for k, v in change.items():
        setattr(a, k, v)
    with pytest.raises(RuntimeError, match="person_step: .*" + match):
        ffi.call("idmvton_person_step", a, 0)


def test_refusal_codes_and_the_null_args_pointer():
    from idm_vton_amd import ffi
    L = ffi.lib()
    code = lambda **ch: (lambda a: ([setattr(a, k, v) for k, v in ch.items()], L.idmvton_person_step(C.byref(a), None))[1])(person_args())
    assert code(coef=None) == -5 and code(branches=4) == -5 and code(dtype=2) == -2 and code(hw=-1) == -1 and code(ldc=0) == -1
    assert code(work=0x50004) == -3 and code(work_floats=0) == -1
    assert L.idmvton_person_step(None, None) == -5
    a = person_args(branches=1)                           # the conditional branch alone has no statistics: no work buffer to refuse ...
    a.work, a.work_floats, a.hw = None, 0, 0
    assert L.idmvton_person_step(C.byref(a), None) == -1  # ... and the shape is still checked


def test_wrapper_checks_its_tensors_before_the_library(monkeypatch):
    from idm_vton_amd import ops
    monkeypatch.setattr(ops, "_call", lambda *a, **k: pytest.fail("launched"))
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else 0x1000)
    eps, lat = torch.zeros(6, 195, 4, dtype=torch.float16), torch.zeros(3, 4, 195)
    row = person_row(G3, PHI3, (1, 0, 1))
    with pytest.raises(ValueError, match="3 \\+ 3B = 12"):                       # a guided row (3 + 2B) is not a person row
        ops.person_step(eps, lat, None, row[:9], torch.zeros(24), 2)
    with pytest.raises(ValueError, match="branches=1"):
        ops.person_step(eps, lat, None, row, None, 1)
    with pytest.raises(ValueError, match="float32"):
        ops.person_step(eps, lat, None, row, torch.zeros(24, dtype=torch.float64), 2)


# ------------------------------------------------------------------------------------------------------------------ tables and step counts
@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_person_coef_table_is_the_guided_rows_plus_the_active_pattern(kind):
    from idm_vton_amd.scheduler import StepScheduler
    s = StepScheduler(kind)
    ts = s.set_timesteps(STEPS)
    guided, person = s.guided_coef_table(ts, G3, PHI3), s.person_coef_table(ts, G3, PHI3, N_ACTIVE)
    assert len(person) == STEPS and all(len(r) == 3 + 3 * 3 for r in person)
    assert [r[:9] for r in person] == guided
    assert [r[9:] for r in person] == [[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0]]
    assert [r[9:] for r in s.person_coef_table(ts, G3, PHI3, [6, 6, 6])] == [[1.0] * 3] * STEPS
    assert [r[9:] for r in s.person_coef_table(ts[3:], G3, PHI3, [1, 3, 2])] == [[0.0, 1.0, 0.0], [0.0, 1.0, 1.0], [1.0, 1.0, 1.0]]
    for bad, match in (([6, 3], "2 step counts for 3 persons"), ([6, 0, 4], "each in \\[1, 6\\]"), ([7, 3, 4], "each in \\[1, 6\\]")):
        with pytest.raises(ValueError, match=match):
            s.person_coef_table(ts, G3, PHI3, bad)


@pytest.mark.parametrize("n, want", [(6, [6, 3, 4, 5]), (30, [30, 15, 21, 29])])
def test_step_counts_are_the_scalar_timestep_lists(n, want):
    """n_i = min(int(n * s_i), n) per person, the length of the scalar call's list; every person's list is a suffix of the longest, which
    is the list of the largest strength -- the one the loop runs."""
    from idm_vton_amd.pipeline import TryonEngine
    strengths = [1.0, 0.5, 0.7, 0.9999]
    s_b, n_b = TryonEngine._person_steps(4, strengths, n)
    assert s_b == strengths and n_b == want == steps_of(strengths, n)
    longest = TryonEngine._timesteps("ddpm", n, max(strengths))[1]
    assert len(longest) == max(n_b)
    for s, n_i in zip(strengths, n_b):
        own = TryonEngine._timesteps("ddpm", n, s)[1]
        assert len(own) == n_i and list(own) == list(longest[len(longest) - n_i:])
    assert steps_of(STRENGTHS, STEPS) == N_ACTIVE


def test_a_scalar_strength_is_no_person_state():
    """Floats, 0-d arrays and 0-d tensors are scalars: no parsing, no new key in the graph key; a sequence adds ("person", branches)."""
    import numpy as np
    from idm_vton_amd.pipeline import TryonEngine
    for scalar in (1.0, 0.5, 1, np.float32(0.5), torch.tensor(0.5), float("nan"), 7.0):
        assert TryonEngine._person_steps(3, scalar, 6) == (None, None)
    assert TryonEngine._person_steps(3, (1.0, 0.5, 0.7), 6) == (STRENGTHS, N_ACTIVE)
    assert TryonEngine._person_steps(3, torch.tensor([1.0, 0.5, 0.75]), 6) == ([1.0, 0.5, 0.75], [6, 3, 4])
    assert TryonEngine._person_steps(1, [0.5], 6) == ([0.5], [3])                # a sequence of one is a sequence
    st = dict(B=3, h=16, w=16, gh=16, gw=16, k=2, steps_noise=None)
    key = TryonEngine._graph_key
    assert key(st, True) == (3, 16, 16, 16, 16, 2, False)                         # what it was on the parent commit
    assert key(dict(st, guided=False, branches=2, work=None), True) == key(st, True)
    assert key(dict(st, guided=True, branches=2), True) == key(st, True) + (("guided", 2),)
    assert key(dict(st, guided=False, branches=2, person=True), True) == key(st, True) + (("person", 2),)
    assert key(dict(st, guided=True, branches=2, person=True), True) == key(st, True) + (("person", 2),)
    assert key(dict(st, guided=True, branches=1, person=True), True) == key(st, True) + (("person", 1),)


# ------------------------------------------------------------------------------------------------------------------ engine arguments
def _cpu_engine(monkeypatch):
    from idm_vton_amd import ffi
    from idm_vton_amd.pipeline import TryonEngine
    for name in ("call", "call_shared", "call_indexed", "call_ragged"):
        monkeypatch.setattr(ffi, name, lambda *a, **k: pytest.fail("a launch before the refusal"))
    return TryonEngine(standin_unet([]), None, None, dtype=DTYPE, device="cpu")


def _kw(**over):
    z = lambda c: torch.zeros(3, c, 16, 16)
    kw = dict(image=z(3), mask_image=z(1), pose_img=z(3), cloth=z(3), prompt_embeds=None, negative_prompt_embeds=None,
              pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, text_embeds_cloth=None, noise={}, num_inference_steps=6, guidance_scale=2.0)
    kw.update(over)
    return kw


BAD = [(dict(strength=[1.0, 0.5]), "`strength` has 2 values for 3 persons"),
       (dict(strength=[0.5] * 4), "`strength` has 4 values for 3 persons"),
       (dict(strength=torch.ones(3, 1)), "`strength` takes a float or a sequence of 3 floats"),
       (dict(strength=[1.0, 0.0, 0.5]), "`strength` lies in \\(0, 1\\]"),
       (dict(strength=[1.0, 1.5, 0.5]), "`strength` lies in \\(0, 1\\]"),
       (dict(strength=[1.0, -0.5, 0.5]), "`strength` lies in \\(0, 1\\]"),
       (dict(strength=[1.0, float("nan"), 0.5]), "`strength` holds NaN"),
       (dict(strength=[1.0, 0.1, 0.5]), "strength parameter: 0.1, the number of pipelinesteps is 0 which is < 1"),      # int(6 * 0.1) = 0
       (dict(strength=[1.0, 0.5, 0.7]), "strength < 1 starts from add_noise\\(encode\\(image\\)\\): pass .* noise\\['image'\\]")]


@pytest.mark.parametrize("over, match", BAD)
def test_prepare_refuses_before_anything_is_launched(over, match, monkeypatch):
    eng = _cpu_engine(monkeypatch)
    with pytest.raises(ValueError, match=match):
        eng.prepare(**_kw(**over))


@pytest.mark.parametrize("over, match", BAD[:1] + BAD[3:4] + BAD[-2:])
def test_call_refuses_before_anything_is_launched(over, match, monkeypatch):
    eng = _cpu_engine(monkeypatch)
    with pytest.raises(ValueError, match=match):
        eng(use_graph=True, overlap=True, **_kw(**over))
