"""Per-person guidance on the host (no GPU): idmvton_guided_step's place in the C ABI -- exported, its struct described by idmvton_sizeof,
additive to ABI version 9, every refusal raised before a launch (the pointers are made up and never dereferenced) --, the coef-table
builder, the restated formula's own sanity, and the argument errors of TryonEngine.prepare / __call__ on a CPU engine with the stand-in
UNet of tests/garment_support.py."""
import ctypes as C
import os

import pytest
import torch

from tests.garment_support import DTYPE, standin_unet
from tests.guidance_support import COEF, G3, PHI3, coef_row, formula, guided_args, operands

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_guided_step_is_additive_to_abi_9():
    from idm_vton_amd import ffi
    L = ffi.lib()
    header = open(os.path.join(ROOT, "include", "idmvton_hip.h")).read()
    for s in ("idmvton_guided_step", "idmvton_guided_step_work_floats", "idmvton_pack_input_cond"):
        assert s in ffi.SYMBOLS and hasattr(L, s) and s + "(" in header, s
    assert L.idmvton_sizeof(b"idmvton_guided_step_args") == C.sizeof(ffi.GuidedStepArgs) == 64
    assert ffi.STRUCTS["idmvton_guided_step_args"] is ffi.GuidedStepArgs
    assert L.idmvton_abi_version() == ffi.ABI_VERSION == 9
    assert L.idmvton_sizeof(b"idmvton_cfg_step_args") == C.sizeof(ffi.CfgStepArgs) == 48      # the plain step's struct is what it was


def test_work_floats():
    from idm_vton_amd import ffi
    L = ffi.lib()
    f = L.idmvton_guided_step_work_floats
    assert [f(1, 1), f(1, 1024), f(1, 1025), f(3, 195), f(3, 4103), f(2, 96 * 128)] == [8, 8, 16, 24, 120, 192]
    assert f(0, 5) == f(5, 0) == f(-1, 5) == -1 and f(1 << 20, 1 << 30) == -1


@pytest.mark.parametrize("change, match", [
    (dict(eps_nhwc=None), "null pointer"), (dict(latents=None), "null pointer"), (dict(coef=None), "null pointer"), (dict(work=None), "null pointer"),
    (dict(B=0), "B=0"), (dict(B=-2), "B=-2"), (dict(hw=0), "hw=0"), (dict(ldc=3), "ldc=3"), (dict(dtype=2), "dtype 2"), (dict(dtype=3), "dtype 3"),
    (dict(branches=0), "branches=0"), (dict(branches=3), "branches=3"), (dict(work=0x50004), "8-byte aligned"), (dict(work_floats=23), "needs 24")])
def test_refusals_arrive_before_any_launch(change, match):
    """Each as RuntimeError with the message of idmvton_last_error(); a launch on these pointers would not return an error code."""
    from idm_vton_amd import ffi
    a = guided_args()
    for k, v in change.items():
        setattr(a, k, v)
    with pytest.raises(RuntimeError, match=match):
        ffi.call("idmvton_guided_step", a, 0)


def test_refusal_codes_and_the_null_args_pointer():
    from idm_vton_amd import ffi
    L = ffi.lib()
    code = lambda **ch: (lambda a: ([setattr(a, k, v) for k, v in ch.items()], L.idmvton_guided_step(C.byref(a), None))[1])(guided_args())
    assert code(coef=None) == -5 and code(branches=4) == -5 and code(dtype=2) == -2 and code(hw=-1) == -1 and code(ldc=0) == -1
    assert code(work=0x50004) == -3 and code(work_floats=0) == -1
    assert L.idmvton_guided_step(None, None) == -5
    a = guided_args(branches=1)                           # the conditional branch alone has no statistics: no work buffer to refuse ...
    a.work, a.work_floats, a.hw = None, 0, 0
    assert L.idmvton_guided_step(C.byref(a), None) == -1  # ... and the shape is still checked
    p = ffi.PackInputArgs()
    p.dtype, p.B, p.hw, p.cpad, p.latents, p.cond, p.out = ffi.F16, 2, 16, 12, 0x10000, 0x20000, 0x30000
    with pytest.raises(RuntimeError, match="cpad=12"):
        ffi.call("idmvton_pack_input_cond", p, 0)
    p.cpad, p.cond = 64, None
    with pytest.raises(RuntimeError, match="null pointer"):
        ffi.call("idmvton_pack_input_cond", p, 0)


def test_wrapper_checks_its_tensors_before_the_library(monkeypatch):
    from idm_vton_amd import ops
    monkeypatch.setattr(ops, "_call", lambda *a, **k: pytest.fail("launched"))
    monkeypatch.setattr(ops, "_ptr", lambda t: None if t is None else 0x1000)
    eps, lat = torch.zeros(6, 195, 4, dtype=torch.float16), torch.zeros(3, 4, 195)
    with pytest.raises(ValueError, match="3 \\+ 2B = 9"):
        ops.guided_step(eps, lat, None, torch.zeros(4), torch.zeros(24), 2)
    with pytest.raises(ValueError, match="branches=1"):
        ops.guided_step(eps, lat, None, coef_row(G3, PHI3), None, 1)
    with pytest.raises(ValueError, match="float32"):
        ops.guided_step(eps, lat, None, coef_row(G3, PHI3), torch.zeros(24, dtype=torch.float64), 2)


# ------------------------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("kind", ["ddpm", "ddim"])
def test_coef_tables_against_the_scheduler(kind):
    from idm_vton_amd.scheduler import StepScheduler
    s = StepScheduler(kind)
    ts = s.set_timesteps(5)
    plain, guided = s.coef_table(ts, 2.0), s.guided_coef_table(ts, G3, PHI3)
    assert len(plain) == len(guided) == 5
    for t, p, g in zip(ts, plain, guided):
        assert p == list(s.coeffs(t)) + [2.0] and len(p) == 4
        assert g == list(s.coeffs(t)) + list(G3) + list(PHI3) and len(g) == 3 + 2 * 3
    with pytest.raises(ValueError, match="3 guidance scales and 2 rescales"):
        s.guided_coef_table(ts, G3, PHI3[:2])


def test_per_person():
    import numpy as np
    from idm_vton_amd.scheduler import per_person
    assert per_person(2, 3, "g") == ([2.0] * 3, False) and per_person(np.float32(0.5), 2, "g") == ([0.5, 0.5], False)
    assert per_person(torch.tensor(1.5), 2, "g") == ([1.5, 1.5], False)
    assert per_person([1, 2.5], 2, "g") == ([1.0, 2.5], True) and per_person(torch.tensor([1.0, 2.0]), 2, "g") == ([1.0, 2.0], True)
    assert per_person((3.0,), 1, "g") == ([3.0], True)
    for bad in ([1.0], [1.0, 2.0, 3.0], [], torch.zeros(2, 2), ["a", "b"], [1.0, float("nan")]):
        with pytest.raises(ValueError, match="`guidance_scale`"):
            per_person(bad, 2, "guidance_scale")


def test_the_restated_formula_is_the_reference_rescale():
    """tests/guidance_support.formula against rescale_noise_cfg as the reference writes it (std over dims 1.., keepdim), in fp64."""
    eps, lat, noise = operands(3, 195, 4, torch.float16)
    got = formula(eps, lat, noise, coef_row(G3, PHI3), 2, torch.float64)
    e = eps.double().reshape(2, 3, 195, 4).permute(0, 1, 3, 2)
    row = coef_row(G3, PHI3).double()                     # the values as the kernel reads them: rounded to fp32 (0.7 is not a float)
    for b, (g, phi) in enumerate(zip(row[3:6].tolist(), row[6:9].tolist())):
        u, t = e[0, b:b + 1], e[1, b:b + 1]
        cfg = u + g * (t - u)
        if phi > 0:
            std_text, std_cfg = t.std(dim=[1, 2], keepdim=True), cfg.std(dim=[1, 2], keepdim=True)
            cfg = phi * (cfg * (std_text / std_cfg)) + (1 - phi) * cfg
        c = [float(torch.tensor(v, dtype=torch.float32)) for v in COEF]
        want = c[0] * lat[b:b + 1].double() + c[1] * cfg + c[2] * noise[b:b + 1].double()
        assert torch.allclose(got[b:b + 1], want, rtol=1e-13, atol=1e-13), b
    one = formula(eps[:3], lat, None, coef_row(G3, PHI3), 1, torch.float64)        # branches 1: e = t, no rescale whatever phi says
    c = coef_row(G3, PHI3).double()
    assert torch.equal(one, c[0] * lat.double() + c[1] * eps[:3].double().permute(0, 2, 1))


# ------------------------------------------------------------------------------------------------------------------ engine arguments
def _cpu_engine(monkeypatch):
    from idm_vton_amd import ffi
    from idm_vton_amd.pipeline import TryonEngine
    for name in ("call", "call_shared", "call_indexed", "call_ragged"):
        monkeypatch.setattr(ffi, name, lambda *a, **k: pytest.fail("a launch before the refusal"))
    return TryonEngine(standin_unet([]), None, None, dtype=DTYPE, device="cpu")


def _kw(**over):
    kw = dict(image=torch.zeros(3, 3, 16, 16), mask_image=None, pose_img=None, cloth=None, prompt_embeds=None, negative_prompt_embeds=None,
              pooled_prompt_embeds=None, negative_pooled_prompt_embeds=None, text_embeds_cloth=None, noise={}, num_inference_steps=3, guidance_scale=2.0)
    kw.update(over)
    return kw


BAD = [(dict(guidance_scale=[7.5, 2.0]), "`guidance_scale` has 2 values for 3 persons"),
       (dict(guidance_scale=[1.0] * 4), "`guidance_scale` has 4 values for 3 persons"),
       (dict(guidance_rescale=[0.0, 0.7]), "`guidance_rescale` has 2 values for 3 persons"),
       (dict(guidance_rescale=1.5), "`guidance_rescale` lies in \\[0, 1\\]"),
       (dict(guidance_rescale=[0.0, -0.1, 0.5]), "`guidance_rescale` lies in \\[0, 1\\]"),
       (dict(guidance_rescale=float("nan")), "`guidance_rescale` holds NaN"),
       (dict(uncond="drop"), "uncond='drop'"),
       (dict(uncond="skip"), "uncond=\"skip\""),                                     # the default scalar 2.0
       (dict(uncond="skip", guidance_scale=[1.0, 1.0, 1.5]), "uncond=\"skip\"")]


@pytest.mark.parametrize("over, match", BAD)
def test_prepare_refuses_before_anything_is_launched(over, match, monkeypatch):
    eng = _cpu_engine(monkeypatch)
    with pytest.raises(ValueError, match=match):
        eng.prepare(**_kw(**over))


@pytest.mark.parametrize("over, match", BAD[:1] + BAD[3:4] + BAD[-1:])
def test_call_refuses_before_anything_is_launched(over, match, monkeypatch):
    eng = _cpu_engine(monkeypatch)
    with pytest.raises(ValueError, match=match):
        eng(use_graph=True, overlap=True, **_kw(**over))


def test_guidance_resolution_and_keys():
    """Which state a request gets, what a person without guidance runs with, and that a plain state's keys are what they were."""
    from idm_vton_amd.pipeline import TryonEngine
    G = TryonEngine._guidance
    assert G(3, 2.0, 0.0, "run") == ([2.0] * 3, [0.0] * 3, False, False)                     # plain
    assert G(3, 0.5, 0.0, "run") == ([1.0] * 3, [0.0] * 3, False, False)                     # plain, guidance 1
    assert G(3, [2, 2, 2], [0, 0, 0], "run") == ([2.0] * 3, [0.0] * 3, True, False)          # equal lists: guided all the same
    assert G(3, 2.0, 0.7, "run") == ([2.0] * 3, [0.7] * 3, True, False)
    assert G(3, G3, PHI3, "run") == ([7.5, 2.0, 1.0], [0.0, 0.7, 0.0], True, False)          # no rescale without CFG
    assert G(2, [0.0, 1.0], 1.0, "skip") == ([1.0, 1.0], [0.0, 0.0], True, True)
    st = dict(B=3, h=16, w=16, gh=16, gw=16, k=2, steps_noise=None)
    key = TryonEngine._graph_key
    assert key(st, True) == (3, 16, 16, 16, 16, 2, False) and TryonEngine._set_key(st) == (3, 16, 16, 2)
    assert key(dict(st, guided=False, branches=2), True) == key(st, True)
    assert key(dict(st, guided=True, branches=2), True) == key(st, True) + (("guided", 2),)
    assert key(dict(st, guided=True, branches=1), True) == key(st, True) + (("guided", 1),)
    assert TryonEngine._set_key(dict(st, branches=1)) == (3, 16, 16, 2, "cond-only")
