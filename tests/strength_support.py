"""What the strength tests share: the issue's per-person strengths and step counts, the made-up argument struct of the refusal tests, the
coefficient row of idmvton_person_step, the poisoned eps rows of a dormant person, and the scalar-strength call a person of a mixed batch
is compared against (the same batch, the step noise sliced to that person's steps).  Importing this module needs no GPU and does not load
the native library."""
import torch

from tests.guidance_support import COEF

STEPS = 6                                                # the engine tests' schedule: blocks of 1, 2, 3 timesteps
STRENGTHS = [1.0, 0.5, 0.7]                              # B = 3: every step, the last int(6 * 0.5) = 3, the last int(6 * 0.7) = 4
N_ACTIVE = [6, 3, 4]
HW = 1100                                                # two statistics chunks of 1024 pixels, the second partial; a partial last apply workgroup
LDC = 8                                                  # > 4: channels 4.. hold NaN and are never read


def steps_of(strengths, n):
    """n_i = min(int(n * s_i), n): the reference's get_timesteps, per person."""
    return [min(int(n * s), n) for s in strengths]


def person_args(B=3, hw=195, ldc=64, branches=2, work_floats=None):
    """An idmvton_person_step_args with made-up pointers: every call of the CPU tests is refused before a launch, none is dereferenced."""
    from idm_vton_amd import ffi
    a = ffi.PersonStepArgs()
    a.dtype, a.B, a.hw, a.ldc, a.branches = ffi.BF16, B, hw, ldc, branches
    a.eps_nhwc, a.latents, a.noise, a.coef, a.work = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    a.work_floats = 8 * B * ((hw + 1023) // 1024) if work_floats is None else work_floats
    return a


def person_row(g, phi, active, device="cpu", coef=COEF):
    """{c_x, c_eps, sigma, g[B], phi[B], active[B]} as float32."""
    return torch.tensor(list(coef) + list(g) + list(phi) + [float(x) for x in active], dtype=torch.float32, device=device)


def poison_person(eps, b, B, branches):
    """eps [branches * B][hw][ldc] with person b's rows -- in every branch, every channel -- alternately NaN, +Inf and -Inf: what a dormant
    person's prediction may hold."""
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")]).to(eps.dtype)
    eps = eps.clone()
    for r in range(branches):
        eps[r * B + b] = bad[torch.arange(eps[b].numel()) % 3].reshape(eps[b].shape)
    return eps


def with_image_noise(inp, seed=77):
    """The inputs of engine_support.engine_inputs plus the posterior draw of the init-image encode, which a strength < 1 needs."""
    B, _, h, w = inp["noise"]["latents"].shape
    inp["noise"]["image"] = torch.randn(B, 4, h, w, generator=torch.Generator().manual_seed(seed))
    return inp


def scalar_call(kw, s, n):
    """The keywords of a per-person call -> those of the same batch at the scalar strength s: noise['steps'] is aligned to the loop's
    n_max steps, and the scalar call gets its last n_i of them."""
    steps = kw["noise"].get("steps")
    n_i = min(int(n * s), n)
    return {**kw, "strength": s, "noise": {**kw["noise"], "steps": None if steps is None else steps[steps.shape[0] - n_i:]}}
