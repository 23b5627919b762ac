"""What the row-plan tests share: the issue's worked example (4 steps, strengths [1.0, 0.5, 0.75], guidance [2, 1, 2]) with the rows it must
give, the made-up argument structs of the refusal tests, the device tables of idmvton_row_step / idmvton_pack_rows, the [uncond B | cond B]
eps tensor a plan's rows stand for, and the keywords of the engine calls.  Importing this module needs no GPU and does not load the native
library."""
import torch

from tests.guidance_support import COEF

STEPS = 4                                                # blocks of 1, 2, 1 timesteps
B = 3
STRENGTHS = [1.0, 0.5, 0.75]                             # n_i = 4, 2, 3: person 1 joins at loop step 2, person 2 at loop step 1
N_ACTIVE = [4, 2, 3]
GUIDANCE = [2.0, 1.0, 2.0]                               # person 1 has no guidance: it never has an unconditional row
R_PER_STEP = [2, 4, 5, 5]                                # u + a of loop steps 0 .. 3
SHAPES = [(2, 1), (4, 2), (5, 3)]                        # (R, a) of the three distinct plans
TOTAL = 16                                               # row-steps, against 4 * 2B = 24 under rows="all"
STEP2 = dict(full_rows=[0, 2, 3, 4, 5], urow=[0, -1, 1], crow=[2, 3, 4], row_person=[0, 2, 0, 1, 2])


def plans_of(n_b=N_ACTIVE, g_b=GUIDANCE, n_max=STEPS, persons=B):
    from idm_vton_amd.pipeline import TryonEngine
    return TryonEngine._row_plans(persons, n_b, g_b, n_max)


def row_args(B=3, R=5, hw=195, ldc=64, work_floats=None):
    """An idmvton_row_step_args with made-up pointers: every call of the CPU tests is refused before a launch, none is dereferenced."""
    from idm_vton_amd import ffi
    a = ffi.RowStepArgs()
    a.dtype, a.B, a.R, a.hw, a.ldc = ffi.BF16, B, R, hw, ldc
    a.eps_nhwc, a.latents, a.noise, a.coef, a.work, a.rows = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
    a.work_floats = 8 * B * ((hw + 1023) // 1024) if work_floats is None else work_floats
    return a


def pack_args(B=3, R=5, hw=195, cpad=16):
    from idm_vton_amd import ffi
    a = ffi.PackRowsArgs()
    a.dtype, a.B, a.R, a.hw, a.cpad = ffi.BF16, B, R, hw, cpad
    a.latents, a.cond, a.out, a.row_person = 0x10000, 0x20000, 0x30000, 0x40000
    return a


def table(urow, crow, device="cpu"):
    """{urow[B], crow[B]} as int32: what idmvton_row_step reads."""
    return torch.tensor(list(urow) + list(crow), dtype=torch.int32, device=device)


def plan_eps(full, urow, crow, R=None):
    """The [R][hw][ldc] eps of a plan from the [uncond B | cond B] tensor `full`: row urow[b] = full[b], row crow[b] = full[B + b]; every
    row no person owns (R may exceed the plan's rows) holds NaN, +Inf and -Inf in turn, in every channel."""
    nb = full.shape[0] // 2
    R = 1 + max(list(urow) + list(crow)) if R is None else R
    bad = torch.tensor([float("nan"), float("inf"), float("-inf")]).to(full.dtype)
    eps = bad[torch.arange(R * full[0].numel()) % 3].reshape((R,) + tuple(full.shape[1:]))
    for b in range(nb):
        if urow[b] >= 0:
            eps[urow[b]] = full[b]
        if crow[b] >= 0:
            eps[crow[b]] = full[nb + b]
    return eps


def coef_row(g, phi, device="cpu", coef=COEF):
    return torch.tensor(list(coef) + list(g) + list(phi), dtype=torch.float32, device=device)


def with_image_noise(inp, seed=77):
    """engine_support.engine_inputs plus the posterior draw of the init-image encode, which a strength < 1 needs."""
    nb, _, h, w = inp["noise"]["latents"].shape
    inp["noise"]["image"] = torch.randn(nb, 4, h, w, generator=torch.Generator().manual_seed(seed))
    return inp


def call_kw(base, cache, index, **over):
    """The worked example as an engine call on `cache`: base = engine_support.base_call(with_image_noise(inp), STEPS)."""
    return {**base, "cloth": cache, "garment_index": index, "strength": list(STRENGTHS), "guidance_scale": list(GUIDANCE), **over}
