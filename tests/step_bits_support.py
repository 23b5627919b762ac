"""The deterministic launches whose result bits tests/golden/step_bits.json pins: every form of idmvton_guided_step, idmvton_person_step and
idmvton_row_step, and the three pack kernels, on operands drawn on the CPU from fixed seeds (guidance_support.operands).  The case list is
shared by the test (tests/test_step_bits_gpu.py) and the recorder (tools/gpu_step_bits.py); a case is keyed by its name.  Importing this
module needs no GPU and does not load the native library."""
import functools
import hashlib

import torch

from tests.guidance_support import G3, HWS, PHI3, coef_row, operands
from tests.rows_support import plan_eps, table

B = 3
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
LDCS = (64, 4)                                           # 64: NaN in channels 4 and up (never read); 4: the channels alone
NAN = float("nan")

# step -> (entry, its last argument or None for "the default row table", what the case does to the operands)
STEPS = {
    "guided_b2": ("guided_step", 2, None),
    "guided_b1": ("guided_step", 1, None),
    "person_active": ("person_step", 2, (1, 1, 1)),
    "person_dormant": ("person_step", 2, (1, 0, 1)),     # the middle person dormant, its eps rows NaN
    "row_both": ("row_step", ([6, 1, 3], [0, 7, 4]), 8),                     # (urow, crow), R: rows 2 and 5 belong to nobody
    "row_no_urow": ("row_step", ([0, -1, 1], [2, 3, 4]), 5),                 # person 1: e = t
    "row_no_crow": ("row_step", ([0, 5, 1], [2, -1, 3]), 7),                 # person 1 dormant; its urow names a row nobody owns
    "row_clamped": ("row_step", ([0, -7, 2], [3, 4, 2 ** 31 - 1]), 6),       # -7 -> -1, 2^31 - 1 -> R - 1 = 5
}
PACKS = ("pack_input", "pack_input_cond", "pack_rows")
ROW_PERSON = [2, 0, 2, 1, 0]                             # pack_rows: R = 5, a permutation with repeats

CASES = tuple(f"{step}-hw{hw}-{dt}-ldc{ldc}-{nz}" for step in STEPS for hw in HWS for dt in DTYPES for ldc in LDCS for nz in ("noise", "null_noise")) \
    + tuple(f"{pack}-hw{hw}-{dt}" for pack in PACKS for hw in HWS for dt in DTYPES)


@functools.lru_cache(maxsize=None)
def _operands(hw, ldc, dt):
    return operands(B, hw, ldc, DTYPES[dt])              # (never modified: a case clones what it changes)


def work_pattern(n):
    """The fixed pattern `work` holds before a launch, so that a digest covers the regions a launch must leave alone."""
    return torch.arange(n, dtype=torch.float32) * 0.5 + 0.25


def run(name, device):
    """Case `name` on `device` -> {what: tensor on the CPU}: latents and work of a step, out of a pack kernel."""
    from idm_vton_amd import ops
    parts = name.split("-")
    hw, dt = int(parts[1][2:]), parts[2]
    if parts[0] in PACKS:
        g = torch.Generator().manual_seed(hw)
        rows = {"pack_input": 2 * B, "pack_input_cond": B, "pack_rows": B}[parts[0]]
        lat, cond = torch.randn(B, 4, hw, generator=g).to(device), torch.randn(rows, hw, 9, generator=g).to(DTYPES[dt]).to(device)
        out = torch.full((len(ROW_PERSON) if parts[0] == "pack_rows" else rows, hw, 16), NAN, dtype=DTYPES[dt], device=device)
        extra = (torch.tensor(ROW_PERSON, dtype=torch.int32, device=device),) if parts[0] == "pack_rows" else ()
        return {"out": getattr(ops, parts[0])(lat, cond, out, *extra).cpu()}
    entry, arg, how = STEPS[parts[0]]
    full, lat, noise = _operands(hw, int(parts[3][3:]), dt)
    row = coef_row(G3, PHI3)
    if entry == "person_step":
        row = torch.cat([row, torch.tensor([float(a) for a in how])])
        if 0 in how:
            full = full.clone()
            full[1], full[B + 1] = NAN, NAN
    elif entry == "row_step":
        urow, crow = arg
        if parts[0] == "row_clamped":
            eps = full                                   # R = 2B: [uncond | cond], the clamped entry reads the last row
        else:                                            # (a dormant person's unconditional row is not part of the plan's eps)
            eps = plan_eps(full, [u if c >= 0 else -1 for u, c in zip(urow, crow)], crow, R=how)
        full, arg = eps, table(urow, crow, device)
    elif arg == 1:
        full = full[B:]                                  # rows [0, B) are the conditional branch
    x = lat.to(device).clone()
    work = work_pattern(ops.guided_step_work_floats(B, hw)).to(device)
    getattr(ops, entry)(full.contiguous().to(device), x, noise.to(device) if parts[4] == "noise" else None, row.to(device), work, arg)
    return {"latents": x.cpu(), "work": work.cpu()}


def digests(tensors):
    return {what: hashlib.sha256(t.contiguous().view(torch.uint8).numpy().tobytes()).hexdigest() for what, t in tensors.items()}
