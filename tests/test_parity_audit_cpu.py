"""CPU only: can the model-level bars of tests/parity_checks.py hear a wiring defect?

tests/test_parity_gpu.py holds the engine to the fp32 oracle at `parity_checks.TOL`.  That only proves something if a defective engine would
leave those bars.  Here each defect of tests/parity_mutants.py is applied to the ORACLE and the mutated oracle is compared with the clean one,
quantity by quantity, exactly as `parity_checks.run` compares the engine with the oracle (`parity_checks.reference` is that oracle half).

A. Audibility.  On the "loud" weights every mutant moves at least one compared quantity by >= 3 x its bar.  Why 3: an engine that carries the
   defect and is otherwise within one bar of the (mutated) arithmetic misses the clean oracle by at least 3 bar - bar = 2 bar, i.e. it fails
   with a full bar of margin.  The factor is this derivation, not a measurement.
B. Reachability.  The oracle with every layer output rounded to the storage type (`storage_rounded`) stays within the bars on the same weights,
   so the bars do not ask a correct 16-bit engine for more than 16-bit storage allows.
C. A record.  On the "quiet" weights (config.random_state_dict as committed) three of the mutants stay below the fp16 latents bar: that is why
   the loud set exists, and it shows this audit can fail.
"""
import functools

import pytest
import torch

from tests import parity_checks as pc
from tests import parity_mutants as pm
from tests import parity_utils as pu

B, STEPS, FACTOR = 2, 3, 3.0
QUANTITIES = tuple(pc.BAR_OF)
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
# {mutant: reason}: the only mutants that may stay below 3 bars at the bf16 bars (at most two; none at the fp16 bars).  Empty: at time gain 1
# `timestep_stale` needed this (GarmentNet exports LayerNorm outputs, which depend on t only through the resnets' additive time term: 4e-2 on
# the latents); LOUD_GAIN["time"] = 2 makes it audible on `image` in bf16 as well.
BF16_EXEMPT = {}
# `storage_rounded` is applied to the two UNets: the loud weights change nothing in the VAE, whose engine runs at split (fp32-equivalent)
# precision and is held to its own bars on the quiet set already
ROUNDED = ("resampler", "garment_feats", "tryon_eps", "step_latents", "image")


def deviation(x, ref, q=None):
    """relerr of one compared quantity as the GPU tests assert it: the garment features by their worst element (`garment_feat_max`), the step
    latents by the last (`latents_final`)."""
    if q == "step_latents":
        assert len(x) == len(ref)
        return pu.relerr(x[-1], ref[-1])
    if isinstance(ref, (list, tuple)):
        assert len(x) == len(ref)
        return max(pu.relerr(a, b) for a, b in zip(x, ref))
    return pu.relerr(x, ref)


@functools.lru_cache(maxsize=None)
def model(kind, weights, dtype):
    return pu.build(kind, dtype, "cpu", weights=weights)


@functools.lru_cache(maxsize=None)
def clean(kind, weights, dtype, H, W):
    m = model(kind, weights, dtype)
    inp = pu.make_inputs(B, H, W, m["xd"], m["pooled"], m["enc_dim"], STEPS, dtype)
    return m, inp, pc.reference(m, inp, B, H, W, STEPS)


@functools.lru_cache(maxsize=None)
def audit(kind, weights, names, H=128, W=128):
    """{mutant: {quantity: relerr(mutated, clean)}}: one reference() call per mutant.  The weights are the fp16-rounded ones; the size of a
    wiring defect does not depend on the last bits of the weights, so one table is judged against both dtypes' bars."""
    m, inp, ref = clean(kind, weights, torch.float16, H, W)
    out = {}
    for name in names:
        with {**pm.MUTANTS, **pm.SIZE_MUTANTS}[name](m["oracle"], inp):
            mut = pc.reference(m, inp, B, H, W, STEPS)
        out[name] = {q: deviation(mut[q], ref[q], q) for q in QUANTITIES}
    return out


def audible(row, dtype):
    return [q for q in QUANTITIES if row[q] >= FACTOR * pc.TOL[dtype][pc.BAR_OF[q]]]


def show(table, dtype):
    head = "%-26s" % "3 x bar" + "".join("%14.1e" % (FACTOR * pc.TOL[dtype][pc.BAR_OF[q]]) for q in QUANTITIES)
    lines = ["%-26s" % "" + "".join("%14s" % q for q in QUANTITIES), head]
    for name, row in table.items():
        lines.append("%-26s" % name + "".join("%13.1e%s" % (row[q], "*" if q in audible(row, dtype) else " ") for q in QUANTITIES))
    return "\n" + "\n".join(lines)


ALL = tuple(pm.MUTANTS)


@pytest.mark.parametrize("kind", ["tiny", "mid"])
def test_every_mutant_is_audible_on_the_loud_weights(kind):
    """Condition A at 128x128."""
    table = audit(kind, "loud", ALL)
    print(show(table, torch.float16))
    for tag, dtype in DTYPES.items():
        deaf = [n for n in ALL if not audible(table[n], dtype)]
        allowed = set(BF16_EXEMPT) if dtype == torch.bfloat16 else set()
        assert len(BF16_EXEMPT) <= 2
        assert set(deaf) <= allowed, "%s bars cannot hear %s on (%s, loud)%s" % (tag, sorted(set(deaf) - allowed), kind, show(table, dtype))


@pytest.mark.parametrize("kind", ["tiny", "mid"])
def test_unmasked_filler_keys_are_audible_at_320x320(kind):
    """Condition A for the size whose coarsest level has 100 tokens (not a multiple of 16): the defect test_sizes_the_reference_accepts_match_
    the_oracle[320x320] exists to catch must leave its bars -- in the catalogue's form (every attention) and in the narrow form that exists
    only at such a size (the self-attentions' filler rows alone).  The loud GPU case at that size runs fp16; the bf16 bars are audited too."""
    names = ("unmasked_pad_keys", "unmasked_self_filler")
    table = audit(kind, "loud", names, 320, 320)
    print(show(table, torch.float16))
    for tag, dtype in DTYPES.items():
        for n in names:
            assert audible(table[n], dtype), "%s bars cannot hear %s on (%s, loud)%s" % (tag, n, kind, show(table, dtype))


@pytest.mark.parametrize("tag", list(DTYPES))
@pytest.mark.parametrize("kind", ["tiny", "mid"])
def test_the_bars_are_reachable_with_16_bit_storage(kind, tag):
    """Condition B: the oracle with 16-bit storage between layers stays within every bar on the loud weights."""
    dtype = DTYPES[tag]
    m, inp, ref = clean(kind, "loud", dtype, 128, 128)
    with pm.storage_rounded(m["oracle"][:2], dtype):
        rnd = pc.reference(m, inp, B, 128, 128, STEPS)
    err = {q: deviation(rnd[q], ref[q], q) for q in ROUNDED}
    print(kind, tag, err)
    over = {q: e for q, e in err.items() if not e <= pc.TOL[dtype][pc.BAR_OF[q]]}
    assert not over, (kind, tag, err)
    assert all(e > 0 for e in err.values()), err                 # the hooks were in place


def test_mutants_restore_the_oracle():
    """After every `with`, the oracle computes what it computed before (the audit reuses one model for all mutants)."""
    m, inp, ref = clean("tiny", "loud", torch.float16, 128, 128)
    audit("tiny", "loud", ALL)
    again = pc.reference(m, inp, B, 128, 128, STEPS)
    assert all(deviation(again[q], ref[q]) == 0.0 for q in QUANTITIES)
    from idm_vton_amd import ops
    assert torch.equal(ops.key_order_index(32)[ops.key_order_index(32)], torch.arange(32))       # what v_key_order_only applies


def test_record_the_quiet_weights_cannot_hear_these_mutants():
    """DOCUMENTATION of the quiet set, not a requirement on it (condition C).  With N(0, 0.02) on every matrix the softmaxes are near uniform
    and each attention branch is a few percent of the residual stream: a V^T in the wrong key order, a softmax scale off by log2(e) and a
    GarmentNet that never sees its caption all move the final latents by less than the fp16 latents bar (5e-3: 8.9e-4, 4.1e-4, 5.7e-4), the
    TryonNet noise prediction by less than the stage bar (4e-3: 1.3e-3, 8.2e-4, 7.1e-4) and the image by less than its bar (1e-2), so every
    quantity downstream of TryonNet is deaf to them in both dtypes.  Only GarmentNet's own exported features (LayerNorm outputs) move more
    (1.3e-2, 6.2e-3, 4.1e-2), which says nothing about the same defect in TryonNet's attentions.  The loud set exists for this reason; the
    same audit that passes above fails here."""
    names = ("v_key_order_only", "log2e_scale", "cloth_text_ignored")
    table = audit("tiny", "quiet", names)
    t = pc.TOL[torch.float16]
    for n in names:
        assert table[n]["step_latents"] < t["latents"], show(table, torch.float16)
        assert table[n]["tryon_eps"] < t["stage"] and table[n]["image"] < t["image"], show(table, torch.float16)
        assert not {"tryon_eps", "step_latents", "image"} & set(audible(table[n], torch.float16))
