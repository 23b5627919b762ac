"""Per-person strength measurement (engine set-up imported from bench.py, not copied): cached graph + overlap calls at 768x1024, 30 DDIM
steps, B = 2, bf16, on a device-resident GarmentCache of the two garments made at strength 1.  Four arms in ONE process, interleaved, ROUNDS
rounds of CALLS timed calls after one discarded warm-up call per arm (graph capture) -> one JSON line with ms per call of every arm:

    scalar        strength=1.0                                 the plain state, idmvton_cfg_step: the parent's path
    person_full   strength=[1.0, 1.0]                          the person state with nobody dormant: idmvton_person_step per step
    person_mixed  strength=[1.0, 0.5]                          person 1 dormant for 15 of the 30 steps (its TryonNet rows run all the same)
    split         two B = 1 calls, strength 1.0 and 0.5        what a service does without the feature: 30 + 15 steps at half the rows

    python tools/gpu_strength.py                      the four arms
    python tools/gpu_strength.py --arms scalar        a subset (--root DIR: import bench and the package from another checkout of the
                                                      project -- the parent commit's tree with its own built library --, to measure the
                                                      scalar arm there in the same job; same code path, so the difference is the noise)
    python tools/gpu_strength.py --trace              one serial eager call of scalar, person_full and person_mixed after a warm-up each, for
                                                      a `rocprofv3 --kernel-trace --stats -- python tools/gpu_strength.py --trace` run: the
                                                      step's own time is the cfg_step_kernel / person_stats_kernel / person_apply_kernel rows
"""
import argparse
import json
import os
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--arms", nargs="+", default=None)
ap.add_argument("--root", default=None)
ap.add_argument("--trace", action="store_true")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--calls", type=int, default=2)
args = ap.parse_args()

ROOT = os.path.abspath(args.root) if args.root else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

DEV, DT = torch.device("cuda", 0), torch.bfloat16
H, W, STEPS, B = 1024, 768, 30, 2
ARMS = dict(scalar=[dict(strength=1.0)], person_full=[dict(strength=[1.0, 1.0])], person_mixed=[dict(strength=[1.0, 0.5])],
            split=[dict(strength=1.0, person=0), dict(strength=0.5, person=1)])
names = args.arms or (["scalar", "person_full", "person_mixed"] if args.trace else list(ARMS))

eng, _ = bench.build_engine(DT, DEV, 0, STEPS)
inp = bench.synth_inputs(B, H, W, STEPS, DEV, first_image_index=0)
inp["noise"]["image"] = torch.randn(B, 4, H // 8, W // 8, generator=torch.Generator().manual_seed(77)).to(DEV)
cache = eng.encode_garment(num_inference_steps=STEPS, scheduler="ddim", cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"],
                           noise_cloth=inp["noise"]["cloth"], height=H, width=W)
form = dict() if args.trace else dict(use_graph=True, overlap=True)
common = dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler="ddim", return_latents=True, **form)


def one_person(i):
    """The inputs of person i alone: the conditional / unconditional image states are [uncond B | cond B] rows."""
    cut = lambda v: torch.cat([v[i:i + 1], v[B + i:B + i + 1]]) if v.shape[0] == 2 * B else v[i:i + 1]
    one = {k: cut(v) for k, v in inp.items() if torch.is_tensor(v)}
    one["noise"] = {k: (v[i:i + 1] if torch.is_tensor(v) else v) for k, v in inp["noise"].items() if k != "steps"}
    return {**one, "cloth": cache.select([i]), "text_embeds_cloth": None}


whole = {**inp, "cloth": cache, "text_embeds_cloth": None}
people = [one_person(i) for i in range(B)]


def call(arm, timing=None):
    """The calls of one arm -> their latents, one row per person."""
    outs = []
    for part in ARMS[arm]:
        part = dict(part)
        kw = people[part.pop("person")] if "person" in part else whole
        outs.append(eng(timing=timing, **common, **kw, **part).clone())
    return torch.cat(outs) if len(outs) > 1 else outs[0]


outs = {a: call(a) for a in names}                                     # warm-up: graph capture, discarded
torch.cuda.synchronize()
if args.trace:
    for a in names:
        call(a)
    torch.cuda.synchronize()
    print(json.dumps(dict(traced=names, form="serial eager", calls_per_arm=2, steps=STEPS)))
    sys.exit(0)
rows = {a: [] for a in names}
for r in range(args.rounds):
    for a in names:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call(a)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rows[a].append(round(dt / args.calls * 1e3, 1))
        print(f"round {r} {a:12s} {dt / args.calls * 1e3:.1f} ms/call", flush=True)
rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
res = dict(shape=f"{W}x{H}, {STEPS} DDIM steps, B={B}, bf16, graph + overlap, device-resident cache", root=ROOT,
           arms={a: dict(ms_per_call=v) for a, v in rows.items()},
           finite=bool(all(torch.isfinite(o).all() for o in outs.values())), graph_states=len(eng._graphs),
           person_steps=eng.stats["person_steps"])
if "person_full" in outs and "scalar" in outs:
    res["person_full_equals_scalar"] = bool(torch.equal(outs["person_full"], outs["scalar"]))
if "person_mixed" in outs and "scalar" in outs:
    res["person_mixed_row0_equals_scalar"] = bool(torch.equal(outs["person_mixed"][0], outs["scalar"][0]))
if "person_mixed" in outs and "split" in outs:
    res["person_mixed_vs_split_latents_relerr"] = rel(outs["person_mixed"], outs["split"])
print(json.dumps(res))
