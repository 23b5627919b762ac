"""Row-plan measurement (engine set-up imported from bench.py, not copied): cached graph + overlap calls at 768x1024, 30 DDIM steps, B = 2,
bf16, on a device-resident GarmentCache of the two garments made at strength 1.  Five arms in ONE process, interleaved, ROUNDS rounds of
CALLS timed calls after one discarded warm-up call per arm (graph capture) -> one JSON line with ms per call of every arm:

    scalar            strength=1.0, guidance 2               the plain state: the unchanged call
    strength_all      strength=[1.0, 0.5]                    the person state: 30 steps of 4 TryonNet rows, 120 row-steps
    strength_needed   the same, rows="needed"                15 steps of 2 rows + 15 of 4: 90 row-steps
    guidance_all      guidance_scale=[2.0, 1.0]              the guided state: 4 rows per step, person 1 at guidance 1
    guidance_needed   the same, rows="needed"                3 rows per step: person 1 has no unconditional row

    python tools/gpu_rows.py                          the five arms
    python tools/gpu_rows.py --arms scalar            a subset (--root DIR: import bench and the package from another checkout of the project
                                                      -- the parent commit's tree with its own built library --, to measure the scalar arm
                                                      there in the same job; same code path, so the difference is the drift of the rounds)
    python tools/gpu_rows.py --trace                  one serial eager call of the four per-person arms after a warm-up each, for a
                                                      `rocprofv3 --kernel-trace --stats -- python tools/gpu_rows.py --trace` run: the edge
                                                      kernels' own times are the pack_rows_kernel / pack_input_kernel and the row_stats_kernel +
                                                      row_apply_kernel / person_* / guided_* rows

A job runs each of these under its own time limit and chains them with &&:

    timeout -k 10 600 python tools/gpu_rows.py && timeout -k 10 300 python tools/gpu_rows.py --arms scalar --root <parent tree> && \\
    timeout -k 10 300 rocprofv3 --kernel-trace --stats -d <out dir> -- python tools/gpu_rows.py --trace
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
ARMS = dict(scalar=dict(strength=1.0, guidance_scale=2.0),
            strength_all=dict(strength=[1.0, 0.5], guidance_scale=2.0), strength_needed=dict(strength=[1.0, 0.5], guidance_scale=2.0, rows="needed"),
            guidance_all=dict(strength=1.0, guidance_scale=[2.0, 1.0]), guidance_needed=dict(strength=1.0, guidance_scale=[2.0, 1.0], rows="needed"))
names = args.arms or [a for a in ARMS if not (args.trace and a == "scalar")]

eng, _ = bench.build_engine(DT, DEV, 0, STEPS)
inp = bench.synth_inputs(B, H, W, STEPS, DEV, first_image_index=0)
inp["noise"]["image"] = torch.randn(B, 4, H // 8, W // 8, generator=torch.Generator().manual_seed(77)).to(DEV)
cache = eng.encode_garment(num_inference_steps=STEPS, scheduler="ddim", cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"],
                           noise_cloth=inp["noise"]["cloth"], height=H, width=W)
form = dict() if args.trace else dict(use_graph=True, overlap=True)
common = dict(num_inference_steps=STEPS, scheduler="ddim", return_latents=True, **form)
whole = {**inp, "cloth": cache, "text_embeds_cloth": None}


def call(arm):
    return eng(**common, **whole, **ARMS[arm]).clone()


outs = {a: call(a) for a in names}                                     # warm-up: graph capture, discarded
torch.cuda.synchronize()
counted = {k: eng.stats[k] for k in ("tryon_rows", "row_steps")}       # of the warm-up calls: one call per arm
if args.trace:
    for a in names:
        call(a)
    torch.cuda.synchronize()
    print(json.dumps(dict(traced=names, form="serial eager", calls_per_arm=2, steps=STEPS)))
    sys.exit(0)
ms = {a: [] for a in names}
for r in range(args.rounds):
    for a in names:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            call(a)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ms[a].append(round(dt / args.calls * 1e3, 1))
        print(f"round {r} {a:16s} {dt / args.calls * 1e3:.1f} ms/call", flush=True)
rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
res = dict(shape=f"{W}x{H}, {STEPS} DDIM steps, B={B}, bf16, graph + overlap, device-resident cache", root=ROOT,
           arms={a: dict(ms_per_call=v) for a, v in ms.items()},
           finite=bool(all(torch.isfinite(o).all() for o in outs.values())), graph_states=len(eng._graphs), warmup_counters=counted)
for kind in ("strength", "guidance"):
    if kind + "_all" in outs and kind + "_needed" in outs:
        a, n = outs[kind + "_all"], outs[kind + "_needed"]
        res[kind + "_needed_equals_all"] = [bool(torch.equal(n[i], a[i])) for i in range(B)]
        res[kind + "_needed_vs_all_relerr"] = rel(n, a)
print(json.dumps(res))
