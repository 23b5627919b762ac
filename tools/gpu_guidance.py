"""Per-person guidance measurement (engine set-up imported from bench.py, not copied): cached graph + overlap calls at 768x1024, 30 DDIM
steps, B = 2, bf16, on a device-resident GarmentCache of the two garments.  Four arms in ONE process, interleaved, ROUNDS rounds of CALLS
timed calls after one discarded warm-up call per arm (graph capture) -> one JSON line with ms per call and loop ms per step of every arm:

    plain         guidance_scale=2.0                                   the [steps][4] table, idmvton_cfg_step: the parent's path
    guided        guidance_scale=[2, 2], guidance_rescale=0.7          idmvton_guided_step: statistics + apply per step
    batched_g1    guidance_scale=1.0                                   both branches, guidance 1
    skip_g1       guidance_scale=1.0, uncond="skip"                    the conditional branch alone: B TryonNet rows

    python tools/gpu_guidance.py                      the four arms
    python tools/gpu_guidance.py --arms plain         a subset (--root DIR: import bench and the package from another checkout of the
                                                      project -- the parent commit's tree with its own built library --, to measure the
                                                      plain arm there in the same job; same code path, so the difference is the noise)
    python tools/gpu_guidance.py --trace              one serial eager call of plain, guided and skip_g1 after a warm-up each, for a
                                                      `rocprofv3 --kernel-trace --stats -- python tools/gpu_guidance.py --trace` run: the
                                                      step's own time is the cfg_step_kernel / guided_stats_kernel / guided_apply_kernel rows
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
ARMS = dict(plain=dict(guidance_scale=2.0), guided=dict(guidance_scale=[2.0, 2.0], guidance_rescale=0.7),
            batched_g1=dict(guidance_scale=1.0), skip_g1=dict(guidance_scale=1.0, uncond="skip"))
names = args.arms or (["plain", "guided", "skip_g1"] if args.trace else list(ARMS))

eng, _ = bench.build_engine(DT, DEV, 0, STEPS)
inp = bench.synth_inputs(B, H, W, STEPS, DEV, first_image_index=0)
cache = eng.encode_garment(num_inference_steps=STEPS, scheduler="ddim", cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"],
                           noise_cloth=inp["noise"]["cloth"], height=H, width=W)
form = dict() if args.trace else dict(use_graph=True, overlap=True)
kw = dict(num_inference_steps=STEPS, scheduler="ddim", return_latents=True, **form, **{**inp, "cloth": cache, "text_embeds_cloth": None})
outs = {a: eng(**kw, **ARMS[a]).clone() for a in names}                 # warm-up: graph capture, discarded
torch.cuda.synchronize()
if args.trace:
    for a in names:
        eng(**kw, **ARMS[a])
    torch.cuda.synchronize()
    print(json.dumps(dict(traced=names, form="serial eager", calls_per_arm=2, steps=STEPS)))
    sys.exit(0)
rows = {a: [] for a in names}
for r in range(args.rounds):
    for a in names:
        timing = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            eng(timing=timing, **kw, **ARMS[a])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        loop = sum(t[1].elapsed_time(t[2]) for t in timing) / len(timing) / STEPS
        rows[a].append((round(dt / args.calls * 1e3, 1), round(loop, 3)))
        print(f"round {r} {a:10s} {dt / args.calls * 1e3:.1f} ms/call  loop {loop:.3f} ms/step", flush=True)
rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
res = dict(shape=f"{W}x{H}, {STEPS} DDIM steps, B={B}, bf16, graph + overlap, device-resident cache", root=ROOT,
           arms={a: dict(ms_per_call=[x[0] for x in v], loop_ms_per_step=[x[1] for x in v]) for a, v in rows.items()},
           finite=bool(all(torch.isfinite(o).all() for o in outs.values())), graph_states=len(eng._graphs))
if "skip_g1" in outs and "batched_g1" in outs:
    res["skip_vs_batched_g1_latents_relerr"] = rel(outs["skip_g1"], outs["batched_g1"])
if "guided" in outs and "plain" in outs:
    res["guided_vs_plain_latents_relerr"] = rel(outs["guided"], outs["plain"])
print(json.dumps(res))
