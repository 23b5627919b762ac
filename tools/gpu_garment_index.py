"""Garment index measurement (engine set-up imported from bench.py, not copied): one cached graph-form call at 768x1024, 30 DDIM steps, bf16,
P = 4 persons on a G = 4 cache, without an index, with garment_index=[0,1,2,3] (the same assignment through the gather form of _fill_set and
the table) and with [3,1,2,0]; arms interleaved, three rounds of two timed calls after one discarded warm-up call per arm -> one JSON line.
    python tools/gpu_garment_index.py"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

DEV, DT = torch.device("cuda", 0), torch.bfloat16
H, W, STEPS, B = 1024, 768, 30, 4
ROUNDS, CALLS = 3, 2

eng, _ = bench.build_engine(DT, DEV, 0, STEPS)
inp = bench.synth_inputs(B, H, W, STEPS, DEV, first_image_index=0)
kw = dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler="ddim", use_graph=True, overlap=True)
cache = eng.encode_garment(num_inference_steps=STEPS, scheduler="ddim", cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"],
                           noise_cloth=inp["noise"]["cloth"], height=H, width=W)
base = {**inp, "cloth": cache, "text_embeds_cloth": None}
arms = {"plain": base, "indexed_0123": {**base, "garment_index": [0, 1, 2, 3]}, "indexed_3120": {**base, "garment_index": [3, 1, 2, 0]}}
outs = {a: eng(**kw, **ai).clone() for a, ai in arms.items()}          # warm-up: graph capture, discarded
torch.cuda.synchronize()
rows = {a: [] for a in arms}
for r in range(ROUNDS):
    for a, ai in arms.items():
        timing = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            eng(timing=timing, **kw, **ai)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        loop = sum(t[1].elapsed_time(t[2]) for t in timing) / len(timing) / STEPS
        prep = sum(t[0].elapsed_time(t[1]) for t in timing) / len(timing)
        rows[a].append((round(B * CALLS / dt, 4), round(loop, 3), round(prep, 1)))
        print(f"round {r} {a:14s} {B * CALLS / dt:.4f} images/s  loop {loop:.3f} ms/step  prepare {prep:.1f} ms", flush=True)
res = dict(shape=f"{W}x{H}, {STEPS} steps, P={B} on G=4, bf16, graph + overlap", cache_nbytes=cache.nbytes,
           arms={a: dict(images_per_s=[x[0] for x in v], loop_ms_per_step=[x[1] for x in v], prepare_ms=[x[2] for x in v]) for a, v in rows.items()},
           indexed_0123_equals_plain=bool(torch.equal(outs["plain"], outs["indexed_0123"])),
           indexed_3120_differs=bool(not torch.equal(outs["plain"], outs["indexed_3120"])), stats=eng.stats)
print(json.dumps(res))
