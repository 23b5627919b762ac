"""Mixed garment sizes measurement (engine set-up imported from bench.py, not copied): one cached graph-form call at 768x1024, 30 DDIM steps,
bf16, P = 2 persons on a slotted cache of two full-size slots -- `mixed`: a 768x1024 and a 384x512 garment, `both_full`: two 768x1024
garments -- arms interleaved, three rounds of two timed calls after one discarded warm-up call per arm -> one JSON line.
    python tools/gpu_garment_ragged.py"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

DEV, DT = torch.device("cuda", 0), torch.bfloat16
H, W, STEPS, B = 1024, 768, 30, 2
ROUNDS, CALLS = 3, 2

eng, _ = bench.build_engine(DT, DEV, 0, STEPS)
inp = bench.synth_inputs(B, H, W, STEPS, DEV, first_image_index=0)
kw = dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler="ddim", use_graph=True, overlap=True)
enc = lambda cloth, nz, j: eng.encode_garment(num_inference_steps=STEPS, scheduler="ddim", cloth=cloth, text_embeds_cloth=inp["text_embeds_cloth"][j:j + 1],
                                              noise_cloth=nz, height=H, width=W)
full = [enc(inp["cloth"][j:j + 1], inp["noise"]["cloth"][j:j + 1], j) for j in range(2)]
half = enc(torch.nn.functional.interpolate(inp["cloth"][1:2].float(), size=(H // 2, W // 2), mode="bilinear"), inp["noise"]["cloth"][1:2, :, :H // 16, :W // 16], 1)
pools = {}
for name, ones in (("both_full", full), ("mixed", [full[0], half])):
    pools[name] = eng.empty_garment_cache(2, H, W, STEPS, scheduler="ddim")
    for s, one in enumerate(ones):
        pools[name].put(s, one)
arms = {a: {**inp, "cloth": p, "text_embeds_cloth": None, "garment_index": [0, 1]} for a, p in pools.items()}
outs = {a: eng(**kw, **ai).clone() for a, ai in arms.items()}          # warm-up: graph capture (one state for both arms), discarded
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
        rows[a].append((round(dt / CALLS * 1e3, 1), round(loop, 3)))
        print(f"round {r} {a:10s} {dt / CALLS * 1e3:.1f} ms/call  loop {loop:.3f} ms/step", flush=True)
res = dict(shape=f"{W}x{H}, {STEPS} steps, P={B}, slots of {W}x{H}, bf16, graph + overlap", sizes={a: p.sizes for a, p in pools.items()},
           garment_nbytes=dict(full=full[0].nbytes, half=half.nbytes),
           arms={a: dict(ms_per_call=[x[0] for x in v], loop_ms_per_step=[x[1] for x in v]) for a, v in rows.items()},
           finite=bool(all(torch.isfinite(o).all() for o in outs.values())), graph_states=len(eng._graphs), stats=eng.stats)
print(json.dumps(res))
