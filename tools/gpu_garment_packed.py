"""Packed garment cache measurements at the configs[1] shape (768x1024, 30 steps, B = 2), engine set-up imported from bench.py.

  (default)       the driver: runs the three steps below one after another, each as a fresh child process under a time limit of its own, and
                  stops at the first one that fails or runs out of time (it opens no GPU itself); every step prints one JSON line
  --step fill     one 6-timestep block fill on SYNTHETIC cache contents (no weights): the 16-bit _fill_set (one copy_ per tensor, as before
                  packed storage) against the packed fill (one idmvton_kv_unpack launch), microseconds and bytes moved per second
  --step call     cached graph + overlap call on a 16-bit cache and on a packed one (--dtype, default bf16): three timed repeats each,
                  interleaved, images/s; the latents error of the packed call against the 16-bit-cached call, max|d| / max|ref|; peak device
                  memory of encode_garment(storage="e4m3") beyond what was allocated before it
  --step error    the latents error alone (--dtype f16: the second storage dtype)
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = torch.device("cuda", 0)
H, W, STEPS, B = 1024, 768, 30, 2
# (features, token rows, channels) of the two attention levels of the SDXL topology at a 128 x 96 latent (garment_cache.py, "Size")
LEVELS = ((10, 3072, 640), (60, 768, 1280))
STEP_LIMITS = (("fill", [], 240), ("call", ["--dtype", "bf16"], 420), ("error", ["--dtype", "f16"], 300))


def timed_us(fn, n=5):
    fn()
    out = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        fn()
        e1.record(); e1.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return out


def fill_step(args):
    from idm_vton_amd.garment_cache import GarmentCache
    from idm_vton_amd.pipeline import TryonEngine
    dt = torch.bfloat16
    eng = TryonEngine(None, None, None, None, dt, DEV)       # the fills need no network: sets, a cache and a block schedule
    G, n, k = B, STEPS, eng.garment_steps
    gen = torch.Generator(device=DEV).manual_seed(0)
    kv = []
    for feats, N, C in LEVELS:
        for _ in range(feats):
            kv.append((torch.randn(n * G * N, C, generator=gen, device=DEV, dtype=dt), torch.randn(n * G, C, N, generator=gen, device=DEV, dtype=dt)))
    cache = GarmentCache(G=G, timesteps=list(range(n, 0, -1)), h=H // 8, w=W // 8, dtype=dt, attn_fp8=False, f8_exp=(0, 0, 0), weights_id="synthetic", kv=kv)
    packed = cache.pack()
    _, blocks = eng._block_schedule(n)
    bi = next(i for i, (_, c) in enumerate(blocks) if c == k)                  # a steady-state block: 6 timesteps
    st = dict(gcache=cache, gidx=list(range(n)), gindex=None, k=k, B=B, blocks=blocks)
    slots, shapes = eng._cache_set_shapes(st)
    fset = eng._alloc_set((), shapes, n, k, slots)
    t16 = timed_us(lambda: eng._fill_set(st, fset, *blocks[bi]))
    want = [(a.clone(), b.clone()) for a, b in fset["kv"][:2]]
    stp = dict(st, gcache=packed)
    t0 = time.perf_counter()
    fill = eng._cached_fill(stp, [fset])
    torch.cuda.synchronize()
    table_ms = (time.perf_counter() - t0) * 1e3
    tp = timed_us(lambda: fill(bi, 0))
    # the packed fill wrote x' = e4m3(x): max|x' - x| / max|x| over the first two features (the format's bound is 2^-4)
    worst = max(float((a.float() - c.float()).abs().max() / c.float().abs().max()) for (a, b), (c, d) in zip(fset["kv"][:2], want))
    elems = sum(a.numel() + b.numel() for a, b in fset["kv"])
    med = lambda v: sorted(v)[len(v) // 2]
    print(json.dumps(dict(step="fill", shape=f"{W}x{H}, {n} steps, G={G}, block of {k} timesteps, bf16, synthetic", elements=elems,
                          fill16_us=[round(x, 1) for x in t16], packed_us=[round(x, 1) for x in tp],
                          fill16_launches=2 * len(kv), packed_launches=1, fill16_GBps=round(elems * 4 / med(t16) / 1e3, 1),
                          packed_GBps=round(elems * 3 / med(tp) / 1e3, 1), table_build_upload_ms=round(table_ms, 2), table_records=len(st["gidx"]) * G * len(kv) * 2,
                          packed_vs_16bit_max_rel=round(worst, 4), cache_nbytes=cache.nbytes, packed_nbytes=packed.nbytes)))


def call_step(args, timing):
    import bench
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float16
    eng, _ = bench.build_engine(dt, DEV, 0, STEPS)
    inp = bench.synth_inputs(B, H, W, STEPS, DEV, first_image_index=0)
    garm = dict(cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"], noise_cloth=inp["noise"]["cloth"], height=H, width=W,
                num_inference_steps=STEPS, scheduler="ddim")
    kw = dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler="ddim", use_graph=True, overlap=True)
    native = eng.encode_garment(**garm)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    packed = eng.encode_garment(storage="e4m3", **garm)
    torch.cuda.synchronize()
    enc_ms = (time.perf_counter() - t0) * 1e3
    peak = torch.cuda.max_memory_allocated() - base
    arms = {"cached16": {**inp, "cloth": native, "text_embeds_cloth": None}, "packed": {**inp, "cloth": packed, "text_embeds_cloth": None}}
    lat = {a: eng(return_latents=True, **kw, **ai).clone() for a, ai in arms.items()}        # warm-up: graph capture; and the latents
    torch.cuda.synchronize()
    res = dict(step="call" if timing else "error", shape=f"{W}x{H}, {STEPS} steps, B={B}, {args.dtype}, graph + overlap",
               latents_err_packed_vs_cached16=float((lat["packed"] - lat["cached16"]).abs().max() / lat["cached16"].abs().max()),
               cache_nbytes=native.nbytes, packed_nbytes=packed.nbytes, encode_e4m3_ms=round(enc_ms, 1), encode_e4m3_peak_bytes_beyond_baseline=peak,
               baseline_bytes_weights_and_native_cache=base)
    if timing:
        rows = {a: [] for a in arms}
        for r in range(3):                                # arms interleaved
            for a, ai in arms.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    eng(**kw, **ai)
                torch.cuda.synchronize()
                rows[a].append(B * args.calls / (time.perf_counter() - t0))
                print(f"repeat {r} {a:9s} {rows[a][-1]:.4f} images/s", flush=True)
        mean = lambda v: sum(v) / len(v)
        spread = max(rows["cached16"]) - min(rows["cached16"])
        res.update(images_per_s={a: [round(x, 4) for x in v] for a, v in rows.items()}, cached16_spread=round(spread, 4),
                   packed_minus_cached16_mean=round(mean(rows["packed"]) - mean(rows["cached16"]), 4),
                   packed_within_spread=mean(rows["packed"]) >= mean(rows["cached16"]) - spread)
    print(json.dumps(res))


def drive(args):
    for name, extra, limit in STEP_LIMITS:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--calls", str(args.calls)] + extra
        print(f"--- step {name} (limit {limit} s)", flush=True)
        try:
            rc = subprocess.run(cmd, timeout=limit).returncode
        except subprocess.TimeoutExpired:
            print(f"step {name} ran out of its {limit} s: stopping here", flush=True)
            return 124
        if rc != 0:
            print(f"step {name} ended with status {rc}: stopping here", flush=True)
            return rc
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["fill", "call", "error"], default=None)
    ap.add_argument("--dtype", choices=["bf16", "f16"], default="bf16")
    ap.add_argument("--calls", type=int, default=2, help="timed calls per repeat")
    a = ap.parse_args()
    if a.step is None:
        sys.exit(drive(a))
    torch.cuda.set_device(0)
    with torch.no_grad():
        fill_step(a) if a.step == "fill" else call_step(a, timing=a.step == "call")
