"""Feature-cache measurement at the configs[1] shape (768x1024, 30 steps, B = 2, bf16, graph + overlap): one process, five arms of the same
call, alternated --

  uncached        GarmentNet runs in the call
  kv              the K / V^T cache on the device (encode_garment(storage="native"))
  features        the feature cache on the device, 16-bit (storage="features")
  features_e4m3   the feature cache on the device, packed (storage="features-e4m3")
  host_copy       the packed feature cache in pinned host memory, host_transport="copy"

One warm-up call per arm (graph capture; its latents are kept and compared), then --repeats rounds of --calls timed calls per arm, arms
interleaved; then one instrumented call per arm with events around every block's garment side (GarmentNet batch + projection, cache fill,
or feature fill + projection: what drive_blocks' garment(bi, p) does) and every block's TryonNet steps.  Prints one JSON line: per arm ms per
call (mean, min .. max over the rounds), images/s, cache.nbytes, bytes over the host link per call, and the garment-side time of one steady
6-timestep block (the median over the call's 6-timestep blocks).  Exit status 1 unless the features arm's latents equal the kv arm's, the
packed arms' are equal to each other, the feature-cached loop equals the uncached loop from the same start (a cached prepare() encodes the
person side at another VAE batch size, so whole calls are not compared: start latents and conditioning are copied over, as the tests do),
and EVERY feature-cached arm is faster than the uncached arm: it does strictly less work.  The difference to the kv arm is reported beside
that arm's own spread; it has no bar.  Engine set-up from bench.py."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = torch.device("cuda", 0)
H, W, STEPS, B = 1024, 768, 30, 2


def main(args):
    import bench
    from idm_vton_amd import pipeline
    dt = torch.bfloat16
    eng, _ = bench.build_engine(dt, DEV, 0, STEPS)
    inp = bench.synth_inputs(B, H, W, STEPS, DEV, first_image_index=0)
    kw = dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler="ddim", use_graph=True, overlap=True)
    enc = lambda storage: eng.encode_garment(cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"], noise_cloth=inp["noise"]["cloth"],
                                             height=H, width=W, num_inference_steps=STEPS, scheduler="ddim", storage=storage)
    kvc, feats = enc("native"), enc("features")
    packed = enc("features-e4m3")
    t0 = time.perf_counter()
    host = packed.to("cpu", pin_memory=True)
    pin_s = time.perf_counter() - t0
    assert feats.features and packed.features and packed.packed and 2 * feats.nbytes == kvc.nbytes
    arms = {"uncached": (None, "kernel"), "kv": (kvc, "kernel"), "features": (feats, "kernel"), "features_e4m3": (packed, "kernel"),
            "host_copy": (host, "copy")}

    def call(a, **more):
        cache, transport = arms[a]
        if cache is None:
            return eng(**kw, **more, **inp)
        return eng(**kw, **more, host_transport=transport, **{**inp, "cloth": cache, "text_embeds_cloth": None})
    lat = {a: call(a, return_latents=True).clone() for a in arms}        # warm-up: graph capture; and the latents
    torch.cuda.synchronize()
    rows = {a: [] for a in arms}
    for r in range(args.repeats):                                        # arms interleaved
        for a in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call(a)
            torch.cuda.synchronize()
            rows[a].append(1e3 * (time.perf_counter() - t0) / args.calls)
            print(f"round {r} {a:14s} {rows[a][-1]:9.2f} ms per call", flush=True)
    blocks, drive = {}, pipeline.drive_blocks
    for a in arms:                                                       # one instrumented call per arm
        log = dict(garment=[], tryon=[])

        def timed(kind, fn, log=log):
            def run(bi, p):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(bi, p)
                e1.record()
                log[kind].append((bi, e0, e1))
                return out
            return run
        pipeline.drive_blocks = lambda bl, garment, tryon, *rest: drive(bl, timed("garment", garment), timed("tryon", tryon), *rest)
        try:
            call(a, return_latents=True)
        finally:
            pipeline.drive_blocks = drive
        torch.cuda.synchronize()
        blocks[a] = {kind: [round(e0.elapsed_time(e1), 3) for _, e0, e1 in sorted(v, key=lambda x: x[0])] for kind, v in log.items()}
    _, sched = eng._block_schedule(STEPS)
    steady = [bi for bi, (_, c) in enumerate(sched) if c == eng.garment_steps]
    med = lambda v: sorted(v)[len(v) // 2]
    mean = lambda v: sum(v) / len(v)
    link = {a: 0 for a in arms}
    link["host_copy"] = host.nbytes - host.exps.numel() * host.exps.element_size()      # every entry of both garments crosses once per call
    res = {a: dict(ms_per_call=round(mean(v), 2), ms_min=round(min(v), 2), ms_max=round(max(v), 2), images_per_s=round(1e3 * B / mean(v), 4),
                   cache_nbytes=0 if arms[a][0] is None else arms[a][0].nbytes, link_bytes_per_call=link[a],
                   steady_block_garment_side_ms=round(med([blocks[a]["garment"][bi] for bi in steady]), 3),
                   garment_side_ms_per_block=blocks[a]["garment"], tryon_ms_per_block=blocks[a]["tryon"]) for a, v in rows.items()}
    eq16 = bool(torch.equal(lat["features"], lat["kv"]))
    # the loops from one start: uncached against feature-cached
    pkw = dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler="ddim")
    st_u = eng.prepare(**pkw, **inp)
    st_f = eng.prepare(**pkw, **{**inp, "cloth": feats, "text_embeds_cloth": None})
    st_f["latents"].copy_(st_u["latents"])
    st_f["cond"].copy_(st_u["cond"])
    lat_u = eng.denoise(st_u, use_graph=True, overlap=True).clone()
    equ = bool(torch.equal(eng.denoise(st_f, use_graph=True, overlap=True), lat_u))
    eq8 = bool(torch.equal(lat["host_copy"], lat["features_e4m3"]))
    faster = {a: res[a]["ms_per_call"] < res["uncached"]["ms_per_call"] for a in ("features", "features_e4m3", "host_copy")}
    out = dict(shape=f"{W}x{H}, {STEPS} steps, B={B}, bf16, graph + overlap, ddim", calls_per_round=args.calls, rounds=args.repeats,
               block_timesteps=[c for _, c in sched], pin_and_copy_s=round(pin_s, 2), arms=res,
               kv_spread_ms=round(max(rows["kv"]) - min(rows["kv"]), 2), uncached_spread_ms=round(max(rows["uncached"]) - min(rows["uncached"]), 2),
               minus_kv_ms={a: round(res[a]["ms_per_call"] - res["kv"]["ms_per_call"], 2) for a in arms if a != "kv"},
               features_latents_equal_kv=eq16, host_copy_latents_equal_features_e4m3=eq8, feature_loop_equals_uncached_loop=equ, every_feature_arm_faster_than_uncached=faster,
               projections=eng.stats["garment_projections"], stage_launches=eng.stats["garment_stage_launches"])
    print(json.dumps(out), flush=True)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(out, f)
    return 0 if eq16 and eq8 and equ and all(faster.values()) else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2, help="timed calls per round and arm")
    ap.add_argument("--repeats", type=int, default=3, help="rounds")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with torch.no_grad():
        sys.exit(main(a))
