"""Feature-shelf measurement at the configs[1] shape (768x1024, 30 steps, B = 2, bf16, graph + overlap, ddim) with two 384x512 garments in
slots of 768x1024: one process, seven arms of the same call, alternated --

  feat16_kernel / feat16_copy   GarmentShelf(storage="features"):      compact 16-bit feature parts, idmvton_kv_fill / copies + idmvton_kv_place
  feat8_kernel  / feat8_copy    GarmentShelf(storage="features-e4m3"): compact packed feature parts, the two transports
  kv8_kernel    / kv8_copy      GarmentShelf(storage="e4m3"):          compact packed K / V^T parts, the two transports
  slotted_device                the K / V^T garments in a device-resident slotted cache (ShelvedGarmentCache.slotted("cuda"))

One warm-up call per arm (graph capture; its latents are kept and compared), then --repeats rounds of --calls timed calls per arm, arms
interleaved; then one instrumented call per arm with events around every block's garment side (what drive_blocks' garment(bi, p) does: the
fill, and on a feature shelf the projection at SLOT size behind it).  Prints one JSON line: per arm ms per call (mean, min .. max over the
rounds), images/s, bytes over the host link per call (the compact parts' tensor bytes: every cache entry crosses once), host bytes per
garment, the garment-side time of a steady 6-timestep block, and what the slot-size projection costs: each feature arm minus the K / V^T
arm of the same transport.  Exit status 1 unless the two transports of every shelf give the same latents and the 16-bit feature shelf's
latents are finite; whether they EQUAL the call on engine.project_garment(<the feature shelf>) is reported (a GEMM row not depending on M is
measured, not implied).  No timing bar: nothing here was measured before.  Engine set-up from bench.py."""
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
GH, GW = 512, 384                                        # the garments' own size


def main(args):
    import bench
    from idm_vton_amd import pipeline
    from idm_vton_amd.garment_cache import GarmentShelf
    dt = torch.bfloat16
    eng, _ = bench.build_engine(dt, DEV, 0, STEPS)
    inp = bench.synth_inputs(B, H, W, STEPS, DEV, first_image_index=0)
    g = torch.Generator(device="cpu").manual_seed(4242)
    cloths = [torch.randn(1, 3, GH, GW, generator=g).clamp(-1, 1).to(DEV) for _ in range(B)]
    noises = [torch.randn(1, 4, GH // 8, GW // 8, generator=g).to(DEV) for _ in range(B)]
    kw = dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler="ddim", use_graph=True, overlap=True)
    enc = lambda j, storage: eng.encode_garment(cloth=cloths[j], text_embeds_cloth=inp["text_embeds_cloth"][j:j + 1], noise_cloth=noises[j],
                                                height=H, width=W, num_inference_steps=STEPS, scheduler="ddim", storage=storage)
    like = eng.empty_garment_cache(1, H, W, STEPS, scheduler="ddim", height=H, width=W)
    keys = [f"sku{j}" for j in range(B)]
    shelves, pin_s = {}, {}
    for name, storage in (("feat16", "features"), ("feat8", "features-e4m3"), ("kv8", "e4m3")):
        shelf = GarmentShelf(like, storage=storage)
        t0 = time.perf_counter()
        for j, key in enumerate(keys):
            shelf.add(key, enc(j, storage))              # (one garment on the device at a time)
        pin_s[name] = round(time.perf_counter() - t0, 2)
        shelves[name] = shelf.get(keys)
        torch.cuda.empty_cache()
    del like                                             # (only its fields and shapes were kept)
    torch.cuda.empty_cache()
    index = shelves["kv8"][1]
    assert all(ix == index for _, ix in shelves.values())
    caches = {name: c for name, (c, _) in shelves.items()}
    assert caches["feat16"].features and caches["feat8"].features and caches["feat8"].packed and not caches["kv8"].features
    tensor_bytes = lambda c: sum(t.numel() * t.element_size() for p in c.parts for e in p.kv for t in e)
    arms = {f"{name}_{tr}": (caches[name], tr) for name in ("feat16", "feat8", "kv8") for tr in ("kernel", "copy")}
    arms["slotted_device"] = (caches["kv8"].slotted(DEV), "kernel")

    def call(a, cache=None, **more):
        c, transport = arms[a] if cache is None else (cache, a)
        return eng(**kw, **more, host_transport=transport, **{**inp, "cloth": c, "garment_index": index, "text_embeds_cloth": None})
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
            print(f"round {r} {a:15s} {rows[a][-1]:9.2f} ms per call", flush=True)
    blocks, drive = {}, pipeline.drive_blocks
    for a in arms:                                                       # one instrumented call per arm
        log = []

        def timed(fn, log=log):
            def run(bi, p):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(bi, p)
                e1.record()
                log.append((bi, e0, e1))
                return out
            return run
        pipeline.drive_blocks = lambda bl, garment, tryon, *rest: drive(bl, timed(garment), tryon, *rest)
        try:
            call(a, return_latents=True)
        finally:
            pipeline.drive_blocks = drive
        torch.cuda.synchronize()
        blocks[a] = [round(e0.elapsed_time(e1), 3) for _, e0, e1 in sorted(log, key=lambda x: x[0])]
    _, sched = eng._block_schedule(STEPS)
    steady = [bi for bi, (_, c) in enumerate(sched) if c == eng.garment_steps]
    med = lambda v: sorted(v)[len(v) // 2]
    mean = lambda v: sum(v) / len(v)
    res = {}
    for a, v in rows.items():
        c = arms[a][0]
        shelved = a != "slotted_device"
        res[a] = dict(ms_per_call=round(mean(v), 2), ms_min=round(min(v), 2), ms_max=round(max(v), 2), images_per_s=round(1e3 * B / mean(v), 4),
                      link_bytes_per_call=tensor_bytes(c) if shelved else 0, host_bytes_per_garment=[p.nbytes for p in c.parts] if shelved else 0,
                      cache_nbytes=c.nbytes, steady_block_garment_side_ms=round(med([blocks[a][bi] for bi in steady]), 3),
                      garment_side_ms_per_block=blocks[a])
    # the comparison anchor: the K / V^T shelf engine.project_garment makes of the 16-bit feature shelf, one call
    proj = eng.project_garment(caches["feat16"])
    lat_proj = call("kernel", cache=proj, return_latents=True).clone()
    diff = (lat["feat16_kernel"] - lat_proj).abs().max().item()
    same = {name: bool(torch.equal(lat[f"{name}_kernel"], lat[f"{name}_copy"])) for name in ("feat16", "feat8", "kv8")}
    finite = bool(torch.isfinite(lat["feat16_kernel"]).all() and torch.isfinite(lat["feat8_kernel"]).all())
    out = dict(shape=f"{W}x{H}, {STEPS} steps, B={B}, two {GW}x{GH} garments in {W}x{H} slots, bf16, graph + overlap, ddim", calls_per_round=args.calls,
               rounds=args.repeats, block_timesteps=[c for _, c in sched], encode_pack_and_pin_s=pin_s, arms=res,
               projection_at_slot_size_ms={f"{name}_{tr}_minus_kv8_{tr}": round(res[f"{name}_{tr}"]["ms_per_call"] - res[f"kv8_{tr}"]["ms_per_call"], 2)
                                           for name in ("feat16", "feat8") for tr in ("kernel", "copy")},
               minus_slotted_device_ms={a: round(res[a]["ms_per_call"] - res["slotted_device"]["ms_per_call"], 2) for a in arms if a != "slotted_device"},
               spread_ms={a: round(max(v) - min(v), 2) for a, v in rows.items()},
               transports_give_equal_latents=same, feature_latents_finite=finite,
               feat16_equals_projected_kv_shelf=bool(torch.equal(lat["feat16_kernel"], lat_proj)), feat16_minus_projected_kv_shelf_max_abs=diff,
               kv8_shelf_equals_slotted_device=bool(torch.equal(lat["kv8_kernel"], lat["slotted_device"])),
               projections=eng.stats["garment_projections"], stream_launches=eng.stats["garment_stream_launches"],
               stage_launches=eng.stats["garment_stage_launches"])
    print(json.dumps(out), flush=True)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(out, f)
    return 0 if all(same.values()) and finite else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2, help="timed calls per round and arm")
    ap.add_argument("--repeats", type=int, default=3, help="rounds")
    ap.add_argument("--json-out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with torch.no_grad():
        sys.exit(main(a))
