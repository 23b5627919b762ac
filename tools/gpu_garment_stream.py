"""Host-resident garment cache measurements at the configs[1] shape (768x1024, 30 steps, B = 2, bf16), on a PACKED cache only (9.44 GB of
page-locked host memory, pinned once; a 16-bit cache would pin 18.9 GB).  Engine set-up imported from bench.py.

  (default)       the driver: runs the two steps below one after another, each as a fresh child process under a time limit of its own, and
                  stops at the first one that fails or runs out of time (it opens no GPU itself); every step prints one JSON line, and the
                  link rate the first step measured is handed to the second
  --step fill     one steady 6-timestep block (G = 2: 1 887 436 800 source bytes) from SYNTHETIC cache contents in pinned host memory into a
                  16-bit set, one idmvton_kv_stream launch, on an otherwise idle GPU, for workgroups in {4, 8, 16, 32, 64, 256}: microseconds
                  and source GB/s.  The largest GB/s is the box's host-link rate; the default to ship for `workgroups`
                  (ops.KV_STREAM_WORKGROUPS) is the smallest count within 3 % of it -- the box-to-box spread DESIGN.md states.  The set is
                  compared bit for bit with the one the device-resident fill (idmvton_kv_unpack) writes.
  --step call     cached graph + overlap call on the packed cache in pinned host memory and on the device-resident one (the parent's path,
                  which this change must not move): three timed repeats each, interleaved, images/s; then one instrumented call per arm with
                  events around every block's fill and every block's TryonNet steps.  The host arm is expected within (block 0's bytes /
                  --link-gbps) per call plus the device arm's own spread; if it is not, the per-block times say whether a fill outran the
                  TryonNet block it hides behind, or TryonNet itself ran slower next to the fills.  --workgroups N ...: further host arms
                  with those `workgroups` values (the fill's rate against what it costs TryonNet).  The arm "copy" is the same host cache
                  with host_transport="copy": each block's packed bytes go into the engine's staging arena with the copy engines and one
                  idmvton_kv_place launch places them -- the same bytes over the same link, without a kernel that reads host memory.  It is
                  held to one condition: its ms per call below the host arm's by more than the device arm's own spread.
  --step fillrate idmvton_kv_fill against idmvton_kv_stream (the reference: what plain host caches use) on the SAME data-only table -- one
                  steady block of ONE packed 768x1024 garment from pinned memory, 16 workgroups --, in one process, alternating, nine timed
                  launches each after one discarded: median source GB/s of both and the run-to-run spread (min .. max); the two sets are
                  compared bit for bit.  Then, the same way, idmvton_kv_place against idmvton_kv_unpack (the reference: what device-resident
                  packed caches use) on that table with the SAME bytes in device memory: medians, spread, bit equality, and whether the
                  new launch's median lies within +3 % of the old one's or below it.  Run on its own (the driver above does not include it).
  --step shelf    the garment shelf in a call: B = 2 persons at 768x1024, 30 steps, graph + overlap, each in a 384x512 packed garment, from
                  a GarmentShelf ("shelf"), from the device-resident slotted cache the same garments give ("device"), and with the garments
                  encoded at 768x1024 in today's GarmentPool(resident="host") ("host_full"), and from the shelf again with
                  host_transport="copy" ("shelf_copy"): images/s of the four, interleaved, three repeats; the bytes a call loads over the host link and the zero-tail bytes a block writes, both summed from the descriptor
                  tables of the launches of one call.  Run on its own.
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
WORKGROUPS = (4, 8, 16, 32, 64, 256)
STEP_LIMITS = (("fill", 300), ("call", 540))
SPEC_GBPS = 63.0                                         # the link's spec rate: what --step call assumes when no measured rate is given


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
    from idm_vton_amd import ops
    from idm_vton_amd.garment_cache import PackedGarmentCache
    from idm_vton_amd.pipeline import TryonEngine
    dt = torch.bfloat16
    eng = TryonEngine(None, None, None, None, dt, DEV)       # the fills need no network: a set, a cache and one block
    G, k = B, eng.garment_steps
    gen = torch.Generator(device=DEV).manual_seed(0)

    def rand_bytes(*shape):                                  # finite e4m3 bytes (0x7f / 0xff, the NaN bytes, become 0)
        b = torch.randint(0, 256, shape, generator=gen, device=DEV, dtype=torch.uint8)
        return torch.where((b & 0x7f) == 0x7f, torch.zeros_like(b), b)
    kv = [(rand_bytes(k * G * N, C), rand_bytes(k * G, C, N)) for feats, N, C in LEVELS for _ in range(feats)]
    exps = torch.randint(-7, 16, (G, len(kv), 2), generator=gen, device=DEV, dtype=torch.int32)
    dev_cache = PackedGarmentCache(G=G, timesteps=list(range(k, 0, -1)), h=H // 8, w=W // 8, dtype=dt, attn_fp8=False, f8_exp=(0, 0, 0),
                                   weights_id="synthetic", kv=kv, exps=exps)
    t0 = time.perf_counter()
    host = dev_cache.to("cpu", pin_memory=True)
    pin_s = time.perf_counter() - t0
    st = dict(gcache=host, gidx=list(range(k)), gindex=None, k=k, B=B, blocks=[(0, k)])       # ONE block: the k timesteps of the cache
    slots, shapes = eng._cache_set_shapes(st)
    fset, ref = eng._alloc_set((), shapes, k, k, slots), eng._alloc_set((), shapes, k, k, slots)
    eng._cached_fill(dict(st, gcache=dev_cache), [ref])(0, 0)
    t0 = time.perf_counter()
    fill = eng._cached_fill(st, [fset])
    torch.cuda.synchronize()
    table_ms = (time.perf_counter() - t0) * 1e3
    src_bytes = sum(a.numel() + b.numel() for a, b in host.kv)
    rows = {}
    for wg in WORKGROUPS:
        ops.KV_STREAM_WORKGROUPS = wg
        for a, b in fset["kv"]:
            a.zero_(); b.zero_()
        us = timed_us(lambda: fill(0, 0))
        same = all(torch.equal(a, c) and torch.equal(b, d) for (a, b), (c, d) in zip(fset["kv"], ref["kv"]))
        med = sorted(us)[len(us) // 2]
        rows[wg] = dict(us=[round(x, 1) for x in us], GBps=round(src_bytes / med / 1e3, 2), bit_equal_to_device_fill=same)
        print(f"workgroups {wg:4d}: median {med:10.1f} us, {rows[wg]['GBps']:7.2f} GB/s from host memory, bit-equal {same}", flush=True)
    best = max(r["GBps"] for r in rows.values())
    default = min(wg for wg, r in rows.items() if r["GBps"] >= 0.97 * best)
    emit(args, dict(step="fill", shape=f"{W}x{H}, G={G}, one block of {k} timesteps, bf16 sets, packed synthetic cache in pinned host memory",
                          source_bytes=src_bytes, pin_and_copy_s=round(pin_s, 2), table_build_upload_ms=round(table_ms, 2), per_workgroups=rows,
                          link_GBps=best, spec_GBps=SPEC_GBPS, default_workgroups=default,
                    all_bit_equal=all(r["bit_equal_to_device_fill"] for r in rows.values())))
    return 0 if all(r["bit_equal_to_device_fill"] for r in rows.values()) else 1


def call_step(args):
    import bench
    from idm_vton_amd import ops, pipeline
    dt = torch.bfloat16
    eng, _ = bench.build_engine(dt, DEV, 0, STEPS)
    inp = bench.synth_inputs(B, H, W, STEPS, DEV, first_image_index=0)
    kw = dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler="ddim", use_graph=True, overlap=True)
    device = eng.encode_garment(cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"], noise_cloth=inp["noise"]["cloth"], height=H, width=W,
                                num_inference_steps=STEPS, scheduler="ddim", storage="e4m3")
    t0 = time.perf_counter()
    host = device.to("cpu", pin_memory=True)
    pin_s = time.perf_counter() - t0
    # arms: the device-resident cache, the host-resident one with the shipped `workgroups` ("host"), with every --workgroups value, and with
    # the copy-engine transport ("copy")
    arms = {"device": (device, None, "kernel"), "host": (host, ops.KV_STREAM_WORKGROUPS, "kernel"),
            **{f"host@{wg}": (host, wg, "kernel") for wg in args.workgroups}, "copy": (host, None, "copy")}

    def call(a, **more):
        cache, wg, transport = arms[a]
        if wg is not None:
            ops.KV_STREAM_WORKGROUPS = wg
        return eng(**kw, **more, host_transport=transport, **{**inp, "cloth": cache, "text_embeds_cloth": None})
    lat = {a: call(a, return_latents=True).clone() for a in arms}                             # warm-up: graph capture; and the latents
    torch.cuda.synchronize()
    rows = {a: [] for a in arms}
    for r in range(3):                                    # arms interleaved
        for a in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call(a)
            torch.cuda.synchronize()
            rows[a].append(B * args.calls / (time.perf_counter() - t0))
            print(f"repeat {r} {a:7s} {rows[a][-1]:.4f} images/s", flush=True)
    # one instrumented call per arm: events around every block's fill (on the stream it runs on) and every block's TryonNet steps
    blocks, drive = {}, pipeline.drive_blocks
    for a in arms:
        log = dict(fill=[], tryon=[])

        def timed(kind, fn, log=log):
            def run(bi, p):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = fn(bi, p)
                e1.record()
                log[kind].append((bi, e0, e1))
                return out
            return run
        pipeline.drive_blocks = lambda bl, garment, tryon, *rest: drive(bl, timed("fill", garment), timed("tryon", tryon), *rest)
        try:
            call(a, return_latents=True)
        finally:
            pipeline.drive_blocks = drive
        torch.cuda.synchronize()
        blocks[a] = {kind: [round(e0.elapsed_time(e1), 3) for _, e0, e1 in sorted(v, key=lambda x: x[0])] for kind, v in log.items()}
    mean = lambda v: sum(v) / len(v)
    ms = {a: [1e3 * B / x for x in v] for a, v in rows.items()}          # per call
    spread_ms = max(ms["device"]) - min(ms["device"])
    _, sched = eng._block_schedule(STEPS)
    per_step = (host.nbytes - host.exps.numel() * 4) // STEPS
    block0_ms = sched[0][1] * per_step / (args.link_gbps * 1e6)
    excess_ms = mean(ms["host"]) - mean(ms["device"])
    gain_ms = mean(ms["host"]) - mean(ms["copy"])            # the one condition on the copy arm: below the host arm by more than the device arm's spread
    within = excess_ms <= block0_ms + spread_ms
    fh, th, td = blocks["host"]["fill"], blocks["host"]["tryon"], blocks["device"]["tryon"]
    outran = [bi for bi in range(1, len(fh)) if fh[bi] > th[bi - 1]]      # block bi's fill runs behind TryonNet's block bi - 1
    slowed_ms = sum(th) - sum(td)
    verdict = ("within block 0's exposed transfer plus the device arm's spread" if within else
               ("fills outran TryonNet in blocks %s" % outran if outran else "no fill outran its TryonNet block") +
               f"; TryonNet's blocks took {slowed_ms:+.2f} ms in the host call against the device call")
    emit(args, dict(step="call", shape=f"{W}x{H}, {STEPS} steps, B={B}, bf16, graph + overlap, packed cache", pin_and_copy_s=round(pin_s, 2),
                          latents_equal=all(bool(torch.equal(lat[a], lat["device"])) for a in arms), workgroups={a: wg for a, (_, wg, _) in arms.items()},
                          tryon_ms_beside_fills={a: round(sum(v["tryon"]), 2) for a, v in blocks.items()}, fill_ms={a: round(sum(v["fill"]), 2) for a, v in blocks.items()}, images_per_s={a: [round(x, 4) for x in v] for a, v in rows.items()},
                          ms_per_call={a: round(mean(v), 2) for a, v in ms.items()}, device_spread_ms=round(spread_ms, 2),
                          host_minus_device_ms=round(excess_ms, 2), link_GBps=args.link_gbps, block0_bytes=sched[0][1] * per_step,
                          block0_exposed_ms=round(block0_ms, 2), within_expectation=within, verdict=verdict, block_timesteps=[c for _, c in sched],
                          per_block_ms=blocks, serial_form_exposed_ms=round(sum(fh), 2),
                          copy_minus_device_ms=round(mean(ms["copy"]) - mean(ms["device"]), 2), host_minus_copy_ms=round(gain_ms, 2),
                          copy_below_host_by_more_than_device_spread=gain_ms > spread_ms,
                          stage_launches=eng.stats["garment_stage_launches"], stage_copies=eng.stats["garment_stage_copies"],
                          arena_bytes=[a.numel() for a, _ in eng._arenas.values()],
                    stream_launches=eng.stats["garment_stream_launches"], cache_nbytes=host.nbytes))
    return 0 if all(torch.equal(lat[a], lat["device"]) for a in arms) else 1


def fillrate_step(args):
    from idm_vton_amd import ffi, ops
    from idm_vton_amd.garment_cache import PackedGarmentCache, fill_records
    from idm_vton_amd.pipeline import TryonEngine
    dt = torch.bfloat16
    eng = TryonEngine(None, None, None, None, dt, DEV)
    G, k = 1, eng.garment_steps
    gen = torch.Generator(device=DEV).manual_seed(0)

    def rand_bytes(*shape):
        b = torch.randint(0, 256, shape, generator=gen, device=DEV, dtype=torch.uint8)
        return torch.where((b & 0x7f) == 0x7f, torch.zeros_like(b), b)
    kv = [(rand_bytes(k * G * N, C), rand_bytes(k * G, C, N)) for feats, N, C in LEVELS for _ in range(feats)]
    exps = torch.randint(-7, 16, (G, len(kv), 2), generator=gen, device=DEV, dtype=torch.int32)
    dev = PackedGarmentCache(G=G, timesteps=list(range(k, 0, -1)), h=H // 8, w=W // 8, dtype=dt, attn_fp8=False, f8_exp=(0, 0, 0),
                             weights_id="synthetic", kv=kv, exps=exps)
    host = dev.to("cpu", pin_memory=True)
    st = dict(gcache=host, gidx=list(range(k)), gindex=None, k=k, B=B, blocks=[(0, k)])
    slots, shapes = eng._cache_set_shapes(st)
    sets = {name: eng._alloc_set((), shapes, k, k, slots) for name in ("kv_stream", "kv_fill", "kv_unpack", "kv_place")}
    addr = {}

    def address(t):
        if t.data_ptr() not in addr:
            addr[t.data_ptr()] = ops.stream_address(t)
        return addr[t.data_ptr()]
    # the same records, two destinations (so that neither launch finds the other's lines in a cache) and two entry points
    tables = {}
    for name, cls in (("kv_stream", ops.KvStreamTable), ("kv_fill", ops.KvFillTable)):
        rec = fill_records(host.kv, k, G, sets[name]["kv"], k, slots, host.exps, list(range(k)), list(range(k)), [0], [0], address=address)
        tables[name] = cls(rec, DEV, ffi.KVS_WIDEN_E4M3)
    assert torch.equal(tables["kv_stream"].host[:, [0, 2, 3, 4]], tables["kv_fill"].host[:, [0, 2, 3, 4]]) and (tables["kv_fill"].host[:, 0] != 0).all()
    # the same table again with the same bytes in DEVICE memory: the parent's idmvton_kv_unpack against idmvton_kv_place
    rec = {name: fill_records(dev.kv, k, G, sets[name]["kv"], k, slots, dev.exps, list(range(k)), list(range(k)), [0], [0]) for name in ("kv_unpack", "kv_place")}
    unpack, place = ops.KvUnpackTable(rec["kv_unpack"], DEV), ops.KvPlaceTable(rec["kv_place"], DEV, ffi.KVS_WIDEN_E4M3)
    assert torch.equal(unpack.host[:, [0, 2, 3, 4]], place.host[:, [0, 2, 3, 4]]) and torch.equal(place.host[:, [3, 4]], tables["kv_fill"].host[:, [3, 4]])
    launches = {"kv_stream": lambda: tables["kv_stream"].launch(dt, 0, args.fill_workgroups), "kv_fill": lambda: tables["kv_fill"].launch(dt, 0, args.fill_workgroups),
                "kv_unpack": lambda: unpack.launch(dt), "kv_place": lambda: place.launch(dt)}
    src_bytes = sum(a.numel() + b.numel() for a, b in host.kv)
    us = {name: [] for name in launches}
    for pair in (("kv_stream", "kv_fill"), ("kv_unpack", "kv_place")):
        for name in pair:                                     # one discarded launch each
            launches[name]()
        torch.cuda.synchronize()
        for _ in range(9):                                    # alternating
            for name in pair:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize(); e0.record()
                launches[name]()
                e1.record(); e1.synchronize()
                us[name].append(e0.elapsed_time(e1) * 1e3)
    same = all(torch.equal(a, c) and torch.equal(b, d) for other in ("kv_fill", "kv_unpack", "kv_place")
               for (a, b), (c, d) in zip(sets["kv_stream"]["kv"], sets[other]["kv"]))
    gbps = {name: sorted(src_bytes / x / 1e3 for x in v) for name, v in us.items()}
    res = {name: dict(median_GBps=round(v[len(v) // 2], 2), min_GBps=round(v[0], 2), max_GBps=round(v[-1], 2), us=[round(x, 1) for x in us[name]],
                      median_us=round(sorted(us[name])[len(us[name]) // 2], 1)) for name, v in gbps.items()}
    ratio = res["kv_place"]["median_us"] / res["kv_unpack"]["median_us"]
    for name, r in res.items():
        print(f"{name:10s} median {r['median_us']:9.1f} us, {r['median_GBps']:8.2f} source GB/s (min {r['min_GBps']:.2f} .. max {r['max_GBps']:.2f}) over 9 launches", flush=True)
    emit(args, dict(step="fillrate", shape=f"{W}x{H}, one packed garment, one block of {k} timesteps, bf16 set, data-only table of {tables['kv_fill'].n} runs",
                    source_bytes=src_bytes, workgroups=args.fill_workgroups, bit_equal=same, place_over_unpack_median=round(ratio, 4),
                    place_within_3_percent_of_unpack_or_better=ratio <= 1.03, **res))
    return 0 if same else 1


def shelf_step(args):
    import bench
    import torch.nn.functional as F
    from idm_vton_amd import ops
    from idm_vton_amd.garment_cache import GarmentPool, GarmentShelf
    dt = torch.bfloat16
    eng, _ = bench.build_engine(dt, DEV, 0, STEPS)
    inp = bench.synth_inputs(B, H, W, STEPS, DEV, first_image_index=0)
    kw = dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler="ddim", use_graph=True, overlap=True)
    gh, gw = H // 2, W // 2                                   # 512 x 384 garments (height x width) for 1024 x 768 persons
    small = F.interpolate(inp["cloth"], size=(gh, gw), mode="bilinear", align_corners=False).clamp(-1, 1)
    noise_small = torch.randn(B, 4, gh // 8, gw // 8, generator=torch.Generator().manual_seed(5)).to(DEV)
    enc = lambda cloth, noise, i: eng.encode_garment(cloth=cloth[i:i + 1], text_embeds_cloth=inp["text_embeds_cloth"][i:i + 1], noise_cloth=noise[i:i + 1],
                                                     height=H, width=W, num_inference_steps=STEPS, scheduler="ddim", storage="e4m3")
    keys = [f"sku{i}" for i in range(B)]
    shelf = GarmentShelf(eng.empty_garment_cache(1, H, W, STEPS, scheduler="ddim", height=H, width=W), storage="e4m3")
    for i, key in enumerate(keys):
        shelf.add(key, enc(small, noise_small, i))
    shelved, index = shelf.get(keys)
    full = {key: enc(inp["cloth"], inp["noise"]["cloth"], i) for i, key in enumerate(keys)}
    pool = GarmentPool(B, like=full[keys[0]], resident="host")
    pool_index = pool.get(keys, encode=full.get)
    del full
    arms = {"shelf": (shelved, index, "kernel"), "device": (shelved.slotted(DEV), index, "kernel"), "host_full": (pool.cache, pool_index, "kernel"),
            "shelf_copy": (shelved, index, "copy")}

    def call(a, **more):
        cache, idx, transport = arms[a]
        return eng(**kw, **more, host_transport=transport, **{**inp, "cloth": cache, "garment_index": idx, "text_embeds_cloth": None})
    lat = {a: call(a, return_latents=True).clone() for a in arms}                             # warm-up: graph capture; and the latents
    torch.cuda.synchronize()
    # link and zero-tail bytes of ONE call, summed from the descriptor tables of its launches
    traffic, launch = {}, ops.KvStreamTable.launch
    for a in ("shelf", "host_full"):
        log = []

        def counted(self, dtype, which=0, workgroups=None, log=log):
            f0, c = self.slices[which]
            data = self.host[f0:f0 + c, 0] != 0
            log.append((16 * int(self.items[f0:f0 + c][data].sum()), 32 * int(self.items[f0:f0 + c][~data].sum())))
            return launch(self, dtype, which, workgroups)
        ops.KvStreamTable.launch = counted
        try:
            call(a)
        finally:
            ops.KvStreamTable.launch = launch
        torch.cuda.synchronize()
        traffic[a] = dict(launches=len(log), link_bytes_per_call=sum(x for x, _ in log), zero_tail_bytes_per_block=[z for _, z in log])
    rows = {a: [] for a in arms}
    for r in range(3):                                        # arms interleaved
        for a in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                call(a)
            torch.cuda.synchronize()
            rows[a].append(B * args.calls / (time.perf_counter() - t0))
            print(f"repeat {r} {a:10s} {rows[a][-1]:.4f} images/s", flush=True)
    equal = bool(torch.equal(lat["shelf"], lat["device"])) and bool(torch.equal(lat["shelf_copy"], lat["device"]))
    _, sched = eng._block_schedule(STEPS)
    emit(args, dict(step="shelf", shape=f"{W}x{H} persons, {gw}x{gh} packed garments, {STEPS} steps, B={B}, bf16, graph + overlap",
                    shelf_latents_equal_device_slotted=equal, ms_per_call={a: round(sum(1e3 * B / x for x in v) / len(v), 2) for a, v in rows.items()},
                    arena_bytes=[a.numel() for a, _ in eng._arenas.values()], images_per_s={a: [round(x, 4) for x in v] for a, v in rows.items()},
                    traffic=traffic, link_ratio_shelf_to_host_full=round(traffic["shelf"]["link_bytes_per_call"] / traffic["host_full"]["link_bytes_per_call"], 4),
                    block_timesteps=[c for _, c in sched], shelf_nbytes=shelf.nbytes, host_full_nbytes=pool.cache.nbytes))
    return 0 if equal else 1


def drive(args):
    import tempfile
    link = None
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEP_LIMITS:
            out = os.path.join(tmp, name + ".json")
            cmd = [sys.executable, os.path.abspath(__file__), "--step", name, "--calls", str(args.calls), "--json-out", out]
            if name == "call" and args.workgroups:
                cmd += ["--workgroups"] + [str(wg) for wg in args.workgroups]
            if name == "call" and link:
                cmd += ["--link-gbps", str(link)]
            print(f"--- step {name} (limit {limit} s)", flush=True)
            try:
                rc = subprocess.run(cmd, timeout=limit).returncode
            except subprocess.TimeoutExpired:
                print(f"step {name} ran out of its {limit} s: stopping here", flush=True)
                return 124
            if rc != 0:
                print(f"step {name} ended with status {rc}: stopping here", flush=True)
                return rc
            if name == "fill":
                link = json.load(open(out))["link_GBps"]
    return 0


def emit(args, res):
    print(json.dumps(res), flush=True)
    if args.json_out:
        with open(args.json_out, "w") as f:
            json.dump(res, f)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["fill", "call", "fillrate", "shelf"], default=None)
    ap.add_argument("--calls", type=int, default=2, help="timed calls per repeat")
    ap.add_argument("--workgroups", type=int, nargs="*", default=[], help="--step call: further host arms with these `workgroups` values")
    ap.add_argument("--json-out", default=None, help="also write the step's JSON result to this file (the driver reads the link rate from it)")
    ap.add_argument("--fill-workgroups", type=int, default=16, help="--step fillrate: persistent workgroups of both launches")
    ap.add_argument("--link-gbps", type=float, default=SPEC_GBPS, help="the host-link rate --step fill measured (default: the spec rate)")
    a = ap.parse_args()
    if a.step is None:
        sys.exit(drive(a))
    torch.cuda.set_device(0)
    with torch.no_grad():
        sys.exit({"fill": fill_step, "call": call_step, "fillrate": fillrate_step, "shelf": shelf_step}[a.step](a))
