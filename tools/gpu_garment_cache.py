"""Garment cache measurements (engine set-up imported from bench.py, not copied).

  (default)            cached vs uncached call at the configs[1] shape (768x1024, 30 steps, B = 2, bf16, hipGraph + two-stream overlap):
                       arms `uncached`, `cached_G2`, `cached_G1` interleaved over --rounds rounds of --calls timed calls each, one warm-up call
                       per arm discarded; images/s, loop ms/step, encode_garment time and cache.nbytes -> one JSON line
  --cloth-size HxW     the same with a garment image of its own size (e.g. 512x384: a quarter of the tokens at every level, a quarter of the
                       cache); the person stays 768x1024.  --arms picks a subset of the arms (an A/B against another tree: uncached only)
  --nbytes-only        only build the cache and print its size (with --attn-fp8: the e4m3 form)
  --attn               the self-attention launches on their own: the six CFG lines of profiles/r06_attention_sp_tuner_lines.txt through the OLD
                       entry point (IDMVTON_HIP_LIB selects the build: run once per build, interleaved, for an A/B), then shared vs materialised
                       garment segment at P = 4, G = 1 on the level-1 / level-2 shapes (--old-only: without that part, for a tree that
                       predates the shared entry point)
  --pmc-arm shared|mat 20 launches of one arm of the P = 4, G = 1 pair at --pmc-level 1|2, for a `rocprofv3 --pmc FETCH_SIZE` run of its own
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from idm_vton_amd import ops  # noqa: E402

DEV, DT = torch.device("cuda", 0), torch.bfloat16
H, W, STEPS, B = 1024, 768, 30, 2


def cloth_size(text):
    hg, wg = (int(x) for x in text.lower().split("x"))
    if hg % 8 or wg % 8 or hg < 8 or wg < 8:
        raise argparse.ArgumentTypeError(f"--cloth-size {text}: height and width must be multiples of 8")
    return hg, wg


def with_cloth_of_size(inp, Hg, Wg, device=None):
    """The call's inputs with a garment image of Hg x Wg and the posterior draw of its latent: the cloth fields of bench.synth_inputs at that
    size (same per-image seeds), everything else untouched."""
    g = bench.synth_inputs(inp["image"].shape[0], Hg, Wg, 1, device or inp["image"].device, first_image_index=0)
    return {**inp, "cloth": g["cloth"], "noise": {**inp["noise"], "cloth": g["noise"]["cloth"]}}


def call_arms(args):
    eng, _ = bench.build_engine(DT, DEV, 0, STEPS, attn_fp8=args.attn_fp8)
    inp = bench.synth_inputs(B, H, W, STEPS, DEV, first_image_index=0)
    Hg, Wg = args.cloth_size or (H, W)
    if (Hg, Wg) != (H, W):
        inp = with_cloth_of_size(inp, Hg, Wg)
    gh, gw = Hg // 8, Wg // 8
    n1, n2 = ops.round16((gh + 1) // 2 * ((gw + 1) // 2)), ops.round16((gh + 3) // 4 * ((gw + 3) // 4))      # token rows at the two attention levels
    want = [a for a in args.arms.split(",") if a]
    kw = dict(num_inference_steps=STEPS, guidance_scale=2.0, scheduler="ddim", use_graph=True, overlap=True)
    garm = lambda G: dict(cloth=inp["cloth"][:G], text_embeds_cloth=inp["text_embeds_cloth"][:G], noise_cloth=inp["noise"]["cloth"][:G],
                          height=H, width=W)
    caches, enc_ms = {}, {}
    for G in ((2,) if args.nbytes_only else tuple(g for g in (2, 1) if f"cached_G{g}" in want)):
        eng.encode_garment(num_inference_steps=STEPS, scheduler="ddim", **garm(G))          # warm-up (shape discovery, allocator)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        caches[G] = eng.encode_garment(num_inference_steps=STEPS, scheduler="ddim", **garm(G))
        torch.cuda.synchronize()
        enc_ms[G] = (time.perf_counter() - t0) * 1e3
    res = {"shape": f"{W}x{H}, cloth {Wg}x{Hg}, {STEPS} steps, B={B}, bf16{' + fp8 attention' if args.attn_fp8 else ''}",
           "cache_nbytes": {f"G{G}": c.nbytes for G, c in caches.items()}, "encode_garment_ms": {f"G{G}": round(v, 1) for G, v in enc_ms.items()},
           "derived_bytes_per_garment_16bit": (10 * n1 * 640 + 60 * n2 * 1280) * 2 * 2 * STEPS}
    if args.nbytes_only:
        print(json.dumps(res))
        return
    arms = {"uncached": inp, **{f"cached_G{G}": {**inp, "cloth": c, "text_embeds_cloth": None} for G, c in caches.items()}}
    arms = {a: arms[a] for a in want}
    outs, rows = {}, {a: [] for a in arms}
    for a, ai in arms.items():                            # warm-up: graph capture, discarded
        outs[a] = eng(**kw, **ai).clone()
    torch.cuda.synchronize()
    for r in range(args.rounds):
        for a, ai in arms.items():
            timing = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                eng(timing=timing, **kw, **ai)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            loop = sum(t[1].elapsed_time(t[2]) for t in timing) / len(timing) / STEPS
            prep = sum(t[0].elapsed_time(t[1]) for t in timing) / len(timing)
            rows[a].append(dict(images_per_s=B * args.calls / dt, loop_ms_per_step=loop, prepare_ms=prep))
            print(f"round {r} {a:10s} {B * args.calls / dt:.4f} images/s  loop {loop:.3f} ms/step  prepare {prep:.1f} ms", flush=True)
    res["arms"] = {a: dict(images_per_s=[round(x["images_per_s"], 4) for x in v], loop_ms_per_step=[round(x["loop_ms_per_step"], 3) for x in v],
                           prepare_ms=[round(x["prepare_ms"], 1) for x in v]) for a, v in rows.items()}
    # same garment noise and same per-garment batches: the G = 2 cached call computes the uncached call's latents (its person-side VAE encodes
    # run at another batch size, so the images are compared, not asserted equal)
    if "cached_G2" in outs and "uncached" in outs:
        res["max_abs_image_diff_cached_G2_vs_uncached"] = (outs["cached_G2"].float() - outs["uncached"].float()).abs().max().item()
    res["garment_batches_total"] = eng.stats["garment_batches"]
    print(json.dumps(res))


def timed(fn, n=40):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(n):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def _rand(*s):
    return torch.randn(*s, device=DEV, dtype=torch.float32).to(DT)


def attn_launch(Bq, heads, N, nk2, b0, nb=0, garments=None, nk1=None):
    """The engine's attn1 launch: q | k in one [Bq*N][2C] tensor, own segment + (nk2 > 0) a garment segment from batch b0 on.  nk1: the first
    segment holds nk1 keys of its own instead of the N tokens (the text / image-token launches among the tuner's lines)."""
    C = heads * 64
    qk, vt = _rand(Bq * N, 2 * C), _rand(Bq, C, N)
    segs = [dict(k=qk[:, C:], vt=vt, nk=N, ldk=2 * C, ldvt=N, k_rows=N)]
    if nk1 is not None:
        segs = [dict(k=_rand(Bq * nk1, C), vt=_rand(Bq, C, ops.round16(nk1)), nk=nk1, ldk=C, ldvt=ops.round16(nk1), k_rows=nk1)]
    if nk2:
        Bg = garments if garments is not None else Bq - b0
        ld = ops.round16(nk2)
        seg = dict(k=_rand(Bg * nk2, C), vt=_rand(Bg, C, ld), nk=nk2, ldk=C, ldvt=ld, k_rows=nk2, b0=b0)
        if nb:
            assert hasattr(ops, "_seg_nb"), "this build of the package has no shared-segment entry point"
            seg["nb"] = nb
        segs.append(seg)
    out = torch.empty(Bq * N, C, dtype=DT, device=DEV)
    return lambda: ops.attention(qk, out, segs, heads, B=Bq, Nq=N, ldq=2 * C, ldo=C, q_prescaled=True)


LEVELS = {1: (10, 3072), 2: (20, 768)}


def shared_pair(level, P=4):
    heads, N = LEVELS[level]
    return dict(shared=attn_launch(2 * P, heads, N, N, P, nb=1, garments=1), mat=attn_launch(2 * P, heads, N, N, P))


def attn_mode(args):
    torch.manual_seed(0)
    print("library:", os.environ.get("IDMVTON_HIP_LIB", "(in-tree)"))
    # (dtype, mode, B, heads, Nq, nseg, nk0, nk1, b0): the six lines of profiles/r06_attention_sp_tuner_lines.txt, old entry point
    for Bq, heads, N, nk1, nk2, b0 in ((4, 20, 768, None, 768, 2), (12, 20, 768, None, 0, 0), (12, 20, 768, 77, 0, 0), (4, 10, 3072, None, 3072, 2),
                                       (12, 10, 3072, None, 0, 0), (4, 20, 16, 257, 16, 0)):
        fn = attn_launch(Bq, heads, N, nk2, b0, nk1=nk1)
        ts = [timed(fn) for _ in range(3)]
        print(f"old entry  B={Bq:2d} heads={heads} N={N} keys={nk1 or N}+{nk2} b0={b0}: " + " ".join(f"{t:7.1f}" for t in ts) + " us", flush=True)
    for level in (() if args.old_only else (1, 2)):
        pair = shared_pair(level)
        for rep in range(3):                               # arms interleaved
            for arm, fn in pair.items():
                print(f"P=4 G=1 level {level} {arm:6s} rep {rep}: {timed(fn):7.1f} us", flush=True)


def pmc_mode(args):
    torch.manual_seed(0)
    fn = shared_pair(args.pmc_level)[args.pmc_arm]
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    print("launched 20 x", args.pmc_arm, "level", args.pmc_level)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--attn-fp8", action="store_true")
    ap.add_argument("--nbytes-only", action="store_true")
    ap.add_argument("--cloth-size", type=cloth_size, default=None, metavar="HxW", help="garment image size (default: the person's 1024x768)")
    ap.add_argument("--arms", default="uncached,cached_G2,cached_G1", help="comma-separated subset of uncached, cached_G2, cached_G1")
    ap.add_argument("--attn", action="store_true")
    ap.add_argument("--old-only", action="store_true", help="--attn: only the old entry point's lines (A/B against a tree without the shared one)")
    ap.add_argument("--pmc-arm", choices=["shared", "mat"], default=None)
    ap.add_argument("--pmc-level", type=int, choices=[1, 2], default=1)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    with torch.no_grad():
        pmc_mode(a) if a.pmc_arm else attn_mode(a) if a.attn else call_arms(a)
