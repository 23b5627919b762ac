"""-m gpu: the garment cache on the GPU.  Kernel level: the shared (broadcast) key segment of idmvton_attn_fwd_shared / idmvton_attn_f8_shared
against the old entry points fed the same K / V^T materialised once per person -- same kernel, same tiles, same values, so EQUALITY, no
tolerance.  Engine level: a call on a GarmentCache against the uncached call (bit for bit, every execution form), shared against
materialised (bit for bit), against the oracle (the bars of tests/parity_checks.py, which tests/test_parity_gpu.py is held to), and the boundary pipeline."""
import pytest
import torch
import torch.nn.functional as F

from tests.engine_support import (DEV, boundary_inputs, boundary_pipeline, engine_inputs, engine_reference, f8_operands, garment_kw, ip_states, pair,
                                  reference_draws, self_attn_operands)
from tests.garment_support import DTYPES, FORMS, HEADS, SHAPES
from tests.kernel_checks import TUNES

pytestmark = pytest.mark.gpu
PERSONS_GARMENTS = [(2, 1), (4, 1), (2, 2), (4, 2)]


@DTYPES
@pytest.mark.parametrize("tune", list(TUNES), ids=list(TUNES))
def test_shared_segment_equals_materialised_copies(tune, dtype):
    from idm_vton_amd import ops
    from tests.kernel_checks import TOL as KTOL
    for Nq, nkg in SHAPES:
        for P, G in PERSONS_GARMENTS:
            q, k1, v1, k2, v2, ko = self_attn_operands(P, G, Nq, nkg, dtype, seed=7 * P + G)
            B, Cc = 2 * P, HEADS * 64
            pres = tune != "auto"                        # kernels 3, 7, 8, 16 need a pre-multiplied q; `auto` runs the library's rule for a raw q
            qq = (q.float() * ops.QSCALE).to(dtype) if pres else q
            vt1, ld1 = ko(v1, Nq)
            vt2, ld2 = ko(v2, nkg)
            own = dict(k=k1, vt=vt1, nk=Nq, ldk=Cc, ldvt=ld1)
            shared = dict(k=k2, vt=vt2, nk=nkg, ldk=Cc, ldvt=ld2, b0=P, nb=G)
            mat = dict(k=k2.repeat(P // G, 1, 1).contiguous(), vt=vt2.repeat(P // G, 1, 1).contiguous(), nk=nkg, ldk=Cc, ldvt=ld2, b0=P)
            o_s = torch.full((B, Nq, Cc), float("nan"), dtype=dtype, device=DEV)
            o_m = torch.full((B, Nq, Cc), float("nan"), dtype=dtype, device=DEV)
            ops.attention(qq, o_s, [own, shared], HEADS, tune=TUNES[tune], q_prescaled=pres)
            ops.attention(qq, o_m, [own, mat], HEADS, tune=TUNES[tune], q_prescaled=pres)
            assert torch.isfinite(o_m).all(), (tune, Nq, nkg, P, G)
            assert torch.equal(o_s, o_m), (tune, Nq, nkg, P, G, (o_s.float() - o_m.float()).abs().max().item())
            if G == 1 and P == 2:                        # the values are attention, not merely equal: fp32 SDPA on the same operands
                sp = lambda t: t.float().view(t.shape[0], t.shape[1], HEADS, 64).transpose(1, 2)
                z = torch.zeros(P, HEADS, nkg, 64, device=DEV)
                kk = torch.cat([sp(k1), torch.cat([z, sp(k2).expand(P, -1, -1, -1)])], dim=2)
                vv = torch.cat([sp(v1), torch.cat([z, sp(v2).expand(P, -1, -1, -1)])], dim=2)
                ref = F.scaled_dot_product_attention(sp(qq) / (ops.QSCALE if pres else 1.0), kk, vv).transpose(1, 2).reshape(B, Nq, Cc)
                err = ((o_s.float() - ref).abs().max() / ref.abs().max()).item()
                assert err <= KTOL[dtype], (tune, err)  # the bar tests/kernel_checks.py holds check_attn_self to (imported)


@DTYPES
def test_shared_segment_equals_materialised_copies_fp8(dtype):
    from idm_vton_amd import ops
    for Nq, nkg in SHAPES:
        for P, G in PERSONS_GARMENTS:
            B, Cc = 2 * P, HEADS * 64
            q8, (k8a, vt8a), (k8b, vt8b) = f8_operands(P, G, Nq, nkg, dtype, seed=5 * P + G)
            ld = vt8b.shape[1]
            own = dict(k8=k8a, vt8=vt8a, nk=Nq, ldk=Cc, ldvt=vt8a.shape[1])
            shared = dict(k8=k8b, vt8=vt8b, nk=nkg, ldk=Cc, ldvt=ld, b0=P, nb=G)
            mat = dict(k8=k8b.view(G, nkg * Cc).repeat(P // G, 1).view(P * nkg, Cc).contiguous(),
                       vt8=vt8b.view(G, Cc * ld).repeat(P // G, 1).view(P * Cc, ld).contiguous(), nk=nkg, ldk=Cc, ldvt=ld, b0=P)
            o_s = torch.full((B, Nq, Cc), float("nan"), dtype=dtype, device=DEV)
            o_m = torch.full((B, Nq, Cc), float("nan"), dtype=dtype, device=DEV)
            kw = dict(qk_scale_exp=-4, v_scale_exp=-2, B=B, Nq=Nq, ldq=Cc, ldo=Cc)
            ops.attention_f8(q8, o_s, [own, shared], HEADS, **kw)
            ops.attention_f8(q8, o_m, [own, mat], HEADS, **kw)
            assert torch.isfinite(o_m).all() and torch.equal(o_s, o_m), (Nq, nkg, P, G)


@DTYPES
def test_old_entry_points_equal_the_shared_ones_with_zero_seg_nb(dtype, monkeypatch):
    """seg_nb = {0, 0} is the old rule: idmvton_attn_fwd / idmvton_attn_f8 and their _shared forms give the same bits."""
    from idm_vton_amd import ops
    calls = []
    real_shared = ops.ffi.call_shared
    monkeypatch.setattr(ops.ffi, "call_shared", lambda fn, a, nb, st: (calls.append((fn, list(nb))), real_shared(fn, a, nb, st))[1])
    P, Nq, nkg = 2, 320, 200
    B, Cc = 2 * P, HEADS * 64
    q, k1, v1, k2, v2, ko = self_attn_operands(P, P, Nq, nkg, dtype, seed=3)
    qq = (q.float() * ops.QSCALE).to(dtype)
    vt1, ld1 = ko(v1, Nq)
    vt2, ld2 = ko(v2, nkg)
    segs = [dict(k=k1, vt=vt1, nk=Nq, ldk=Cc, ldvt=ld1), dict(k=k2, vt=vt2, nk=nkg, ldk=Cc, ldvt=ld2, b0=P)]
    q8, (k8a, vt8a), (k8b, vt8b) = f8_operands(P, P, Nq, nkg, dtype, seed=3)
    segs8 = [dict(k8=k8a, vt8=vt8a, nk=Nq, ldk=Cc, ldvt=vt8a.shape[1]), dict(k8=k8b, vt8=vt8b, nk=nkg, ldk=Cc, ldvt=vt8b.shape[1], b0=P)]
    outs = {}
    for form in ("old", "shared0"):
        if form == "shared0":
            monkeypatch.setattr(ops, "_seg_nb", lambda s: [0, 0])
        for name, tune in TUNES.items():
            o = torch.full((B, Nq, Cc), float("nan"), dtype=dtype, device=DEV)
            ops.attention(qq, o, segs, HEADS, tune=tune, q_prescaled=True)
            outs[(form, name)] = o
        o = torch.full((B, Nq, Cc), float("nan"), dtype=dtype, device=DEV)
        ops.attention_f8(q8, o, segs8, HEADS, qk_scale_exp=-4, v_scale_exp=-2, B=B, Nq=Nq, ldq=Cc, ldo=Cc)
        outs[(form, "f8")] = o
        assert len(calls) == (0 if form == "old" else len(TUNES) + 1)
    assert all(nb == [0, 0] for _, nb in calls) and {fn for fn, _ in calls} == {"idmvton_attn_fwd_shared", "idmvton_attn_f8_shared"}
    for name in list(TUNES) + ["f8"]:
        assert torch.isfinite(outs[("old", name)]).all() and torch.equal(outs[("old", name)], outs[("shared0", name)]), name


# ------------------------------------------------------------------------------------------------------------------ engine


@pytest.mark.parametrize("scheduler", ["ddpm", "ddim"])
@DTYPES
def test_cached_loop_is_bit_identical_to_the_uncached_loop(dtype, scheduler):
    """n = 7 steps: blocks of 1, 2, 4 timesteps.  encode_garment runs the same GarmentNet batches an uncached call runs, so the cached K / V^T
    are that call's bits and every execution form must reproduce its latents exactly."""
    steps = 7
    eng, inp, _ = engine_inputs(dtype, 2, steps)
    kw = dict(num_inference_steps=steps, guidance_scale=2.0, scheduler=scheduler, **inp)
    cache = eng.encode_garment(num_inference_steps=steps, scheduler=scheduler, **garment_kw(inp))
    assert cache.G == 2 and len(cache.timesteps) == steps and cache.nbytes > 0
    for form in FORMS:
        lat_u, lat_c = pair(eng, kw, cache, form)
        print(f"{dtype} {scheduler} {form}: max|cached - uncached| = {(lat_u - lat_c).abs().max().item():.3e}")
        assert torch.isfinite(lat_u).all() and torch.equal(lat_u, lat_c), (form, (lat_u - lat_c).abs().max().item())


def test_cached_loop_is_bit_identical_with_fp8_attention():
    steps = 7
    eng, inp, _ = engine_inputs(torch.float16, 2, steps, fp8=True)
    kw = dict(num_inference_steps=steps, guidance_scale=2.0, scheduler="ddpm", **inp)
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp))
    assert cache.attn_fp8 and {k.dtype for k, _ in cache.kv} == {torch.uint8, torch.float16}    # e4m3 where whole 64-key tiles, else 16-bit
    for form in ("serial_eager", "graph_overlap"):
        lat_u, lat_c = pair(eng, kw, cache, form)
        print(f"fp8 {form}: max|cached - uncached| = {(lat_u - lat_c).abs().max().item():.3e}")
        assert torch.isfinite(lat_u).all() and torch.equal(lat_u, lat_c), form


@DTYPES
def test_cache_built_at_full_strength_serves_strength_0_6(dtype):
    """The cache of the 7-step schedule serves strength = 0.6: the last int(7 * 0.6) = 4 of its timesteps, found by value."""
    steps = 7
    eng, inp, _ = engine_inputs(dtype, 2, steps)
    inp["noise"]["image"] = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(77))
    inp["noise"]["steps"] = inp["noise"]["steps"][:4]
    kw = dict(num_inference_steps=steps, guidance_scale=2.0, scheduler="ddpm", strength=0.6, **inp)
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp))                    # strength = 1
    for form in ("serial_eager", "graph_overlap"):
        lat_u, lat_c = pair(eng, kw, cache, form)
        print(f"{dtype} strength 0.6 {form}: max|cached - uncached| = {(lat_u - lat_c).abs().max().item():.3e}")
        assert torch.isfinite(lat_u).all() and torch.equal(lat_u, lat_c), (form, (lat_u - lat_c).abs().max().item())


@pytest.mark.parametrize("mode", ["f16", "bf16", "f16_fp8"])
def test_one_shared_garment_equals_the_garment_held_once_per_person(mode):
    """P = 2 persons, G = 1 garment: the shared key segment against a cache that holds the garment twice."""
    dtype = torch.bfloat16 if mode == "bf16" else torch.float16
    steps = 5
    eng, inp, _ = engine_inputs(dtype, 2, steps, fp8=mode.endswith("fp8"))
    cache1 = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp, 1))
    cache2 = cache1.repeat_garments(2)
    assert (cache1.G, cache2.G) == (1, 2) and cache2.nbytes == 2 * cache1.nbytes
    base = dict(num_inference_steps=steps, guidance_scale=2.0, scheduler="ddpm", **{**inp, "text_embeds_cloth": None})
    for form in ("serial_eager", "graph", "graph_overlap"):
        lats = [eng.denoise(eng.prepare(**{**base, "cloth": c}), **FORMS[form]).clone() for c in (cache1, cache2)]
        assert torch.isfinite(lats[0]).all() and torch.equal(lats[0], lats[1]), form
    # and the second person really wears garment 0: a cache of two different garments gives other latents
    other = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp, 2))
    assert not torch.equal(eng.denoise(eng.prepare(**{**base, "cloth": other})).clone(), lats[0])


@DTYPES
def test_cached_call_against_the_oracle(dtype):
    """The whole cached call, decode included, at the size / step count of test_parity_gpu.test_tiny_pipeline_parity and held to its bars."""
    from oracle import pipeline as opipe
    from oracle.scheduler import Scheduler
    from tests.parity_checks import TOL
    from tests import parity_utils as pu
    steps = 4
    eng, inp, m = engine_inputs(dtype, 1, steps)
    o_t, o_g, o_v = m["oracle"]
    tr = {}
    img_o = opipe.run(o_t, o_g, o_v, Scheduler("ddpm"), num_inference_steps=steps, guidance_scale=2.0, trace=tr, **inp)
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp))
    call = dict(num_inference_steps=steps, guidance_scale=2.0, scheduler="ddpm", **{**inp, "cloth": cache, "text_embeds_cloth": None})
    for kw in (dict(), dict(use_graph=True, overlap=True)):
        lat = eng(return_latents=True, **kw, **call).clone()
        img = eng(**kw, **call)
        e_lat, e_img = pu.relerr(lat, tr["step_latents"][-1]), pu.relerr(img, img_o)
        print(f"{dtype} {kw}: latents {e_lat:.3e} image {e_img:.3e}")
        assert e_lat <= TOL[dtype]["latents"] and e_img <= TOL[dtype]["image"], (kw, e_lat, e_img)


def test_a_call_on_a_cache_runs_no_garmentnet_batch_and_a_wrong_cache_is_refused():
    steps = 7
    eng, inp, _ = engine_inputs(torch.float16, 2, steps)
    kw = dict(num_inference_steps=steps, guidance_scale=2.0, scheduler="ddpm", **inp)
    eng.denoise(eng.prepare(**kw), **FORMS["graph_overlap"])                         # (the first graph call also runs one warm-up batch)
    for form in ("serial_eager", "graph_overlap"):
        n0 = eng.stats["garment_batches"]
        st = eng.prepare(**kw)
        eng.denoise(st, **FORMS[form])
        assert eng.stats["garment_batches"] - n0 == len(st["blocks"]) == 3          # 1 + 2 + 4 timesteps: launched, or replayed
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp))
    n1 = eng.stats["garment_batches"]
    ckw = {**kw, "cloth": cache, "text_embeds_cloth": None}
    for form in FORMS:
        for _ in range(2):
            eng.denoise(eng.prepare(**ckw), **FORMS[form])
    torch.cuda.synchronize()
    assert eng.stats["garment_batches"] == n1
    assert eng.stats["garment_set_copies"] > 0                                       # the graph forms moved cache blocks into their sets
    with pytest.raises(ValueError, match="GarmentCache timesteps mismatch"):
        eng.prepare(**{**ckw, "num_inference_steps": 5, "noise": {**inp["noise"], "steps": inp["noise"]["steps"][:5]}})
    with pytest.raises(ValueError, match="GarmentCache resolution mismatch"):
        eng.prepare(**{**ckw, "height": 64, "width": 64})
    three = {k: (torch.cat([v, v[:1]]) if torch.is_tensor(v) and k != "ip_hidden_states" else v) for k, v in ckw.items()}
    with pytest.raises(ValueError, match="GarmentCache persons mismatch"):
        eng.prepare(**three)
    eng2, _, _ = engine_inputs(torch.bfloat16, 2, steps)
    with pytest.raises(ValueError, match="GarmentCache dtype mismatch"):
        eng2.prepare(**ckw)


def test_captured_graphs_do_not_keep_a_cache_alive():
    """The persistent graph state owns its buffers and nothing of a call: once the caller drops a GarmentCache (gigabytes at full size) it
    is freed although the engine and the graphs captured on that call live on, and the next cache runs through the same graphs."""
    import gc
    import weakref
    steps = 3
    eng, inp, _ = engine_inputs(torch.float16, 2, steps)
    call = lambda c: dict(num_inference_steps=steps, guidance_scale=2.0, scheduler="ddpm",
                          **{**inp, "cloth": c, "text_embeds_cloth": None, "noise": {**inp["noise"], "cloth": None}})
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp))
    st = eng.prepare(**call(cache))
    first = eng.denoise(st, **FORMS["graph_overlap"]).clone()
    ref = weakref.ref(cache)
    del cache, st
    gc.collect()
    assert ref() is None, "the engine's graph state still refers to the first call's GarmentCache"
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp))
    again = eng.denoise(eng.prepare(**call(cache)), **FORMS["graph_overlap"]).clone()
    serial = eng.denoise(eng.prepare(**call(cache)), **FORMS["serial_eager"]).clone()
    assert torch.isfinite(serial).all() and torch.equal(again, serial) and torch.equal(first, serial)


# ------------------------------------------------------------------------------------------------------------------ boundary


def test_boundary_pipeline_takes_the_cache_as_cloth():
    from idm_vton_amd.garment_cache import GarmentCache
    DT = torch.float16
    pipe, enc, kw = boundary_pipeline(DT)
    B, H, W, steps = 2, 128, 128, 3
    inp, clip_pix, call = boundary_inputs(kw, B, H, W, steps, DT)
    cache = pipe.encode_garment(inp["cloth"], inp["text_embeds_cloth"], steps, H, W, generator=torch.Generator(DEV).manual_seed(11))
    assert isinstance(cache, GarmentCache) and cache.G == B and len(cache.timesteps) == steps
    eng = pipe.hip_engine()
    n_garm = eng.stats["garment_batches"]
    gen_c = torch.Generator(DEV).manual_seed(7)
    torch.manual_seed(123)                                                         # the pose posterior uses the GLOBAL generator
    img_c = pipe(generator=gen_c, cloth=cache, text_embeds_cloth=None, **call)[0]
    assert eng.stats["garment_batches"] == n_garm
    # the engine-level cached call on the draws of the reference's order: the cloth draw is made and dropped
    gen, noise = reference_draws(7, 123, B, H, W, steps, DT)
    ip = ip_states(enc, clip_pix)
    ref = engine_reference(eng, inp, noise, ip, steps, cloth=cache)
    assert torch.isfinite(img_c).all() and torch.equal(img_c, ref)
    # an uncached call with the same generator leaves it in the same state: the cached call made every draw of it
    gen_u = torch.Generator(DEV).manual_seed(7)
    torch.manual_seed(123)
    img_u = pipe(generator=gen_u, cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"], **call)[0]
    assert torch.equal(gen_c.get_state(), gen_u.get_state())
    assert torch.equal(gen_c.get_state(), gen.get_state())
    assert img_u.shape == img_c.shape and not torch.equal(img_u, img_c)           # (other cloth posterior noise: seed 11 against the call's third draw)
    with pytest.raises(ValueError, match="`cloth` is required"):
        pipe(generator=gen_u, cloth=None, text_embeds_cloth=None, **call)
