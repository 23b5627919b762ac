"""-m gpu: any person wears any cached garment, by index.  Kernel level: the indexed key segment of idmvton_attn_fwd_indexed /
idmvton_attn_f8_indexed (query batch b reads element table[b - b0] of the nb a pool holds) against the plain entry points fed k[idx] / vt[idx]
materialised once per person -- same kernel, same tiles, same values, so EQUALITY, no tolerance.  Engine level: a call with garment_index
on a G-garment cache against the call on cache.select(garment_index) (bit for bit, every execution form), indices that change between two
replays of one captured graph set, a garment swapped in place, pools larger than the batch, refusals, and the boundary pipeline.
No test hands a kernel an index outside [0, nb): the kernels' clamp is a guard."""
import pytest
import torch
import torch.nn.functional as F

from tests.engine_support import (DEV, base_call, boundary_inputs, boundary_pipeline, engine_inputs, engine_reference, f8_operands, garment_kw, int_table,
                                  ip_states, model, nan_out, reference_draws, run_on, self_attn_operands)
from tests.garment_support import DTYPES, F8_SDPA_BAR, FORMS, HEADS, IDX, SHAPES, pool_cache, same_values
from tests.kernel_checks import TUNES

pytestmark = pytest.mark.gpu

# (P, G, index): P % G != 0 with a repeated value, not monotone; a pool larger than the batch; one garment for all
PATTERNS = [(4, 3, [2, 0, 2, 1]), (2, 5, [4, 4]), (3, 1, [0, 0, 0])]
# index = [i % G]: what the shared segment reads
MODULO = [(4, 2, [0, 1, 0, 1]), (3, 1, [0, 0, 0]), (3, 3, [0, 1, 2])]


def _segments16(P, G, Nq, nkg, dtype, seed, pres):
    from idm_vton_amd import ops
    q, k1, v1, k2, v2, ko = self_attn_operands(P, G, Nq, nkg, dtype, seed)
    qq = (q.float() * ops.QSCALE).to(dtype) if pres else q
    vt1, ld1 = ko(v1, Nq)
    vt2, ld2 = ko(v2, nkg)
    Cc = HEADS * 64
    own = dict(k=k1, vt=vt1, nk=Nq, ldk=Cc, ldvt=ld1)
    garment = lambda kk, vv, **kw: dict(k=kk, vt=vv, nk=nkg, ldk=Cc, ldvt=ld2, b0=P, **kw)
    return qq, own, garment, (k1, v1, k2, v2, vt2)


@DTYPES
@pytest.mark.parametrize("tune", list(TUNES), ids=list(TUNES))
def test_indexed_segment_equals_materialised_copies(tune, dtype):
    from idm_vton_amd import ops
    from tests.kernel_checks import TOL as KTOL
    pres = tune != "auto"                                # kernels 3, 7, 8, 16 need a pre-multiplied q; `auto` runs the library's rule for a raw q
    for Nq, nkg in SHAPES:
        for P, G, idx in PATTERNS:
            B, Cc = 2 * P, HEADS * 64
            qq, own, garment, (k1, v1, k2, v2, vt2) = _segments16(P, G, Nq, nkg, dtype, 11 * P + G, pres)
            o_i, o_m = nan_out(B, Nq, Cc, dtype), nan_out(B, Nq, Cc, dtype)
            ops.attention(qq, o_i, [own, garment(k2, vt2, nb=G, index=int_table(idx))], HEADS, tune=TUNES[tune], q_prescaled=pres)
            ops.attention(qq, o_m, [own, garment(k2[idx].contiguous(), vt2[idx].contiguous())], HEADS, tune=TUNES[tune], q_prescaled=pres)
            assert torch.isfinite(o_m).all(), (tune, Nq, nkg, idx)
            assert torch.equal(o_i, o_m), (tune, Nq, nkg, P, G, idx, (o_i.float() - o_m.float()).abs().max().item())
            if (P, G) == (2, 5):                         # the values are attention, not merely equal: fp32 SDPA on the same operands
                sp = lambda t: t.float().view(t.shape[0], t.shape[1], HEADS, 64).transpose(1, 2)
                z = torch.zeros(P, HEADS, nkg, 64, device=DEV)
                kk = torch.cat([sp(k1), torch.cat([z, sp(k2[idx])])], dim=2)
                vv = torch.cat([sp(v1), torch.cat([z, sp(v2[idx])])], dim=2)
                ref = F.scaled_dot_product_attention(sp(qq) / (ops.QSCALE if pres else 1.0), kk, vv).transpose(1, 2).reshape(B, Nq, Cc)
                err = ((o_i.float() - ref).abs().max() / ref.abs().max()).item()
                print(f"{tune} {dtype} Nq={Nq} nkg={nkg}: indexed against fp32 SDPA {err:.3e} (bar {KTOL[dtype]:.1e})")
                assert err <= KTOL[dtype], (tune, err)  # the bar tests/kernel_checks.py holds check_attn_self to (imported)


@DTYPES
@pytest.mark.parametrize("tune", list(TUNES), ids=list(TUNES))
def test_the_modulo_table_equals_the_shared_segment(tune, dtype):
    from idm_vton_amd import ops
    pres = tune != "auto"
    Nq, nkg = SHAPES[0]
    for P, G, idx in MODULO:
        B, Cc = 2 * P, HEADS * 64
        qq, own, garment, (_, _, k2, _, vt2) = _segments16(P, G, Nq, nkg, dtype, 13 * P + G, pres)
        o_i, o_s = nan_out(B, Nq, Cc, dtype), nan_out(B, Nq, Cc, dtype)
        ops.attention(qq, o_i, [own, garment(k2, vt2, nb=G, index=int_table(idx))], HEADS, tune=TUNES[tune], q_prescaled=pres)
        ops.attention(qq, o_s, [own, garment(k2, vt2, nb=G if G < P else 0)], HEADS, tune=TUNES[tune], q_prescaled=pres)
        assert torch.isfinite(o_s).all() and torch.equal(o_i, o_s), (tune, P, G)


def _segments8(P, G, Nq, nkg, dtype, seed):
    q8, (k8a, vt8a), (k8b, vt8b) = f8_operands(P, G, Nq, nkg, dtype, seed)
    Cc, ld = HEADS * 64, vt8b.shape[1]
    own = dict(k8=k8a, vt8=vt8a, nk=Nq, ldk=Cc, ldvt=vt8a.shape[1])
    garment = lambda kk, vv, **kw: dict(k8=kk, vt8=vv, nk=nkg, ldk=Cc, ldvt=ld, b0=P, **kw)
    return q8, own, garment, k8b, vt8b


@DTYPES
def test_indexed_segment_equals_materialised_copies_fp8(dtype):
    from idm_vton_amd import ops
    from tests.kernel_checks import TOL as KTOL
    for Nq, nkg in SHAPES:
        for P, G, idx in PATTERNS + MODULO:
            B, Cc = 2 * P, HEADS * 64
            q8, own, garment, k8b, vt8b = _segments8(P, G, Nq, nkg, dtype, 5 * P + G)
            ld = vt8b.shape[1]
            kw = dict(qk_scale_exp=-4, v_scale_exp=-2, B=B, Nq=Nq, ldq=Cc, ldo=Cc)
            o_i, o_m = nan_out(B, Nq, Cc, dtype), nan_out(B, Nq, Cc, dtype)
            ops.attention_f8(q8, o_i, [own, garment(k8b, vt8b, nb=G, index=int_table(idx))], HEADS, **kw)
            k_m = k8b.view(G, nkg * Cc)[idx].reshape(P * nkg, Cc).contiguous()
            vt_m = vt8b.view(G, Cc * ld)[idx].reshape(P * Cc, ld).contiguous()
            ops.attention_f8(q8, o_m, [own, garment(k_m, vt_m)], HEADS, **kw)
            assert torch.isfinite(o_m).all() and torch.equal(o_i, o_m), (Nq, nkg, P, G, idx)
            if (P, G, idx) in MODULO:                    # ... and the shared segment's bits
                o_s = nan_out(B, Nq, Cc, dtype)
                ops.attention_f8(q8, o_s, [own, garment(k8b, vt8b, nb=G if G < P else 0)], HEADS, **kw)
                assert torch.equal(o_i, o_s), (Nq, nkg, P, G)
            if (P, G) == (2, 5):
                # attention, not merely equal: held to F8_SDPA_BAR (see there why not KTOL)
                q, k1, v1, k2, v2, _ = self_attn_operands(P, G, Nq, nkg, dtype, 5 * P + G)
                sp = lambda t: t.float().view(t.shape[0], t.shape[1], HEADS, 64).transpose(1, 2)
                z = torch.zeros(P, HEADS, nkg, 64, device=DEV)
                kk = torch.cat([sp(k1), torch.cat([z, sp(k2[idx])])], dim=2)
                vv = torch.cat([sp(v1), torch.cat([z, sp(v2[idx])])], dim=2)
                ref = F.scaled_dot_product_attention(sp(q), kk, vv).transpose(1, 2).reshape(B, Nq, Cc)
                err = ((o_i.float() - ref).abs().max() / ref.abs().max()).item()
                print(f"fp8 {dtype} Nq={Nq} nkg={nkg}: indexed against fp32 SDPA {err:.3e} (16-bit bar {KTOL[dtype]:.1e}, fp8 bar {F8_SDPA_BAR:.1e})")
                assert err <= F8_SDPA_BAR, err


@DTYPES
def test_null_tables_are_the_shared_rule_and_bad_combinations_are_refused(dtype, monkeypatch):
    """seg_index = {NULL, NULL} through the _indexed entry points gives the _shared / plain bits; a table with seg_nb = 0 and a table in CROSS
    mode are refused with an error code before any launch (the outputs stay as they were)."""
    from idm_vton_amd import ffi, ops
    P, G, (Nq, nkg) = 4, 2, SHAPES[0]
    B, Cc = 2 * P, HEADS * 64
    qq, own, garment, (_, _, k2, _, vt2) = _segments16(P, G, Nq, nkg, dtype, 3, True)
    q8, own8, garment8, k8b, vt8b = _segments8(P, G, Nq, nkg, dtype, 3)
    kw8 = dict(qk_scale_exp=-4, v_scale_exp=-2, B=B, Nq=Nq, ldq=Cc, ldo=Cc)
    calls, outs = [], {}
    real = ffi.call_indexed
    monkeypatch.setattr(ops.ffi, "call_indexed", lambda fn, a, nb, ix, st: (calls.append((fn, list(nb), list(ix))), real(fn, a, nb, ix, st))[1])
    for form in ("shared", "null_tables"):
        if form == "null_tables":
            monkeypatch.setattr(ops, "_seg_index", lambda segs, B: [0, 0])
        for nb in (G, 0):
            gk, gv = (k2, vt2) if nb else (k2.repeat(2, 1, 1).contiguous(), vt2.repeat(2, 1, 1).contiguous())
            for name, tune in TUNES.items():
                o = nan_out(B, Nq, Cc, dtype)
                ops.attention(qq, o, [own, garment(gk, gv, nb=nb)], HEADS, tune=tune, q_prescaled=True)
                outs[(form, nb, name)] = o
            g8k, g8v = (k8b, vt8b) if nb else (k8b.repeat(2, 1).contiguous(), vt8b.repeat(2, 1).contiguous())
            o = nan_out(B, Nq, Cc, dtype)
            ops.attention_f8(q8, o, [own8, garment8(g8k, g8v, nb=nb)], HEADS, **kw8)
            outs[(form, nb, "f8")] = o
        assert len(calls) == (0 if form == "shared" else 2 * (len(TUNES) + 1))
    assert {fn for fn, _, _ in calls} == {"idmvton_attn_fwd_indexed", "idmvton_attn_f8_indexed"} and all(ix == [0, 0] for _, _, ix in calls)
    for nb in (G, 0):
        for name in list(TUNES) + ["f8"]:
            assert torch.isfinite(outs[("shared", nb, name)]).all() and torch.equal(outs[("shared", nb, name)], outs[("null_tables", nb, name)]), (nb, name)
    monkeypatch.undo()
    # refusals: nothing is launched, so the output keeps its NaN fill
    o = nan_out(B, Nq, Cc, dtype)
    t = int_table([0, 1, 0, 1])
    with pytest.raises(ValueError, match="needs nb="):
        ops.attention(qq, o, [own, garment(k2, vt2, index=t)], HEADS, q_prescaled=True)
    with pytest.raises(ValueError, match="int32 device tensor of B - b0 = 4 entries"):
        ops.attention(qq, o, [own, garment(k2, vt2, nb=G, index=int_table([0, 1]))], HEADS, q_prescaled=True)
    monkeypatch.setattr(ops, "_seg_nb", lambda segs: [0, 0])                               # past the host op's own check: the C entry points'
    with pytest.raises(RuntimeError, match=r"idmvton_attn_fwd_indexed failed \(-1\).*needs seg_nb >= 1 \(0\)"):
        ops.attention(qq, o, [own, garment(k2, vt2, nb=G, index=t)], HEADS, q_prescaled=True)
    with pytest.raises(RuntimeError, match=r"idmvton_attn_f8_indexed failed \(-1\).*needs seg_nb >= 1 \(0\)"):
        ops.attention_f8(q8, o, [own8, garment8(k8b, vt8b, nb=G, index=t)], HEADS, **kw8)
    monkeypatch.undo()
    q2 = qq[:, :, :Cc].contiguous()
    ctx = dict(k=k2.repeat(4, 1, 1).contiguous(), vt=vt2.repeat(4, 1, 1).contiguous(), nk=nkg, ldk=Cc, ldvt=vt2.shape[-1])
    with pytest.raises(RuntimeError, match=r"idmvton_attn_fwd_indexed failed \(-5\).*CROSS mode takes no table"):
        ops.attention(q2, o, [ctx, dict(ctx, nb=1, index=int_table(list(range(B))))], HEADS, mode=ffi.ATTN_CROSS)
    torch.cuda.synchronize()
    assert torch.isnan(o).all()


# ------------------------------------------------------------------------------------------------------------------ engine


@pytest.mark.parametrize("scheduler", ["ddpm", "ddim"])
@DTYPES
def test_indexed_call_equals_the_call_on_the_selected_cache(dtype, scheduler):
    """P = 4 persons on a G = 3 cache, garment_index = [2, 0, 2, 1], 4 steps (blocks of 1, 2, 1 timesteps), against the same call on
    cache.select([2, 0, 2, 1]) (G = P, no index): every execution form, and under on_step."""
    steps = 4
    eng, inp, _ = engine_inputs(dtype, 4, steps)
    cache = eng.encode_garment(num_inference_steps=steps, scheduler=scheduler, **garment_kw(inp, 3))
    sel = cache.select(IDX)
    assert (cache.G, sel.G) == (3, 4)
    base = base_call(inp, steps, scheduler)
    for form in FORMS:
        lat_i, lat_s = run_on(eng, base, cache, form, IDX), run_on(eng, base, sel, form)
        print(f"{dtype} {scheduler} {form}: max|indexed - selected| = {(lat_i - lat_s).abs().max().item():.3e}")
        assert torch.isfinite(lat_s).all() and torch.equal(lat_i, lat_s), (form, (lat_i - lat_s).abs().max().item())
    # and the index is read: another assignment gives other latents
    assert not torch.equal(run_on(eng, base, cache, "serial_eager", [0, 0, 0, 0]), lat_s)


def test_indexed_call_equals_the_selected_cache_with_fp8_attention():
    steps = 3
    eng, inp, _ = engine_inputs(torch.float16, 4, steps, fp8=True)
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp, 3))
    assert cache.attn_fp8 and {k.dtype for k, _ in cache.kv} == {torch.uint8, torch.float16}    # both routes: e4m3 from the projection, quantised per launch
    sel, base = cache.select(IDX), base_call(inp, steps)
    for form in FORMS:
        lat_i, lat_s = run_on(eng, base, cache, form, IDX), run_on(eng, base, sel, form)
        assert torch.isfinite(lat_s).all() and torch.equal(lat_i, lat_s), form


def test_indexed_call_equals_the_selected_cache_with_a_garment_of_another_size():
    """Person 128x128, cloth 64x96: the garment segment has its own token count at both levels."""
    steps = 3
    eng, inp, _ = engine_inputs(torch.float16, 4, steps)
    g = torch.Generator().manual_seed(21)
    cloth, nz = torch.randn(3, 3, 64, 96, generator=g).clamp(-1, 1), torch.randn(3, 4, 8, 12, generator=g)
    cache = eng.encode_garment(cloth=cloth, text_embeds_cloth=inp["text_embeds_cloth"][:3], noise_cloth=nz, num_inference_steps=steps, height=128, width=128)
    assert (cache.gh, cache.gw, cache.h, cache.w) == (8, 12, 16, 16)
    sel, base = cache.select(IDX), base_call(inp, steps)
    for form in FORMS:
        lat_i, lat_s = run_on(eng, base, cache, form, IDX), run_on(eng, base, sel, form)
        assert torch.isfinite(lat_s).all() and torch.equal(lat_i, lat_s), form


def test_unet_forward_takes_the_table_on_the_garment_feats_route():
    """HipUNet.forward(garment_feats=..., garment_index=...): the per-launch projection route of _block, against the features gathered by hand."""
    from tests import parity_utils as pu
    dtype, P, G = torch.float16, 3, 2
    m = model(dtype)
    t, g = m["product"][0], m["product"][1]
    inp = pu.make_inputs(P, 128, 128, m["xd"], m["pooled"], m["enc_dim"], 1, dtype)
    h = w = 16
    gen = torch.Generator().manual_seed(3)
    xg = torch.zeros(G, h * w, g.cin_pad, dtype=dtype, device=DEV)
    xg[..., :4] = torch.randn(G, h * w, 4, generator=gen).to(DEV, dtype)
    _, feats = g.forward(xg, g.time_embeddings([500], G)[0], g.encode_context(inp["text_embeds_cloth"][:G].to(DEV)), G, h, w)
    x = torch.zeros(2 * P, h * w, t.cin_pad, dtype=dtype, device=DEV)
    x[..., :13] = torch.randn(2 * P, h * w, 13, generator=gen).to(DEV, dtype)
    pe = torch.cat([inp["negative_prompt_embeds"], inp["prompt_embeds"]]).to(DEV)
    add = torch.cat([inp["negative_pooled_prompt_embeds"], inp["pooled_prompt_embeds"]]).to(DEV)
    ids = torch.tensor([[128, 128, 0, 0, 128, 128]], dtype=torch.float32, device=DEV).repeat(2 * P, 1)
    ctx = t.encode_context(pe, m["product"][3](inp["ip_hidden_states"].to(DEV)))
    temb = t.time_embeddings([500], 2 * P, dict(text_embeds=add, time_ids=ids))[0]
    idx = [1, 0, 1]
    e_i, _ = t.forward(x, temb, ctx, 2 * P, h, w, garment_feats=feats, garment_index=int_table(idx))
    e_m, _ = t.forward(x, temb, ctx, 2 * P, h, w, garment_feats=[f[idx].contiguous() for f in feats])
    assert torch.isfinite(e_m).all() and torch.equal(e_i, e_m)


def test_two_graph_calls_with_different_indices_and_a_garment_swapped_in_place():
    """One engine, one captured graph set: calls of one shape with different indices each equal their own reference (an index baked into a
    capture would repeat the first), also after cache.put(1, other) between them -- with no GarmentNet batch and no new graph state."""
    from idm_vton_amd.garment_cache import GarmentCache
    steps = 3
    eng, inp, _ = engine_inputs(torch.float16, 4, steps)
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp, 3))
    other = eng.encode_garment(num_inference_steps=steps, cloth=inp["cloth"][3:], text_embeds_cloth=inp["text_embeds_cloth"][3:], noise_cloth=inp["noise"]["cloth"][3:])
    swapped = GarmentCache.cat([cache.select([0]), other, cache.select([2])])                # what the pool holds after the put, built apart from it
    base = base_call(inp, steps)
    a, b = [2, 0, 2, 1], [1, 1, 0, 2]
    ref = {(name, tuple(i)): run_on(eng, base, c.select(i), "serial_eager") for name, c in (("before", cache), ("after", swapped)) for i in (a, b)}
    assert len({tuple(v.flatten().tolist()) for v in ref.values()}) == 4                    # four different results to tell apart
    n_garm = eng.stats["garment_batches"]
    for form in ("graph", "graph_overlap"):
        for i in (a, b, a):
            assert torch.equal(run_on(eng, base, cache, form, i), ref[("before", tuple(i))]), (form, i)
    states = len(eng._graphs)
    ptr = cache.kv[0][0].data_ptr()
    cache.put(1, other)
    assert cache.kv[0][0].data_ptr() == ptr
    for form in ("graph", "graph_overlap", "serial_eager"):
        for i in (a, b):
            assert torch.equal(run_on(eng, base, cache, form, i), ref[("after", tuple(i))]), (form, i)
    assert eng.stats["garment_batches"] == n_garm and len(eng._graphs) == states


def test_modulo_index_equals_the_call_without_an_index():
    steps = 3
    eng, inp, _ = engine_inputs(torch.bfloat16, 4, steps)
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp, 2))
    base = base_call(inp, steps)
    for form in ("serial_eager", "graph_overlap"):
        lat_i, lat_n = run_on(eng, base, cache, form, [0, 1, 0, 1]), run_on(eng, base, cache, form)
        assert torch.isfinite(lat_n).all() and torch.equal(lat_i, lat_n), form


def test_a_pool_larger_than_the_batch_fills_person_sized_sets():
    """G = 6 garments resident, P = 2 persons, graph form: the persistent sets have 2 slots per timestep, not 6, one fill per block, and
    pools of other sizes run through the same graph state."""
    steps = 3
    eng, inp, _ = engine_inputs(torch.float16, 2, steps)
    cache2 = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp))
    pool = cache2.repeat_garments(3)                                                       # g0 g1 g0 g1 g0 g1
    assert pool.G == 6
    base = base_call(inp, steps)
    ref = run_on(eng, base, pool.select([5, 2]), "serial_eager")
    n0 = eng.stats["garment_set_copies"]
    st = eng.prepare(**{**base, "cloth": pool, "garment_index": [5, 2]})
    lat = eng.denoise(st, **FORMS["graph_overlap"]).clone()
    assert torch.equal(lat, ref)
    assert eng.stats["garment_set_copies"] - n0 == len(st["blocks"]) + 1                  # one fill per block (+ the state's warm-up fill)
    keys = [k for k in eng._graphs if "indexed" in k]
    assert len(keys) == 1 and 6 not in keys[0][7:]
    state = eng._graphs[keys[0]]
    assert tuple(state["gix"].tolist()) == (0, 1) and state["gix"].dtype == torch.int32
    for fset in state["sets"]:
        for (k, vt), (pk, pvt) in zip(fset["kv"], pool.kv):
            N = pk.shape[0] // (steps * 6)
            assert vt.shape[0] == st["k"] * 2 and k.shape[0] == st["k"] * 2 * N, (tuple(k.shape), tuple(vt.shape))
    # the same state serves the 2-garment cache and another assignment; both persons on one garment use one slot
    assert torch.equal(run_on(eng, base, cache2, "graph_overlap", [1, 0]), ref)
    assert torch.equal(run_on(eng, base, pool, "graph_overlap", [3, 3]), run_on(eng, base, pool.select([3, 3]), "serial_eager"))
    assert tuple(state["gix"].tolist()) == (0, 0) and [k for k in eng._graphs if "indexed" in k] == keys


def _device_cache(G, seed, dtype=torch.float16):
    return pool_cache(G=G, seed=seed, dtype=dtype).to(DEV)


def test_host_offload_and_return_are_bit_equal_and_complete_on_return():
    """cache.to("cpu") hands back host tensors that may be read at once (no copy still in flight), pinned or not; take / put move one slot
    straight between the device and pinned host memory; save from the device and load to it round-trip."""
    import os
    import tempfile
    from idm_vton_amd.garment_cache import GarmentCache
    big = GarmentCache.cat([_device_cache(4, s) for s in range(8)])
    assert big.G == 32 and all(k.is_cuda for k, _ in big.kv)
    ref = [(k.clone(), vt.clone()) for k, vt in big.kv]
    host = big.to("cpu")                                                                   # unpinned: read immediately, no synchronize
    assert all(not k.is_cuda and torch.equal(k, rk.cpu()) and torch.equal(vt, rvt.cpu()) for (k, vt), (rk, rvt) in zip(host.kv, ref))
    pinned = big.to("cpu", pin_memory=True)
    assert all(k.is_pinned() and vt.is_pinned() for k, vt in pinned.kv) and same_values(pinned, host)
    for src in (host, pinned):
        back = src.to(DEV)
        assert all(k.is_cuda for k, _ in back.kv) and same_values(back, big)
    one = big.take(5, "cpu", pin_memory=True)
    assert one.G == 1 and all(k.is_pinned() for k, _ in one.kv) and same_values(one, host.select([5]))
    other = _device_cache(32, 77)
    other.put(9, one)                                                                      # pinned host -> one slot of a device cache
    assert same_values(other.select([9]), one) and same_values(other.select([8, 10]), _device_cache(32, 77).select([8, 10]))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "pool.safetensors")
        big.save(path)
        loaded = GarmentCache.load(path, device=DEV)
        assert all(k.is_cuda for k, _ in loaded.kv) and same_values(loaded, big) and (loaded.G, loaded.timesteps, loaded.weights_id) == (32, big.timesteps, "w0")


def test_pool_on_the_device_spills_to_pinned_host_memory_and_restores():
    from idm_vton_amd.garment_cache import GarmentPool
    truth = {key: _device_cache(1, 100 + key) for key in range(5)}
    made = []
    encode = lambda key: (made.append(key), truth[key])[1]
    pool = GarmentPool(2, like=truth[0], spill=2)
    ptr = pool.cache.kv[0][0].data_ptr()
    assert pool.get([1, 2, 1], encode) == [0, 1, 0]
    assert pool.get([3, 2], encode) == [0, 1] and list(pool.host) == [1] and all(k.is_pinned() for k, _ in pool.host[1].kv)
    assert same_values(pool.host[1], truth[1])
    assert pool.get([1, 4], encode) == [0, 1] and made == [1, 2, 3, 4]                     # 1 came back from the host: not encoded again
    assert list(pool.host) == [3, 2] and pool.stats == dict(hits=1, encoded=4, restored=1, evicted=3)   # bound 2: 1's copy, the oldest, was dropped
    for key, slot in pool.slots().items():
        assert same_values(pool.cache.select([slot]), truth[key]), key
    assert pool.cache.kv[0][0].data_ptr() == ptr and pool.cache.kv[0][0].is_cuda


def test_a_bad_index_is_refused_before_anything_is_launched():
    steps = 3
    eng, inp, _ = engine_inputs(torch.float16, 4, steps)
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp, 3))
    base = base_call(inp, steps)
    eng.denoise(eng.prepare(**{**base, "cloth": cache, "garment_index": IDX}), **FORMS["graph"])
    torch.cuda.synchronize()
    stats, graphs = dict(eng.stats), len(eng._graphs)
    launched = []
    from idm_vton_amd import ops
    real = ops._call
    ops._call = lambda *a, **kw: (launched.append(a[0]), real(*a, **kw))[1]
    try:
        with pytest.raises(ValueError, match="GarmentCache garment_index mismatch: 3 entries for P = 4 persons"):
            eng.prepare(**{**base, "cloth": cache, "garment_index": [0, 1, 2]})
        with pytest.raises(ValueError, match=r"GarmentCache garment_index mismatch: \[3\] outside \[0, G = 3\)"):
            eng.prepare(**{**base, "cloth": cache, "garment_index": [0, 1, 2, 3]})
        with pytest.raises(ValueError, match="garment_index names garments of a GarmentCache"):
            eng.prepare(**{**base, "cloth": inp["cloth"], "text_embeds_cloth": inp["text_embeds_cloth"], "noise": inp["noise"], "garment_index": IDX})
        with pytest.raises(ValueError, match="GarmentCache persons mismatch"):             # without an index the modulo rule stands
            eng.prepare(**{**base, "cloth": cache})
    finally:
        ops._call = real
    assert launched == [] and eng.stats == stats and len(eng._graphs) == graphs


# ------------------------------------------------------------------------------------------------------------------ boundary
def test_boundary_pipeline_passes_the_index_to_the_engine():
    DT = torch.float16
    pipe, enc, kw = boundary_pipeline(DT)
    B, H, W, steps = 3, 128, 128, 3
    inp, clip_pix, call = boundary_inputs(kw, B, H, W, steps, DT)
    cache = pipe.encode_garment(inp["cloth"][:2], inp["text_embeds_cloth"][:2], steps, H, W, generator=torch.Generator(DEV).manual_seed(11))
    idx = [1, 0, 1]                                                                # P = 3 persons on G = 2 garments
    eng = pipe.hip_engine()
    n_garm = eng.stats["garment_batches"]
    gen_c = torch.Generator(DEV).manual_seed(7)
    torch.manual_seed(123)                                                         # the pose posterior uses the GLOBAL generator
    img_c = pipe(generator=gen_c, cloth=cache, text_embeds_cloth=None, garment_index=idx, **call)[0]
    assert eng.stats["garment_batches"] == n_garm
    # the engine-level call on the draws of the reference's order: the cloth draw is made and dropped, index or not
    gen, noise = reference_draws(7, 123, B, H, W, steps, DT)
    ip = ip_states(enc, clip_pix)
    ref = engine_reference(eng, inp, noise, ip, steps, cloth=cache, garment_index=idx)
    assert torch.isfinite(img_c).all() and torch.equal(img_c, ref)
    assert torch.equal(gen_c.get_state(), gen.get_state())                         # every draw of the call was made
    with pytest.raises(ValueError, match="GarmentCache persons mismatch"):         # 3 persons on 2 garments needs the index
        pipe(generator=gen_c, cloth=cache, text_embeds_cloth=None, **call)
    with pytest.raises(ValueError, match="`garment_index` names garments of a GarmentCache"):
        pipe(generator=gen_c, cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"], garment_index=idx, **call)
