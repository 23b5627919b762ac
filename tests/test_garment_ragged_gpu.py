"""-m gpu: garments of several sizes in one pool.  Kernel level: the ragged key segment of idmvton_attn_fwd_ragged / idmvton_attn_f8_ragged
(query batch b has table[b] of the keys a slot holds) against the _indexed entry points at a launch-wide nk equal to each person's count --
same kernel, same grid, same tile walk, so EQUALITY, no tolerance -- with NaN wherever the header says a ragged launch does not look, and
against fp32 SDPA on per-person keys.  Engine level: persons wearing garments of three sizes in one call against the oracle run per person,
every execution form, one graph state across assignments and across a put that changes a slot's size, a slotted cache of equal sizes
against the plain cache, refusals, and the boundary pipeline.  No test hands a kernel a count outside [1, nk]: the kernels' clamp is a guard."""
import pytest
import torch
import torch.nn.functional as F

from tests.engine_support import (DEV, GARMENT_HW, STEPS, WEARS, H, W, base_call, boundary_inputs, boundary_pipeline, encode_three, engine, engine_reference,
                                  f8_operands, int_table, ip_states, model, nan_out, no_tune_table, oracle_latents, reference_draws, run_on,
                                  self_attn_operands, slotted_pool, three_garments)
from tests.garment_support import DTYPES, F8_SDPA_BAR, FORMS, HEADS
from tests.kernel_checks import TUNES

pytestmark = pytest.mark.gpu
CAP = 320                                                # keys a slot holds
# (P, G, index, slot lengths): lengths below / at / between tile multiples, one of a single partial tile, one shorter than 16; a slot (length
# 15) no person reads; two persons on one slot -- then a full and a 6-key slot -- then every length the capacity
PATTERNS = [(3, 4, [2, 0, 2], [48, 320, 200, 15]), (2, 2, [1, 0], [64, 6]), (2, 2, [0, 1], [CAP, CAP])]
NQS = [320, 256]                                         # 320 query rows are not a multiple of any kernel's 64 / 128 / 256 workgroup rows
E4M3_NAN = 0x7f


def _sp(t):
    return t.float().view(t.shape[0], t.shape[1], HEADS, 64).transpose(1, 2)


def _sdpa_per_person(q, k1, v1, k2, v2, idx, lens):
    """fp32 SDPA with per-person materialised keys: row i (unconditional) sees lens[idx[i]] zero keys, row P + i that garment's real ones."""
    P, out = len(idx), []
    for b in range(2 * P):
        i = b % P
        L = lens[idx[i]]
        kg, vg = _sp(k2[idx[i]:idx[i] + 1, :L]), _sp(v2[idx[i]:idx[i] + 1, :L])
        if b < P:
            kg, vg = torch.zeros_like(kg), torch.zeros_like(vg)
        kk, vv = torch.cat([_sp(k1[b:b + 1]), kg], dim=2), torch.cat([_sp(v1[b:b + 1]), vg], dim=2)
        out.append(F.scaled_dot_product_attention(_sp(q[b:b + 1]), kk, vv).transpose(1, 2).reshape(1, q.shape[1], HEADS * 64))
    return torch.cat(out)


def _ragged16(P, G, lens, Nq, dtype, seed, pres):
    """self_attn_operands with a garment segment of G slots of CAP keys; slot g holds lens[g] keys: its V^T is zero
    from there to round16 (the finite filler a real slot has there) and NaN beyond, its K rows NaN from lens[g] on."""
    from idm_vton_amd import ops
    q, k1, v1, k2, v2, ko = self_attn_operands(P, G, Nq, CAP, dtype, seed)
    qq = (q.float() * ops.QSCALE).to(dtype) if pres else q
    k2, v2 = k2.clone(), v2.clone()
    for g, L in enumerate(lens):
        v2[g, L:] = 0
    vt1, ld1 = ko(v1, Nq)
    vt2, ld2 = ko(v2, CAP)
    for g, L in enumerate(lens):
        k2[g, L:] = float("nan")
        vt2[g, :, ops.round16(L):] = float("nan")
    Cc = HEADS * 64
    own = dict(k=k1, vt=vt1, nk=Nq, ldk=Cc, ldvt=ld1)
    garment = lambda nk, **kw: dict(k=k2, vt=vt2, nk=nk, ldk=Cc, ldvt=ld2, k_rows=CAP, b0=P, nb=G, **kw)
    return q, qq, own, garment, (k1, v1, k2, v2)


@DTYPES
@pytest.mark.parametrize("tune", list(TUNES), ids=list(TUNES))
def test_ragged_segment_equals_the_indexed_launch_at_each_persons_count(tune, dtype, monkeypatch):
    no_tune_table(monkeypatch)
    from idm_vton_amd import ops
    from tests.kernel_checks import TOL as KTOL
    pres = tune != "auto"                                # kernels 3, 7, 8, 16 need a pre-multiplied q; `auto` runs the library's rule for a raw q
    for Nq in NQS:
        for P, G, idx, lens in PATTERNS:
            B, Cc = 2 * P, HEADS * 64
            q, qq, own, garment, (k1, v1, k2, v2) = _ragged16(P, G, lens, Nq, dtype, 17 * P + G, pres)
            per = [lens[g] for g in idx]
            o_r = nan_out(B, Nq, Cc, dtype)
            ops.attention(qq, o_r, [own, garment(CAP, index=int_table(idx), nk_table=int_table(per * 2))], HEADS, tune=TUNES[tune], q_prescaled=pres)
            assert torch.isfinite(o_r).all(), (tune, Nq, idx, lens)
            for i, L in enumerate(per):                  # the _indexed entry point, launch-wide nk = this person's count, same strides, same tune
                o_i = nan_out(B, Nq, Cc, dtype)
                ops.attention(qq, o_i, [own, garment(L, index=int_table(idx))], HEADS, tune=TUNES[tune], q_prescaled=pres)
                for b in (i, P + i):
                    assert torch.equal(o_r[b], o_i[b]), (tune, Nq, idx, lens, b, (o_r[b].float() - o_i[b].float()).abs().max().item())
            if P == 3:                                   # the values are attention, not merely equal
                ref = _sdpa_per_person(qq.float() / (ops.QSCALE if pres else 1.0), k1, v1, k2, v2, idx, lens)
                err = ((o_r.float() - ref).abs().max() / ref.abs().max()).item()
                print(f"{tune} {dtype} Nq={Nq}: ragged against fp32 SDPA {err:.3e} (bar {KTOL[dtype]:.1e})")
                assert err <= KTOL[dtype], (tune, err)  # the bar tests/kernel_checks.py holds check_attn_self to (imported)


def _ragged8(P, G, lens, Nq, dtype, seed):
    """f8_operands with slot lengths: the garment V^T bytes are zero at the positions of keys >= lens[g] inside the last tile and e4m3 NaN from
    roundup64(lens[g]) on, the K rows e4m3 NaN from lens[g] on."""
    q8, (k8a, vt8a), (k8b, vt8b) = f8_operands(P, G, Nq, CAP, dtype, seed)
    Cc, ld = HEADS * 64, vt8b.shape[1]
    k8b, vt8b = k8b.clone().view(G, CAP, Cc), vt8b.clone().view(G, Cc, ld)
    pos = torch.arange(ld, device=DEV)
    key = (pos & ~63) | (((pos >> 4) & 1) << 5) | (((pos >> 2) & 3) << 3) | (((pos >> 5) & 1) << 2) | (pos & 3)      # the key a position holds
    for g, L in enumerate(lens):
        k8b[g, L:] = E4M3_NAN
        vt8b[g][:, key >= L] = 0
        vt8b[g][:, (L + 63) // 64 * 64:] = E4M3_NAN
    own = dict(k8=k8a, vt8=vt8a, nk=Nq, ldk=Cc, ldvt=vt8a.shape[1])
    garment = lambda nk, **kw: dict(k8=k8b.view(G * CAP, Cc), vt8=vt8b.view(G * Cc, ld), nk=nk, ldk=Cc, ldvt=ld, k_rows=CAP, b0=P, nb=G, **kw)
    return q8, own, garment


@DTYPES
def test_ragged_segment_equals_the_indexed_launch_at_each_persons_count_fp8(dtype):
    from idm_vton_amd import ops
    for Nq in NQS:
        for P, G, idx, lens in PATTERNS:
            B, Cc = 2 * P, HEADS * 64
            q8, own, garment = _ragged8(P, G, lens, Nq, dtype, 5 * P + G)
            kw = dict(qk_scale_exp=-4, v_scale_exp=-2, B=B, Nq=Nq, ldq=Cc, ldo=Cc)
            per = [lens[g] for g in idx]
            o_r = nan_out(B, Nq, Cc, dtype)
            ops.attention_f8(q8, o_r, [own, garment(CAP, index=int_table(idx), nk_table=int_table(per * 2))], HEADS, **kw)
            assert torch.isfinite(o_r).all(), (Nq, idx, lens)
            for i, L in enumerate(per):
                o_i = nan_out(B, Nq, Cc, dtype)
                ops.attention_f8(q8, o_i, [own, garment(L, index=int_table(idx))], HEADS, **kw)
                for b in (i, P + i):
                    assert torch.equal(o_r[b], o_i[b]), (Nq, idx, lens, b)
            if P == 3:                                   # held to F8_SDPA_BAR, the bar the header states for this kernel (see there why not TOL)
                q, k1, v1, k2, v2, _ = self_attn_operands(P, G, Nq, CAP, dtype, 5 * P + G)
                ref = _sdpa_per_person(q, k1, v1, k2, v2, idx, lens)
                err = ((o_r.float() - ref).abs().max() / ref.abs().max()).item()
                print(f"fp8 {dtype} Nq={Nq}: ragged against fp32 SDPA {err:.3e} (fp8 bar {F8_SDPA_BAR:.1e})")
                assert err <= F8_SDPA_BAR, err


@DTYPES
def test_capacity_tables_and_null_tables_are_the_indexed_launch(dtype, monkeypatch):
    """A table that holds the capacity for every batch, and {NULL, NULL} through the _ragged entry points, give the _indexed launch's bits,
    in every kernel; without nk_table nothing goes through _ragged."""
    from idm_vton_amd import ffi, ops
    no_tune_table(monkeypatch)
    P, G, idx, lens = PATTERNS[2]
    Nq, B, Cc = NQS[0], 2 * P, HEADS * 64
    kw8 = dict(qk_scale_exp=-4, v_scale_exp=-2, B=B, Nq=Nq, ldq=Cc, ldo=Cc)
    _, qq, own, garment, _ = _ragged16(P, G, lens, Nq, dtype, 23, True)
    q8, own8, garment8 = _ragged8(P, G, lens, Nq, dtype, 23)
    calls = []
    real = ffi.call_ragged
    monkeypatch.setattr(ops.ffi, "call_ragged", lambda fn, a, nb, ix, nk, st: (calls.append((fn, list(nk))), real(fn, a, nb, ix, nk, st))[1])

    def launch(**seg_kw):
        outs = {}
        for name, tune in TUNES.items():
            outs[name] = nan_out(B, Nq, Cc, dtype)
            ops.attention(qq, outs[name], [own, garment(CAP, index=int_table(idx), **seg_kw)], HEADS, tune=tune, q_prescaled=True)
        outs["f8"] = nan_out(B, Nq, Cc, dtype)
        ops.attention_f8(q8, outs["f8"], [own8, garment8(CAP, index=int_table(idx), **seg_kw)], HEADS, **kw8)
        return outs
    indexed = launch()
    assert calls == []
    full = launch(nk_table=int_table([CAP] * B))
    assert len(calls) == len(TUNES) + 1 and all(nk[0] == 0 and nk[1] != 0 for _, nk in calls)
    monkeypatch.setattr(ops, "_seg_nk", lambda segs, B: [0, 0])
    null = launch()
    assert len(calls) == 2 * (len(TUNES) + 1) and {fn for fn, _ in calls} == {"idmvton_attn_fwd_ragged", "idmvton_attn_f8_ragged"}
    for name in indexed:
        assert torch.isfinite(indexed[name]).all() and torch.equal(full[name], indexed[name]) and torch.equal(null[name], indexed[name]), name
    monkeypatch.undo()
    o = nan_out(B, Nq, Cc, dtype)                           # refusals: nothing is launched, so the output keeps its NaN fill
    with pytest.raises(ValueError, match="nk_table must be a contiguous int32 device tensor of B = 4 entries"):
        ops.attention(qq, o, [own, garment(CAP, index=int_table(idx), nk_table=int_table([CAP] * P))], HEADS, q_prescaled=True)
    with pytest.raises(ValueError, match="nk_table must be a contiguous int32 device tensor of B = 4 entries"):
        ops.attention_f8(q8, o, [own8, garment8(CAP, nk_table=torch.full((B,), CAP, device=DEV))], HEADS, **kw8)
    torch.cuda.synchronize()
    assert torch.isnan(o).all()


# ------------------------------------------------------------------------------------------------------------------ engine


@DTYPES
def test_persons_wearing_garments_of_three_sizes_match_the_oracle_per_person(dtype):
    from tests import parity_utils as pu
    from tests.parity_checks import TOL
    m = model(dtype)
    eng = engine(m, dtype)
    inp, garments = three_garments(dtype)
    ones = encode_three(eng, garments)
    pool = slotted_pool(eng, ones)
    assert pool.sizes == [(8, 12), (16, 16), (9, 5)] and (pool.gh, pool.gw) == (16, 16)
    # the analytic slot shapes are those of a garment encoded at the slot's size
    assert [(tuple(k.shape), tuple(vt.shape)) for k, vt in pool.select([1]).kv] == [(tuple(k.shape), tuple(vt.shape)) for k, vt in ones[1].kv]
    st = eng.prepare(**{**base_call(inp, STEPS), "cloth": pool, "garment_index": WEARS})
    tokens = [m["product"][0].feature_tokens(*pool.sizes[g]) for g in WEARS]
    assert st["gnk"].dtype == torch.int32 and st["gnk"].tolist() == [[t[f] for t in tokens] * 2 for f in range(len(tokens[0]))]
    lat = eng.denoise(st)
    for i, ref in enumerate(oracle_latents(dtype)):
        err = pu.relerr(lat[i:i + 1], ref)
        print(f"{dtype} person {i} in garment {WEARS[i]} ({GARMENT_HW[WEARS[i]]}): latents against the oracle {err:.3e} (bar {TOL[dtype]['latents']:.1e})")
        assert err <= TOL[dtype]["latents"], (i, err)


def test_three_sizes_with_fp8_attention_match_the_oracle_within_the_variants_tolerance():
    """The fp8-attention engine at the 8e-2 of test_fp8_attention_engine_matches_oracle_within_its_stated_tolerance.  Garment B has features
    whose token rows are whole 64-key tiles: the fused projection wrote them as e4m3, `put` widens them into the 16-bit slot, and the
    per-launch quantisation must give the projection's values back."""
    from idm_vton_amd import ops
    from idm_vton_amd.garment_cache import widen_f8
    from tests import parity_utils as pu
    dtype = torch.float16
    eng = engine(model(dtype, True), dtype)
    inp, garments = three_garments(dtype)
    ones = encode_three(eng, garments)
    assert {k.dtype for k, _ in ones[1].kv} == {torch.uint8, torch.float16} and {k.dtype for k, _ in ones[0].kv} == {torch.float16}
    _, ek, ev = eng.unet.f8_exp
    k8, vt8 = next((k, vt) for k, vt in ones[1].kv if k.dtype == torch.uint8)
    k16, vt16 = widen_f8(k8, vt8, dtype, ek, ev)
    f8 = lambda t: t.view(torch.float8_e4m3fn).float()
    assert torch.equal(f8(ops.quant_f8(k16, 2.0 ** ek)), f8(k8))
    assert torch.equal(f8(ops.quant_f8(vt16.reshape(-1, vt16.shape[-1]), 2.0 ** ev, mode=1)), f8(vt8.reshape(-1, vt8.shape[-1])))
    pool = slotted_pool(eng, ones)
    assert {k.dtype for k, _ in pool.kv} == {torch.float16}
    lat = run_on(eng, base_call(inp, STEPS), pool, "serial_eager", WEARS)
    for i, ref in enumerate(oracle_latents(dtype)):
        err = pu.relerr(lat[i:i + 1], ref)
        print(f"fp8 attention, person {i} in garment {WEARS[i]}: latents against the oracle {err:.3e} (bar 8.0e-02)")
        assert err <= 8e-2, (i, err)
    assert torch.equal(run_on(eng, base_call(inp, STEPS), pool, "graph_overlap", WEARS), lat)


@DTYPES
def test_every_execution_form_gives_the_bits_of_serial_eager_for_a_ragged_call(dtype):
    eng = engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    pool = slotted_pool(eng, encode_three(eng, garments))
    base = base_call(inp, STEPS)
    ref = run_on(eng, base, pool, "serial_eager", WEARS)
    assert torch.isfinite(ref).all()
    for form in FORMS:
        assert torch.equal(run_on(eng, base, pool, form, WEARS), ref), form
    assert not torch.equal(run_on(eng, base, pool, "serial_eager", [0, 0, 0]), ref)          # and the assignment is read


def test_one_graph_state_serves_every_assignment_and_a_put_that_changes_a_slots_size():
    dtype = torch.float16
    eng = engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    ones = encode_three(eng, garments)
    pool = slotted_pool(eng, ones)
    base = base_call(inp, STEPS)
    n_garm = eng.stats["garment_batches"]
    smallest = [2, 2, 2]                                 # every person in the 9x5 garment
    assign = [WEARS, smallest, [1, 1, 0]]
    ref = {tuple(a): run_on(eng, base, pool, "serial_eager", a) for a in assign}
    assert len({tuple(v.flatten().tolist()) for v in ref.values()}) == len(assign)
    for form in ("graph", "graph_overlap"):
        for a in assign + [WEARS]:
            assert torch.equal(run_on(eng, base, pool, form, a), ref[tuple(a)]), (form, a)
    states = [k for k in eng._graphs if "ragged" in k]
    assert len(states) == 1 and len(eng._graphs) == 1
    ptr = pool.kv[0][0].data_ptr()
    pool.put(1, ones[2])                                 # the slot of the largest garment now holds the smallest
    assert pool.sizes == [(8, 12), (9, 5), (9, 5)] and pool.kv[0][0].data_ptr() == ptr
    after = {tuple(a): run_on(eng, base, pool, "serial_eager", a) for a in (WEARS, [1, 1, 0])}
    assert torch.equal(run_on(eng, base, pool, "serial_eager", [1, 1, 1]), ref[tuple(smallest)])    # slot 1 IS garment C now
    assert not torch.equal(after[tuple(WEARS)], ref[tuple(WEARS)])
    for form in ("graph", "graph_overlap"):
        for a in (WEARS, [1, 1, 0]):
            assert torch.equal(run_on(eng, base, pool, form, a), after[tuple(a)]), (form, a)
    assert eng.stats["garment_batches"] == n_garm and list(eng._graphs) == states


@DTYPES
def test_a_slotted_cache_of_equal_sizes_gives_the_bits_of_the_plain_cache(dtype, monkeypatch):
    from idm_vton_amd import ffi, ops
    eng = engine(model(dtype), dtype)
    inp, _ = three_garments(dtype)
    plain = eng.encode_garment(num_inference_steps=STEPS, cloth=inp["cloth"], text_embeds_cloth=inp["text_embeds_cloth"], noise_cloth=inp["noise"]["cloth"])
    pool = slotted_pool(eng, [plain.select([g]) for g in range(3)])
    assert pool.sizes == [(16, 16)] * 3 and plain.sizes is None and pool.rows == [None] * 3
    ragged = []
    real = ffi.call_ragged
    monkeypatch.setattr(ops.ffi, "call_ragged", lambda fn, *a: (ragged.append(fn), real(fn, *a))[1])
    base = base_call(inp, STEPS)
    for form in ("serial_eager", "graph_overlap"):
        lat_p = run_on(eng, base, plain, form, WEARS)
        assert ragged == []                              # a plain cache: through _indexed, no table
        lat_s = run_on(eng, base, pool, form, WEARS)
        assert len(ragged) > 0 and set(ragged) == {"idmvton_attn_fwd_ragged"}
        assert torch.isfinite(lat_p).all() and torch.equal(lat_s, lat_p), form
        del ragged[:]
    assert len([k for k in eng._graphs if "ragged" in k]) == 1 and len(eng._graphs) == 2   # ragged and plain states are told apart


def test_refusals_come_before_anything_is_launched():
    from idm_vton_amd import ops
    dtype = torch.float16
    eng = engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    ones = encode_three(eng, garments, which=(0, 1))
    pool = slotted_pool(eng, [ones[0]] * 3)
    torch.cuda.synchronize()
    launched = []
    real = ops._call
    ops._call = lambda *a, **kw: (launched.append(a[0]), real(*a, **kw))[1]
    try:
        with pytest.raises(ValueError, match="holds garments of several sizes: pass garment_index"):
            eng.prepare(**{**base_call(inp, STEPS), "cloth": pool})
        small = eng.empty_garment_cache(1, 64, 96, STEPS, height=H, width=W)
        with pytest.raises(ValueError, match="put: does not fit"):
            small.put(0, ones[1])                        # 128x128 into a 64x96 slot
        with pytest.raises(ValueError, match="divisible by 8"):
            eng.empty_garment_cache(1, 60, 96, STEPS)
    finally:
        ops._call = real
    assert launched == [] and small.sizes == [(8, 12)]


# ------------------------------------------------------------------------------------------------------------------ boundary
def test_boundary_pipeline_passes_a_slotted_pool_through():
    from idm_vton_amd.garment_cache import GarmentPool
    DT = torch.float16
    pipe, enc, kw = boundary_pipeline(DT)
    B, steps = 3, 3
    inp, clip_pix, call = boundary_inputs(kw, B, H, W, steps, DT)
    small = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(13)).clamp(-1, 1)
    cloths = {"small": (small, inp["text_embeds_cloth"][:1]), "full": (inp["cloth"][1:2], inp["text_embeds_cloth"][1:2])}
    encode = lambda key: pipe.encode_garment(cloths[key][0], cloths[key][1], steps, H, W, generator=torch.Generator(DEV).manual_seed(11))
    pool = GarmentPool(2, like=pipe.empty_garment_cache(1, H, W, steps), mixed_sizes=True)
    idx = pool.get(["full", "small", "full"], encode)
    assert idx == [0, 1, 0] and pool.cache.sizes == [(16, 16), (8, 12)]
    eng = pipe.hip_engine()
    n_garm = eng.stats["garment_batches"]
    gen_c = torch.Generator(DEV).manual_seed(7)
    torch.manual_seed(123)                                                         # the pose posterior uses the GLOBAL generator
    img_c = pipe(generator=gen_c, cloth=pool.cache, text_embeds_cloth=None, garment_index=idx, **call)[0]
    assert eng.stats["garment_batches"] == n_garm
    # the engine-level call on the draws of the reference's order: the cloth draw (of the slot's latent size) is made and dropped
    _, noise = reference_draws(7, 123, B, H, W, steps, DT)
    ip = ip_states(enc, clip_pix)
    ref = engine_reference(eng, inp, noise, ip, steps, cloth=pool.cache, garment_index=idx)
    assert torch.isfinite(img_c).all() and torch.equal(img_c, ref)
    with pytest.raises(ValueError, match="holds garments of several sizes: pass garment_index"):
        pipe(generator=gen_c, cloth=pool.cache, text_embeds_cloth=None, **call)
