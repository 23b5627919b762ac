"""-m gpu: the garment shelf on the GPU.  Kernel level: idmvton_kv_fill on framed operands (tests/frames.py) -- data runs from page-locked host
memory against the torch definition of the packed format (widening) or the source bits (copying), ZERO runs against the bits 0x0000, both
kinds in one table and into one destination (a compact run in front, the zero tail behind it), bit for bit.  Engine level: a call on a
ShelvedGarmentCache -- compact garments of three sizes in pinned host memory -- against the same call on slotted("cuda"), the device-resident
slotted cache the same garments give: the sets receive the same bits, so EQUALITY in every execution form, no tolerance; slot reuse through one
graph state; the refusals; the boundary pipeline.  A chunk is 1024 16-byte items: the shapes are the smallest that cross one."""
import pytest
import torch

from tests.engine_support import (DEV, KEYS, MIXED_DSTS, MIXED_RUNS, STEPS, WEARS, H, W, base_call, boundary_inputs, boundary_pipeline, check_fill, e4m3_bytes,
                                  encode_three, engine, engine_reference, gpu_shelf, ip_states, model, pin_frame, reference_draws, run_on, three_garments)
from tests.garment_support import DTYPES, FORMS

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ kernel


def _fill(dsts, runs, dtype, workgroups, copy=False, on_device=()):
    """Framed destinations on the device, framed sources (and one exponent per data run) in pinned host memory -- runs whose number is in
    `on_device`: in device memory --, ONE idmvton_kv_fill launch of `workgroups` workgroups.  -> (destinations, sources by run, values by run,
    table)."""
    from idm_vton_amd import ffi, ops
    from tests import frames
    outs = [frames.framed_out((r, w), dtype, DEV, ld) for r, w, ld in dsts]
    exps_h = torch.tensor([run[4] if run[0] == "d" else 0 for run in runs], dtype=torch.int32).pin_memory()
    exps_d = exps_h.to(DEV)
    srcs, vals, descs = {}, {}, []
    for i, run in enumerate(runs):
        if run[0] == "z":
            _, rows, cols, d, c0 = run
            descs.append((None, outs[d][:rows, c0:c0 + cols], None))
            continue
        _, rows, cols, lds, e, d, c0 = run
        x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(i)).to(dtype) if copy else e4m3_bytes(rows, cols, seed=i)
        s = frames.framed(x.to(DEV), lds) if i in on_device else pin_frame(frames.framed(x, lds))
        srcs[i], vals[i] = s, x
        descs.append((s, outs[d][:rows, c0:c0 + cols], None if copy else (exps_d if i in on_device else exps_h)[i:i + 1]))
    table = ops.kv_fill(descs, dtype, mode=ffi.KVS_COPY if copy else ffi.KVS_WIDEN_E4M3, workgroups=workgroups)
    torch.cuda.synchronize()
    return outs, srcs, vals, table


@DTYPES
@pytest.mark.parametrize("workgroups", [1, 3, 16])
def test_kv_fill_widens_data_runs_and_writes_zero_runs_in_one_table(dtype, workgroups):
    """Six chunks (1, 1, 2, 2).  One workgroup walks data and zero chunks alternately through both register sets; with 16, ten are idle."""
    outs, srcs, vals, table = _fill(MIXED_DSTS, MIXED_RUNS, dtype, workgroups)
    assert table.ENTRY == "kv_fill" and table.items.tolist() == [15, 20, 1120, 1056] and table.first_host.tolist() == [0, 1, 2, 4, 6]
    assert table.host[:, 0].ne(0).tolist() == [True, False, True, False] and table.host[1, 2] == 0
    assert all(not s.is_cuda and s.is_pinned() for s in srcs.values())
    assert table.link_bytes() == 16.0 * (15 + 1120)
    check_fill(MIXED_DSTS, MIXED_RUNS, outs, srcs, vals, dtype)


ORDERINGS = {"zdz": "zdz", "dzd": "dzd", "zdzd": "zdzd", "zzz": "zzz"}


@pytest.mark.parametrize("order", list(ORDERINGS), ids=list(ORDERINGS))
def test_kv_fill_orderings_of_single_chunk_runs_with_one_workgroup(order):
    """The prologue on a zero chunk, both arms of the loop's tail, odd and even chunk counts -- and a table of zero runs only, whose src and
    exp are NULL."""
    dtype = torch.float16
    dsts, runs = [], []
    for i, kind in enumerate(ORDERINGS[order]):
        if kind == "d":
            dsts.append((9 + i, 80, 88)); runs.append(("d", 9 + i, 80, 96, i - 2, i, 0))
        else:
            dsts.append((7 + i, 48, 56)); runs.append(("z", 7 + i, 48, i, 0))
    outs, srcs, vals, table = _fill(dsts, runs, dtype, 1)
    assert table.first_host.tolist() == list(range(len(runs) + 1))
    if order == "zzz":
        assert not srcs and (table.host[:, 0] == 0).all() and (table.host[:, 2] == 0).all() and table.link_bytes() == 0.0
    check_fill(dsts, runs, outs, srcs, vals, dtype)


@DTYPES
@pytest.mark.parametrize("workgroups", [1, 3, 16])
def test_kv_fill_copy_mode(dtype, workgroups):
    """The same table with 16-bit sources in pinned memory: byte units (30, 40, 2240 and 2112 items), zero BYTES."""
    outs, srcs, vals, table = _fill(MIXED_DSTS, MIXED_RUNS, dtype, workgroups, copy=True)
    assert table.items.tolist() == [30, 40, 2240, 2112] and table.first_host.tolist() == [0, 1, 2, 5, 8]
    check_fill(MIXED_DSTS, MIXED_RUNS, outs, srcs, vals, dtype, copy=True)


def test_kv_fill_one_table_mixes_host_and_device_sources_with_zero_runs():
    outs, srcs, vals, _ = _fill(MIXED_DSTS, MIXED_RUNS, torch.bfloat16, 8, on_device=(2,))
    assert [srcs[i].is_cuda for i in sorted(srcs)] == [False, True]
    check_fill(MIXED_DSTS, MIXED_RUNS, outs, srcs, vals, torch.bfloat16)


def test_kv_fill_wrapper_refuses_a_malformed_run():
    from idm_vton_amd import ops
    d = torch.full((4, 32), float("nan"), dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match="kv_fill: a run is"):
        ops.kv_fill([(None, d.to(torch.bfloat16), None)], torch.float16)
    with pytest.raises(ValueError, match="pin_memory"):
        ops.kv_fill([(torch.zeros(4, 32, dtype=torch.uint8), d, torch.zeros(1, dtype=torch.int32).pin_memory())], torch.float16)
    with pytest.raises(RuntimeError, match=r"idmvton_kv_fill failed \(-1\).*cols=24"):
        ops.kv_fill([(None, d[:, :24], None)], torch.float16)
    torch.cuda.synchronize()
    assert torch.isnan(d).all()                          # nothing was launched


# ------------------------------------------------------------------------------------------------------------------ engine


def _against_the_slotted_device_cache(dtype, storage):
    eng = engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    shelf = gpu_shelf(eng, encode_three(eng, garments), storage)
    assert shelf.nbytes == sum(p.nbytes for p in shelf._parts.values()) < 3 * shelf._parts["g1"].nbytes       # compact: less than 3 slots
    shelved, index = shelf.get([KEYS[j] for j in WEARS])
    assert index == [0, 1, 2] and shelved.sizes == [(9, 5), (8, 12), (16, 16)] and shelved.packed == (storage == "e4m3") and shelved.host_resident
    device = shelved.slotted(DEV)
    assert device.sizes == shelved.sizes and not device.host_resident and not device.packed
    base = base_call(inp, STEPS)
    nblocks = len(eng._block_schedule(STEPS)[1])
    assert nblocks == 2
    for form in FORMS:                                   # (the device call first: a graph form's state then exists and must serve the shelved call)
        lat_d = run_on(eng, base, device, form, index)
        states, n0, c0 = len(eng._graphs), eng.stats["garment_stream_launches"], eng.stats["garment_set_copies"]
        lat_s = run_on(eng, base, shelved, form, index)
        assert torch.isfinite(lat_d).all() and torch.isfinite(lat_s).all(), form
        assert torch.equal(lat_s, lat_d), (form, (lat_s - lat_d).abs().max().item())
        assert eng.stats["garment_stream_launches"] - n0 == nblocks, form
        assert eng.stats["garment_set_copies"] == c0 and len(eng._graphs) == states, form
    assert not torch.equal(run_on(eng, base, shelved, "serial_eager", [0, 0, 1]), lat_d)        # and the assignment is read
    # the reverse: a state built by a shelved call serves the device-resident slotted cache
    fresh = engine(model(dtype), dtype)
    lat_s = run_on(fresh, base, shelved, "graph_overlap", index)
    states = len(fresh._graphs)
    assert torch.equal(run_on(fresh, base, device, "graph_overlap", index), lat_s) and len(fresh._graphs) == states == 1 and torch.equal(lat_s, lat_d)


@DTYPES
def test_packed_shelf_equals_the_slotted_device_call(dtype):
    _against_the_slotted_device_cache(dtype, "e4m3")


@DTYPES
def test_16bit_shelf_equals_the_slotted_device_call(dtype):
    _against_the_slotted_device_cache(dtype, "native")


def test_slot_reuse_through_one_graph_state():
    """Set slot 0 holds the largest garment, then the smallest (its zero tail has to replace the larger garment's values), then the call's
    three; a fourth call names a garment `get` has to encode.  Each against the slotted device call of that assignment."""
    dtype = torch.float16
    eng = engine(model(dtype), dtype)
    fresh = engine(model(dtype), dtype)                # the reference runs apart: its sets never held another garment
    inp, garments = three_garments(dtype)
    ones = encode_three(eng, garments)
    shelf = gpu_shelf(eng, ones[1:], "e4m3")                # g0 = ones[1] (16x16), g1 = ones[2] (9x5): KEYS[:2]
    base = base_call(inp, STEPS)
    encoded = []
    enc = lambda key: (encoded.append(key), ones[0])[1]
    for form in ("graph", "graph_overlap"):
        for keys in (["g0"] * 3, ["g1"] * 3, ["g1", "g0", "g1"], ["new", "g0", "new"]):
            shelved, index = shelf.get(keys, encode=enc)
            lat = run_on(eng, base, shelved, form, index)
            ref = run_on(fresh, base, shelved.slotted(DEV), "serial_eager", index)
            assert torch.isfinite(lat).all() and torch.equal(lat, ref), (form, keys, (lat - ref).abs().max().item())
    assert encoded == ["new"] and "new" in shelf and len(eng._graphs) == 1


def test_shelved_refusals_come_before_anything_is_launched():
    from idm_vton_amd import ops
    from idm_vton_amd.garment_cache import ShelvedGarmentCache
    dtype = torch.float16
    eng = engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    ones = encode_three(eng, garments, which=(0, 1))
    shelf = gpu_shelf(eng, ones, "e4m3")
    good, index = shelf.get(["g0", "g1", "g0"])
    base = base_call(inp, STEPS)
    torch.cuda.synchronize()
    stats, launched = dict(eng.stats), []
    real = ops._call
    ops._call = lambda *a, **kw: (launched.append(a[0]), real(*a, **kw))[1]
    try:
        p1 = good.parts[1]                               # a part built by hand: pageable bytes (a clone of a pinned tensor is pageable)
        pageable = ShelvedGarmentCache([good.parts[0], p1._like(kv=[(k.clone(), vt.clone()) for k, vt in p1.kv], exps=p1.exps)],
                                       gh=good.gh, gw=good.gw, slot_shapes=good.slot_shapes)
        assert not pageable.parts[1].kv[0][0].is_pinned()
        with pytest.raises(ValueError, match="kv mismatch.*pageable.*pin_memory"):
            eng.prepare(**{**base, "cloth": pageable, "garment_index": index})
        half = good.take(1, "cpu", pin_memory=True)
        half.exps = half.exps.clone()                    # pinned bytes, pageable exponents
        assert half.kv[0][0].is_pinned() and not half.exps.is_pinned()
        with pytest.raises(ValueError, match="exps mismatch.*pageable.*pin_memory"):
            eng.prepare(**{**base, "cloth": ShelvedGarmentCache([good.parts[0], half], gh=good.gh, gw=good.gw, slot_shapes=good.slot_shapes),
                           "garment_index": index})
        with pytest.raises(ValueError, match="holds garments of several sizes: pass garment_index"):
            eng.prepare(**{**base, "cloth": good})
    finally:
        ops._call = real
    assert eng.stats == stats and not eng._graphs and launched == []
    eng8 = engine(model(dtype, True), dtype)
    stats8 = dict(eng8.stats)
    with pytest.raises(ValueError, match="attn_fp8 mismatch"):
        eng8.prepare(**{**base, "cloth": good, "garment_index": index})
    good.attn_fp8 = True                                 # past `check`: the engine's own refusal of a host-resident cache
    with pytest.raises(ValueError, match="attn_fp8 mismatch.*does not stream"):
        eng8._check_host_cache(good)
    assert eng8.stats == stats8 and not eng8._graphs


# ------------------------------------------------------------------------------------------------------------------ boundary
def test_boundary_pipeline_passes_a_shelved_cache_through():
    from idm_vton_amd.garment_cache import GarmentShelf, ShelvedGarmentCache
    DT = torch.float16
    pipe, enc, kw = boundary_pipeline(DT)
    B, steps = 3, 3
    inp, clip_pix, call = boundary_inputs(kw, B, H, W, steps, DT)
    small = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(13)).clamp(-1, 1)
    cloths = {"small": (small, inp["text_embeds_cloth"][:1]), "full": (inp["cloth"][1:2], inp["text_embeds_cloth"][1:2])}
    encode = lambda key: pipe.encode_garment(cloths[key][0], cloths[key][1], steps, H, W, generator=torch.Generator(DEV).manual_seed(11))
    shelf = GarmentShelf(pipe.empty_garment_cache(1, H, W, steps), storage="e4m3")
    cache, idx = shelf.get(["full", "small", "full"], encode)
    assert isinstance(cache, ShelvedGarmentCache) and idx == [0, 1, 0] and cache.sizes == [(16, 16), (8, 12)]
    eng = pipe.hip_engine()
    n_garm, n0 = eng.stats["garment_batches"], eng.stats["garment_stream_launches"]
    gen_c = torch.Generator(DEV).manual_seed(7)
    torch.manual_seed(123)                                                         # the pose posterior uses the GLOBAL generator
    img_c = pipe(generator=gen_c, cloth=cache, text_embeds_cloth=None, garment_index=idx, **call)[0]
    assert eng.stats["garment_batches"] == n_garm and eng.stats["garment_stream_launches"] > n0
    # the engine-level call on the draws of the reference's order, on the device-resident slotted cache the same garments give
    _, noise = reference_draws(7, 123, B, H, W, steps, DT)
    ip = ip_states(enc, clip_pix)
    ref = engine_reference(eng, inp, noise, ip, steps, cloth=cache.slotted(DEV), garment_index=idx)
    assert torch.isfinite(img_c).all() and torch.equal(img_c, ref)
    with pytest.raises(ValueError, match="holds garments of several sizes: pass garment_index"):
        pipe(generator=gen_c, cloth=cache, text_embeds_cloth=None, **call)
