"""-m gpu: the copy-engine transport of host-resident garment caches.  Kernel level: idmvton_kv_place on framed operands (tests/frames.py) whose
sources are in device memory -- what the entry point is for -- against the torch definition of the packed format (widening) or the source bits
(copying), zero runs against the bits 0x0000, bit for bit, and against idmvton_kv_fill on the SAME table.  One workgroup per chunk of 1024
16-byte items: the shapes are the smallest that cross a chunk, fill one exactly, or hold one item.  Engine level: host_transport="copy" on a
cache in pinned host memory -- packed or 16-bit, plain, indexed or shelved -- against the same call on the device-resident cache AND against
host_transport="kernel": the sets receive the same bits, so EQUALITY in every execution form, no tolerance."""
import pytest
import torch

from tests.engine_support import (DEV, KEYS, MIXED_DSTS, MIXED_RUNS, STEPS, WEARS, base_call, boundary_inputs, boundary_pipeline, check_fill, e4m3_bytes,
                                  encode_three, engine, engine_inputs, engine_reference, garment_kw, gpu_shelf, ip_states, model, pin_frame,
                                  reference_draws, run_on, three_garments, to_host)
from tests.garment_support import DTYPES, FORMS

pytestmark = pytest.mark.gpu
COPY = pytest.mark.parametrize("copy", [False, True], ids=["widen", "copy"])


# ------------------------------------------------------------------------------------------------------------------ kernel
# (the notation of MIXED_RUNS in tests/engine_support.py) the edges of a one-chunk-per-workgroup grid: a run of exactly 1024 items when widening (64 rows
# x 256 bytes: no lane of its workgroup is clamped; 2048 = two full chunks when copying), a run of ONE item (1 x 16 bytes widening), a run of
# exactly 1024 items when copying (64 x 128 elements), a zero run
EDGE_DSTS = [(64, 256, 264), (1, 16, 24), (64, 128, 136), (3, 32, 40)]
EDGE_RUNS = [("d", 64, 256, 272, 2, 0, 0), ("d", 1, 16, 32, -1, 1, 0), ("d", 64, 128, 128, 7, 2, 0), ("z", 3, 32, 3, 0)]
ZERO_DSTS = [(7, 48, 56), (8, 48, 56), (9, 48, 56)]
ZERO_RUNS = [("z", 7, 48, 0, 0), ("z", 8, 48, 1, 0), ("z", 9, 48, 2, 0)]


def _place(dsts, runs, dtype, copy=False, on_host=()):
    """Framed destinations and framed sources (one exponent per data run) in device memory -- runs whose number is in `on_host`: in pinned host
    memory --, ONE idmvton_kv_place launch.  -> (destinations, sources by run, values by run, table)."""
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
        s = pin_frame(frames.framed(x, lds)) if i in on_host else frames.framed(x.to(DEV), lds)
        srcs[i], vals[i] = s, x
        descs.append((s, outs[d][:rows, c0:c0 + cols], None if copy else (exps_h if i in on_host else exps_d)[i:i + 1]))
    table = ops.kv_place(descs, dtype, mode=ffi.KVS_COPY if copy else ffi.KVS_WIDEN_E4M3)
    torch.cuda.synchronize()
    table.keep = (exps_h, exps_d)                        # the records name their addresses: a second launch of the table reads them again
    return outs, srcs, vals, table


def _same_as_kv_fill(outs, table, dtype):
    """The destinations' buffers -- frames included -- after idmvton_kv_place against idmvton_kv_fill on the same records into the same,
    re-poisoned buffers."""
    from idm_vton_amd import ops
    from tests import frames
    placed = [frames.ints(o._frame.buf).clone() for o in outs]
    for o in outs:
        frames.ints(o._frame.buf).copy_(o._frame.snapshot)
    fill = ops.KvFillTable(table.host, DEV, table.mode)
    assert type(table) is ops.KvPlaceTable and table.ENTRY == "kv_place" and fill.ENTRY == "kv_fill" and torch.equal(fill.first_host, table.first_host)
    ops.kv_fill(fill, dtype, workgroups=3)
    torch.cuda.synchronize()
    for d, (o, was) in enumerate(zip(outs, placed)):
        assert not torch.equal(frames.ints(o._frame.buf), o._frame.snapshot)
        assert torch.equal(frames.ints(o._frame.buf), was), f"destination {d}: idmvton_kv_place and idmvton_kv_fill differ"


@COPY
@DTYPES
def test_kv_place_mixed_table_from_device_memory(dtype, copy):
    """A compact run plus its zero tail into one destination, and 1120- and 1056-item runs that cross a chunk (copying: twice the items)."""
    outs, srcs, vals, table = _place(MIXED_DSTS, MIXED_RUNS, dtype, copy)
    assert table.items.tolist() == ([30, 40, 2240, 2112] if copy else [15, 20, 1120, 1056])
    assert table.first_host.tolist() == ([0, 1, 2, 5, 8] if copy else [0, 1, 2, 4, 6]) and all(s.is_cuda for s in srcs.values())
    assert table.host[:, 0].ne(0).tolist() == [True, False, True, False] and table.host[1, 2] == 0
    check_fill(MIXED_DSTS, MIXED_RUNS, outs, srcs, vals, dtype, copy)
    _same_as_kv_fill(outs, table, dtype)


@COPY
@DTYPES
def test_kv_place_edges_of_a_one_chunk_per_workgroup_grid(dtype, copy):
    outs, srcs, vals, table = _place(EDGE_DSTS, EDGE_RUNS, dtype, copy)
    assert table.items.tolist() == ([2048, 2, 1024, 12] if copy else [1024, 1, 512, 6])
    assert table.first_host.tolist() == ([0, 2, 3, 4, 5] if copy else [0, 1, 2, 3, 4])
    check_fill(EDGE_DSTS, EDGE_RUNS, outs, srcs, vals, dtype, copy)
    _same_as_kv_fill(outs, table, dtype)


@COPY
def test_kv_place_table_of_zero_runs_only(copy):
    dtype = torch.float16
    outs, srcs, vals, table = _place(ZERO_DSTS, ZERO_RUNS, dtype, copy)
    assert not srcs and (table.host[:, 0] == 0).all() and (table.host[:, 2] == 0).all() and table.link_bytes() == 0.0
    assert table.first_host.tolist() == [0, 1, 2, 3]
    check_fill(ZERO_DSTS, ZERO_RUNS, outs, srcs, vals, dtype, copy)
    _same_as_kv_fill(outs, table, dtype)


def test_kv_place_one_table_mixes_device_and_pinned_host_sources():
    outs, srcs, vals, table = _place(MIXED_DSTS, MIXED_RUNS, torch.bfloat16, on_host=(0,))
    assert [srcs[i].is_cuda for i in sorted(srcs)] == [False, True] and srcs[0].is_pinned()
    check_fill(MIXED_DSTS, MIXED_RUNS, outs, srcs, vals, torch.bfloat16)
    _same_as_kv_fill(outs, table, torch.bfloat16)


def test_kv_place_wrapper_refuses_a_malformed_run():
    from idm_vton_amd import ffi, ops
    d = torch.full((4, 32), float("nan"), dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match="kv_place: a run is"):
        ops.kv_place([(None, d.to(torch.bfloat16), None)], torch.float16)
    with pytest.raises(RuntimeError, match=r"idmvton_kv_place failed \(-1\).*cols=24"):
        ops.kv_place([(None, d[:, :24], None)], torch.float16)
    t = ops.KvPlaceTable(torch.tensor([[0, d.data_ptr(), 0, 4 | (32 << 32), 32 | (32 << 32)]]), DEV)
    a = ffi.KvStreamArgs()
    a.dtype, a.mode, a.n, a.workgroups, a.desc, a.first = ffi.F16, ffi.KVS_WIDEN_E4M3, 1, 16, t.dev.data_ptr(), t.first_dev.data_ptr()
    with pytest.raises(RuntimeError, match=r"idmvton_kv_place failed \(-5\).*workgroups=16 must be 0"):
        ffi.call_kv_place(a, t.host.data_ptr(), t.first_host.data_ptr(), 0)
    torch.cuda.synchronize()
    assert torch.isnan(d).all()                          # nothing was launched


# ------------------------------------------------------------------------------------------------------------------ engine


def _forms(dtype):
    """f16: the four execution forms and on_step; bf16: graph + overlap alone."""
    return list(FORMS) if dtype == torch.float16 else ["graph_overlap"]


def _graphs(eng):
    return len(eng._graphs), sum(len(g["graphs"]) for g in eng._graphs.values())


def _three_ways(eng, base, device, host, index, forms, nblocks, copies_per_block):
    """Per form: the device-resident call first (a graph form's state then exists and must serve the other two), the kernel transport, the
    copy transport -- equal latents, no new state or capture, and the copy call's counters."""
    lat_d = None
    for form in forms:
        lat_d = run_on(eng, base, device, form, index)
        lat_k = run_on(eng, base, host, form, index, "kernel")
        graphs, s0 = _graphs(eng), dict(eng.stats)
        lat_c = run_on(eng, base, host, form, index, "copy")
        assert torch.isfinite(lat_d).all() and torch.isfinite(lat_c).all(), form
        assert torch.equal(lat_c, lat_d), (form, (lat_c - lat_d).abs().max().item())
        assert torch.equal(lat_c, lat_k), (form, (lat_c - lat_k).abs().max().item())
        assert _graphs(eng) == graphs, form
        delta = {key: eng.stats[key] - s0[key] for key in s0}
        assert delta == dict(garment_batches=0, garment_set_copies=0, garment_stream_launches=0, garment_stage_launches=nblocks,
                             garment_stage_copies=sum(copies_per_block)), (form, delta)
    return lat_d


def _arena(eng):
    assert len(eng._arenas) == 1
    return next(iter(eng._arenas.values()))[0]


CASES = {"packed": ("e4m3", 2, 2, None, 7), "packed_index": ("e4m3", 4, 3, [2, 0, 2, 0], 4), "16bit_index": ("native", 4, 4, [2, 0, 2, 1], 4)}


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
@DTYPES
def test_copy_transport_equals_the_device_resident_call_and_the_kernel_transport(dtype, case):
    """packed: P = G = 2, no index, 7 steps (blocks of 1, 2, 4 consecutive timesteps: one copy per cache tensor and block).  packed_index: P = 4
    persons on a G = 3 cache, garment_index [2, 0, 2, 0] (repeats; U = 2 < G: garment 1 is never copied), 4 steps (blocks of 1, 2, 1).
    16bit_index: a 16-bit G = 4 cache (copy mode), [2, 0, 2, 1]: U = 3 in the runs [2], [0, 1]."""
    storage, P, G, index, steps = CASES[case]
    eng, inp, _ = engine_inputs(dtype, P, steps)
    device = eng.encode_garment(num_inference_steps=steps, storage=storage, **garment_kw(inp, G))
    host = to_host(device)
    assert host.packed == (storage == "e4m3") and host.G == G
    k, blocks = eng._block_schedule(steps)
    assert [c for _, c in blocks] == ([1, 2, 4] if steps == 7 else [1, 2, 1])
    F = len(host.kv)
    runs = 1 if index is None else 2
    copies = [2 * F if index is None else c * runs * 2 * F for _, c in blocks]
    lat = _three_ways(eng, base_call(inp, steps), device, host, index, _forms(dtype), len(blocks), copies)
    # the arena: k timesteps of the U used garments in the source's storage -- derived, and never the size of the cache
    U = G if index is None else len(set(index))
    arena = _arena(eng)
    assert arena.dtype == torch.uint8 and arena.numel() == k * U * sum(t.numel() * t.element_size() for kv in host.kv for t in kv) // (steps * G)
    assert arena.numel() < host.nbytes
    if index is not None:                                # the assignment is read
        assert not torch.equal(run_on(eng, base_call(inp, steps), host, "serial_eager", index[::-1], "copy"), lat)


@pytest.mark.parametrize("storage", ["e4m3", "native"], ids=["packed", "16bit"])
@DTYPES
def test_copy_transport_of_a_shelf_of_three_sizes(dtype, storage):
    """Compact garments of latent 9x5, 8x12 and 16x16 in pinned host memory against slotted("cuda"): one copy per part tensor and block."""
    eng = engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    shelf = gpu_shelf(eng, encode_three(eng, garments), storage)
    shelved, index = shelf.get([KEYS[j] for j in WEARS])
    assert index == [0, 1, 2] and shelved.sizes == [(9, 5), (8, 12), (16, 16)] and shelved.host_resident
    device = shelved.slotted(DEV)
    k, blocks = eng._block_schedule(STEPS)
    assert len(blocks) == 2
    F = len(shelved.parts[0].kv)
    _three_ways(eng, base_call(inp, STEPS), device, shelved, index, _forms(dtype), len(blocks), [3 * 2 * F] * len(blocks))
    arena = _arena(eng)
    assert arena.numel() == k * sum(t.numel() * t.element_size() for p in shelved.parts for kv in p.kv for t in kv) // STEPS < device.nbytes   # compact


def test_two_copy_calls_through_one_state_use_the_arena_again():
    """A packed G = 3 host cache, two assignments through one graph state and one arena; each against a fresh engine's serial call on the
    device-resident cache."""
    dtype, steps = torch.float16, 4
    eng, inp, _ = engine_inputs(dtype, 4, steps)
    fresh, _, _ = engine_inputs(dtype, 4, steps)
    device = eng.encode_garment(num_inference_steps=steps, storage="e4m3", **garment_kw(inp, 3))
    host = to_host(device)
    base = base_call(inp, steps)
    seen = []
    for index in ([2, 0, 2, 0], [1, 2, 2, 1]):
        for form in ("graph_overlap", "serial_eager"):
            lat = run_on(eng, base, host, form, index, "copy")
            assert torch.equal(lat, run_on(fresh, base, device, "serial_eager", index)), (index, form)
            seen.append(_arena(eng).data_ptr())
    assert len(set(seen)) == 1 and len(eng._graphs) == 1 and eng.stats["garment_stream_launches"] == 0
    assert not eng._streaming or all(h[0] is host for h in eng._streaming)
    torch.cuda.synchronize()
    eng._release_streamed()
    assert eng._streaming == []


def test_shelf_slot_reuse_under_the_copy_transport():
    """Set slot 0 holds the largest garment, then the smallest -- its zero tail has to replace the larger garment's values, and the arena the
    larger call sized serves the smaller --, then a mix.  Each against the slotted device call of that assignment on a fresh engine."""
    dtype = torch.float16
    eng = engine(model(dtype), dtype)
    fresh = engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    ones = encode_three(eng, garments)
    shelf = gpu_shelf(eng, ones[1:], "e4m3")                # g0 = ones[1] (16x16), g1 = ones[2] (9x5): KEYS[:2]
    base = base_call(inp, STEPS)
    seen = []
    for form in ("graph", "graph_overlap"):
        for keys in (["g0"] * 3, ["g1"] * 3, ["g0"] * 3, ["g1", "g0", "g1"]):
            shelved, index = shelf.get(keys)
            lat = run_on(eng, base, shelved, form, index, "copy")
            ref = run_on(fresh, base, shelved.slotted(DEV), "serial_eager", index)
            assert torch.isfinite(lat).all() and torch.equal(lat, ref), (form, keys, (lat - ref).abs().max().item())
            seen.append({key: a.data_ptr() for key, (a, _) in eng._arenas.items()})
    assert len(eng._graphs) == 1 and eng.stats["garment_stream_launches"] == 0
    u1 = next(iter(seen[0]))                             # the U = 1 arena: sized by g0, used again by the smaller g1 and by g0 once more
    assert all(s[u1] == seen[0][u1] for s in seen) and len(seen[-1]) == 2


def test_copy_transport_refusals_come_before_anything_is_launched():
    steps = 3
    eng, inp, _ = engine_inputs(torch.float16, 2, steps)
    base = base_call(inp, steps)
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp))
    packed = cache.pack()
    stats = dict(eng.stats)
    for pageable in (cache.to("cpu"), packed.to("cpu")):
        with pytest.raises(ValueError, match="kv mismatch.*pageable.*pin_memory"):
            eng(return_latents=True, host_transport="copy", **{**base, "cloth": pageable})
    with pytest.raises(ValueError, match="host_transport='dma'"):
        eng(return_latents=True, host_transport="dma", **{**base, "cloth": to_host(packed)})
    with pytest.raises(ValueError, match="host_transport='dma'"):
        eng.denoise(eng.prepare(**{**base, "cloth": to_host(packed)}), host_transport="dma")
    assert eng.stats == stats and not eng._graphs and not eng._arenas
    eng8, inp8, _ = engine_inputs(torch.float16, 2, steps, fp8=True)
    cache8 = eng8.encode_garment(num_inference_steps=steps, **garment_kw(inp8))
    stats8 = dict(eng8.stats)
    with pytest.raises(ValueError, match="attn_fp8 mismatch.*does not stream"):
        eng8(return_latents=True, host_transport="copy", **{**base_call(inp8, steps), "cloth": to_host(cache8)})
    assert eng8.stats == stats8 and not eng8._graphs and not eng8._arenas
    # on a device-resident cache the keyword has no effect
    lat = run_on(eng, base, packed, "serial_eager", None, "copy")
    assert torch.equal(lat, run_on(eng, base, packed, "serial_eager")) and not eng._arenas and eng.stats["garment_stage_launches"] == 0


# ------------------------------------------------------------------------------------------------------------------ boundary
def test_boundary_pipeline_passes_host_transport_through():
    """pipe.host_transport = "copy" on a packed cache in pinned host memory against the engine-level call on the same draws and the
    DEVICE-RESIDENT cache."""
    DT = torch.float16
    pipe, enc, kw = boundary_pipeline(DT)
    assert pipe.host_transport == "kernel"
    B, H, W, steps = 2, 128, 128, 3
    inp, clip_pix, call = boundary_inputs(kw, B, H, W, steps, DT)
    device = pipe.encode_garment(inp["cloth"], inp["text_embeds_cloth"], steps, H, W, generator=torch.Generator(DEV).manual_seed(11), storage="e4m3")
    cache = to_host(device)
    index = [1, 1]
    eng = pipe.hip_engine()
    pipe.host_transport = "copy"
    s0 = dict(eng.stats)
    torch.manual_seed(123)                                                         # the pose posterior uses the GLOBAL generator
    img_c = pipe(generator=torch.Generator(DEV).manual_seed(7), cloth=cache, text_embeds_cloth=None, garment_index=index, **call)[0]
    assert eng.stats["garment_stream_launches"] == s0["garment_stream_launches"] and eng.stats["garment_stage_launches"] > s0["garment_stage_launches"]
    _, noise = reference_draws(7, 123, B, H, W, steps, DT)
    ip = ip_states(enc, clip_pix)
    ref = engine_reference(eng, inp, noise, ip, steps, cloth=device, garment_index=index)
    assert torch.isfinite(img_c).all() and torch.equal(img_c, ref)
    pipe.host_transport = "bogus"
    with pytest.raises(ValueError, match="host_transport='bogus'"):
        pipe(generator=torch.Generator(DEV).manual_seed(7), cloth=cache, text_embeds_cloth=None, garment_index=index, **call)
