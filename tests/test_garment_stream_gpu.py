"""-m gpu: the host-resident garment cache on the GPU.  Kernel level: idmvton_kv_stream on framed operands (tests/frames.py) whose sources and
exponents live in page-locked host memory, against the torch definition of the packed format (widen mode) and against the source bits (copy
mode), bit for bit.  Engine level: a call on a cache moved to pinned host memory against the same call on the device-resident cache --
the sets receive the same bits, so EQUALITY in every execution form --, the refusals, a host pool under captured graphs, and the boundary
pipeline."""
import ctypes as C

import pytest
import torch

from tests.engine_support import (DEV, RUNS, assert_bits, base_call, boundary_inputs, boundary_pipeline, e4m3_bytes, engine_inputs, engine_reference,
                                  garment_kw, ip_states, pin_frame, reference_draws, run_on, to_host)
from tests.garment_support import DTYPES, FORMS, IDX

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------------ kernel


def _widen(runs, dtype, workgroups, on_device=()):
    """Framed sources and one exponent per run in pinned host memory (runs whose number is in `on_device`: in device memory), framed
    destinations on the device, one idmvton_kv_stream launch of `workgroups` workgroups."""
    from idm_vton_amd import ops
    from tests import frames
    exps_h = torch.tensor([r[4] for r in runs], dtype=torch.int32).pin_memory()
    exps_d = exps_h.to(DEV)
    srcs, dsts, descs = [], [], []
    for i, (rows, cols, lds, ldd, _) in enumerate(runs):
        b = e4m3_bytes(rows, cols, seed=i)
        s = frames.framed(b.to(DEV), lds) if i in on_device else pin_frame(frames.framed(b, lds))   # gap columns and guard bands: 0x7f, e4m3's NaN
        d = frames.framed_out((rows, cols), dtype, DEV, ldd)
        srcs.append(s); dsts.append(d)
        descs.append((s, d, (exps_d if i in on_device else exps_h)[i:i + 1]))
    table = ops.kv_stream(descs, dtype, workgroups=workgroups)
    torch.cuda.synchronize()
    return srcs, dsts, table


def _check_widen(runs, srcs, dsts, dtype):
    from idm_vton_amd.garment_cache import unpack_values
    from tests import frames
    for i, ((rows, cols, lds, ldd, e), s, d) in enumerate(zip(runs, srcs, dsts)):
        b = e4m3_bytes(rows, cols, seed=i)
        frames.assert_all_written(d, f"run {i}")
        frames.assert_frame_intact(d, f"run {i}")        # guard bands and the gap columns [cols, ldd)
        frames.assert_untouched(s, f"run {i} source")
        assert_bits(d, unpack_values(b, torch.tensor(e), dtype), b, f"run {i}: not the format's bits")


@DTYPES
def test_kv_stream_widens_from_pinned_memory_bit_for_bit(dtype):
    """The five runs of the packed kernel test, 1 to 20600 16-byte items = 1, 1, 16, 5 and 21 chunks, 44 in all: 3 workgroups each loop fourteen or
    fifteen times and cross every descriptor boundary."""
    srcs, dsts, table = _widen(RUNS, dtype, workgroups=3)
    assert table.n == 5 and table.first_host.tolist() == [0, 1, 2, 18, 23, 44] and int(table.items.max()) == 515 * 40
    assert all(not s.is_cuda and s.is_pinned() for s in srcs)
    _check_widen(RUNS, srcs, dsts, dtype)


@DTYPES
def test_kv_stream_with_idle_workgroups(dtype):
    """64 workgroups, a table of one chunk: 63 find nothing to do."""
    srcs, dsts, table = _widen(RUNS[:1], dtype, workgroups=64)
    assert table.first_host.tolist() == [0, 1]
    _check_widen(RUNS[:1], srcs, dsts, dtype)


def test_kv_stream_one_table_mixes_host_and_device_sources():
    srcs, dsts, _ = _widen(RUNS, torch.bfloat16, workgroups=8, on_device=(1, 3))
    assert [s.is_cuda for s in srcs] == [False, True, False, True, False]
    _check_widen(RUNS, srcs, dsts, torch.bfloat16)


# (rows, cols, source row stride, destination row stride) in 16-bit elements: a row gap in the source, in the destination, in both, in neither
COPY_RUNS = [(1, 8, 8, 8), (37, 80, 96, 80), (200, 640, 640, 648), (515, 640, 656, 664), (96, 208, 208, 208)]


@DTYPES
def test_kv_stream_copy_mode_from_pinned_memory(dtype):
    from idm_vton_amd import ffi, ops
    from tests import frames
    srcs, dsts, vals, descs = [], [], [], []
    for i, (rows, cols, lds, ldd) in enumerate(COPY_RUNS):
        x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(i)).to(dtype)
        s, d = pin_frame(frames.framed(x, lds)), frames.framed_out((rows, cols), dtype, DEV, ldd)
        srcs.append(s); dsts.append(d); vals.append(x)
        descs.append((s, d, None))
    table = ops.kv_stream(descs, dtype, mode=ffi.KVS_COPY, workgroups=3)
    torch.cuda.synchronize()
    assert table.first_host.tolist()[-1] == sum((r * c // 8 + 1023) // 1024 for r, c, _, _ in COPY_RUNS)
    for i, (s, d, x) in enumerate(zip(srcs, dsts, vals)):
        frames.assert_all_written(d, f"run {i}")
        frames.assert_frame_intact(d, f"run {i}")
        frames.assert_untouched(s, f"run {i} source")
        assert torch.equal(frames.ints(d.cpu().contiguous()), frames.ints(x)), f"run {i}: not the source's bits"


def test_host_device_ptr_accepts_pinned_and_refuses_pageable_memory():
    from idm_vton_amd import ffi, ops
    L = ffi.lib()
    torch.cuda.init()
    pinned, pageable = torch.zeros(4096, dtype=torch.uint8).pin_memory(), torch.zeros(4096, dtype=torch.uint8)
    dev = C.c_void_p()
    assert L.idmvton_host_device_ptr(C.c_void_p(pinned.data_ptr()), C.byref(dev)) == 0 and dev.value
    assert L.idmvton_host_device_ptr(C.c_void_p(pinned.data_ptr() + 512), C.byref(dev)) == 0 and dev.value == ffi.host_device_ptr(pinned.data_ptr()) + 512
    assert ops.stream_address(pinned[512:]) == dev.value
    assert L.idmvton_host_device_ptr(C.c_void_p(pageable.data_ptr()), C.byref(dev)) == -5 and not dev.value
    assert b"not page-locked" in L.idmvton_last_error()
    with pytest.raises(ValueError, match="pin_memory"):
        ops.stream_address(pageable)
    d = torch.zeros(8, device=DEV)
    assert ops.stream_address(d) == d.data_ptr()
    torch.cuda.synchronize()                             # the refusal left no error behind
    assert float((d + 1).sum()) == 8.0


def test_kv_stream_wrapper_refuses_a_malformed_run():
    from idm_vton_amd import ffi, ops
    e = torch.zeros(1, dtype=torch.int32).pin_memory()
    s, d = torch.zeros(4, 32, dtype=torch.uint8).pin_memory(), torch.full((4, 32), float("nan"), dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError, match="kv_stream: a run is"):
        ops.kv_stream([(s, d.to(torch.bfloat16), e)], torch.float16)
    with pytest.raises(ValueError, match="pin_memory"):
        ops.kv_stream([(torch.zeros(4, 32, dtype=torch.uint8), d, e)], torch.float16)
    with pytest.raises(RuntimeError, match=r"idmvton_kv_stream failed \(-1\).*cols=24"):
        ops.kv_stream([(s[:, :24], d[:, :24], e)], torch.float16)
    with pytest.raises(RuntimeError, match=r"idmvton_kv_stream failed \(-5\).*workgroups=0"):
        ops.kv_stream([(s, d, e)], torch.float16, workgroups=0)
    with pytest.raises(RuntimeError, match=r"idmvton_kv_stream failed \(-5\).*mode 7"):
        ops.kv_stream(ops.KvStreamTable(ops.kv_stream([(s, d, e)], torch.float16).host, DEV, 7), torch.float16)
    torch.cuda.synchronize()
    assert (d == 0).all()                                # only the one valid launch wrote (zero bytes widen to zero)


# ------------------------------------------------------------------------------------------------------------------ engine


@DTYPES
def test_packed_host_cache_equals_the_device_resident_call(dtype):
    """P = 4 persons on a G = 3 packed cache in pinned host memory, garment_index = [2, 0, 2, 1], 4 steps (blocks of 1, 2, 1 timesteps): every
    execution form against the same call on the device-resident cache, and one idmvton_kv_stream launch per block.  (The device call of a
    form runs first, so a graph form's state exists when the host call starts: a state built on a device cache serves the host one.)"""
    steps = 4
    eng, inp, _ = engine_inputs(dtype, 4, steps)
    packed = eng.encode_garment(num_inference_steps=steps, storage="e4m3", **garment_kw(inp, 3))
    host = to_host(packed)
    assert host.packed and host.exps.is_pinned() and host.G == 3
    base = base_call(inp, steps)
    nblocks = len(eng._block_schedule(steps)[1])
    assert nblocks == 3
    for form in FORMS:
        lat_d = run_on(eng, base, packed, form, IDX)
        states, n0, c0 = len(eng._graphs), eng.stats["garment_stream_launches"], eng.stats["garment_set_copies"]
        lat_h = run_on(eng, base, host, form, IDX)
        assert torch.isfinite(lat_d).all() and torch.equal(lat_h, lat_d), (form, (lat_h - lat_d).abs().max().item())
        assert eng.stats["garment_stream_launches"] - n0 == nblocks, form
        assert eng.stats["garment_set_copies"] == c0 and len(eng._graphs) == states, form
    assert not torch.equal(run_on(eng, base, host, "serial_eager", [0, 0, 1, 2]), lat_d)    # another index gives other latents


@DTYPES
def test_16bit_host_cache_equals_the_device_resident_call(dtype):
    """A 16-bit cache in pinned host memory (copy mode), P = G = 2, 7 steps (blocks of 1, 2, 4 timesteps), and the strength-0.6 call on the
    same 7-step cache (its entries found by value)."""
    steps = 7
    eng, inp, _ = engine_inputs(dtype, 2, steps)
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp))
    host = to_host(cache)
    assert not host.packed
    base = base_call(inp, steps)
    part = dict(base, strength=0.6, noise={**base["noise"], "image": torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(77)),
                                           "steps": inp["noise"]["steps"][:4]})
    for what, call, nblocks in (("full", base, 3), ("strength 0.6", part, len(eng._block_schedule(4)[1]))):
        for form in FORMS:                               # (the device call first: a graph form's state then exists and serves the host call)
            lat_d = run_on(eng, call, cache, form)
            states, n0, c0 = len(eng._graphs), eng.stats["garment_stream_launches"], eng.stats["garment_set_copies"]
            lat_h = run_on(eng, call, host, form)
            assert torch.isfinite(lat_d).all() and torch.equal(lat_h, lat_d), (what, form, (lat_h - lat_d).abs().max().item())
            assert eng.stats["garment_stream_launches"] - n0 == nblocks, (what, form)
            assert eng.stats["garment_set_copies"] == c0 and len(eng._graphs) == states, (what, form)
    assert not torch.equal(lat_d, run_on(eng, base, cache, "serial_eager"))


def test_refusals_before_anything_is_launched():
    from idm_vton_amd.garment_cache import GarmentCache
    steps = 3
    eng, inp, _ = engine_inputs(torch.float16, 2, steps)
    base = base_call(inp, steps)
    cache = eng.encode_garment(num_inference_steps=steps, **garment_kw(inp))
    packed = cache.pack()
    stats = dict(eng.stats)
    with pytest.raises(ValueError, match="kv mismatch.*pageable.*pin_memory"):
        eng.prepare(**{**base, "cloth": cache.to("cpu")})
    with pytest.raises(ValueError, match="kv mismatch.*pageable.*pin_memory"):
        eng.prepare(**{**base, "cloth": packed.to("cpu")})
    half = to_host(packed)
    half.exps = half.exps.clone()                        # pinned bytes, pageable exponents
    assert not half.exps.is_pinned()
    with pytest.raises(ValueError, match="exps mismatch.*pageable.*pin_memory"):
        eng.prepare(**{**base, "cloth": half})
    slotted = to_host(eng.empty_garment_cache(2, garment_height=128, garment_width=128, num_inference_steps=steps))
    assert slotted.sizes is not None
    with pytest.raises(ValueError, match="sizes mismatch.*not streamed"):
        eng.prepare(**{**base, "cloth": slotted, "garment_index": [0, 1]})
    assert eng.stats == stats and not eng._graphs
    eng8, inp8, _ = engine_inputs(torch.float16, 2, steps, fp8=True)
    cache8 = eng8.encode_garment(num_inference_steps=steps, **garment_kw(inp8))
    stats8 = dict(eng8.stats)
    with pytest.raises(ValueError, match="attn_fp8 mismatch.*does not stream"):
        eng8.prepare(**{**base_call(inp8, steps), "cloth": to_host(cache8)})
    assert eng8.stats == stats8 and not eng8._graphs
    assert isinstance(cache8, GarmentCache)


def test_host_pool_swaps_a_garment_between_two_graph_calls():
    """A packed host pool of capacity 3; a fourth garment takes the least recently used slot between two graph-form calls: the second call
    equals a fresh engine's call on the swapped cache built apart on the device, and no graph state or graph was added."""
    from idm_vton_amd.garment_cache import GarmentCache, GarmentPool
    steps = 3
    eng, inp, _ = engine_inputs(torch.float16, 4, steps)
    enc = lambda i: eng.encode_garment(num_inference_steps=steps, storage="e4m3", cloth=inp["cloth"][i:i + 1],
                                       text_embeds_cloth=inp["text_embeds_cloth"][i:i + 1], noise_cloth=inp["noise"]["cloth"][i:i + 1])
    ones = {f"g{i}": enc(i) for i in range(4)}
    pool = GarmentPool(3, like=ones["g0"], resident="host")
    assert pool.cache.host_resident and pool.cache.packed and pool.cache.exps.is_pinned() and all(k.is_pinned() for k, _ in pool.cache.kv)
    assert pool.get(["g0", "g1", "g2"], encode=ones.get) == [0, 1, 2]
    base = base_call(inp, steps)
    fresh, _, _ = engine_inputs(torch.float16, 4, steps)
    before = GarmentCache.cat([ones["g0"], ones["g1"], ones["g2"]])
    swapped = GarmentCache.cat([ones["g0"], ones["g3"], ones["g2"]])
    ref_before, ref_after = run_on(fresh, base, before, "serial_eager", IDX), run_on(fresh, base, swapped, "serial_eager", IDX)
    assert not torch.equal(ref_before, ref_after)
    for form in ("graph", "graph_overlap"):
        assert torch.equal(run_on(eng, base, pool.cache, form, IDX), ref_before), form
    states, graphs = len(eng._graphs), sum(len(g["graphs"]) for g in eng._graphs.values())
    ptrs = [k.data_ptr() for k, _ in pool.cache.kv] + [pool.cache.exps.data_ptr()]
    assert pool.get(["g0", "g3", "g2"], encode=ones.get) == [0, 1, 2]            # g1 is the least recently used garment the batch does not name
    assert ptrs == [k.data_ptr() for k, _ in pool.cache.kv] + [pool.cache.exps.data_ptr()] and pool.stats["evicted"] == 1
    for form in ("graph", "graph_overlap"):
        assert torch.equal(run_on(eng, base, pool.cache, form, IDX), ref_after), form
    assert len(eng._graphs) == states and sum(len(g["graphs"]) for g in eng._graphs.values()) == graphs


def test_boundary_pipeline_takes_a_host_resident_packed_cache():
    """pipe(cloth=<packed cache in pinned host memory>, garment_index=...) against the engine-level call on the same draws."""
    DT = torch.float16
    pipe, enc, kw = boundary_pipeline(DT)
    B, H, W, steps = 2, 128, 128, 3
    inp, clip_pix, call = boundary_inputs(kw, B, H, W, steps, DT)
    cache = to_host(pipe.encode_garment(inp["cloth"], inp["text_embeds_cloth"], steps, H, W, generator=torch.Generator(DEV).manual_seed(11), storage="e4m3"))
    index = [1, 1]
    eng = pipe.hip_engine()
    n0 = eng.stats["garment_stream_launches"]
    torch.manual_seed(123)                                                         # the pose posterior uses the GLOBAL generator
    img_c = pipe(generator=torch.Generator(DEV).manual_seed(7), cloth=cache, text_embeds_cloth=None, garment_index=index, **call)[0]
    assert eng.stats["garment_stream_launches"] > n0 and cache.host_resident
    _, noise = reference_draws(7, 123, B, H, W, steps, DT)
    ip = ip_states(enc, clip_pix)
    ref = engine_reference(eng, inp, noise, ip, steps, cloth=cache, garment_index=index)
    assert torch.isfinite(img_c).all() and torch.equal(img_c, ref)
