"""-m gpu: the FEATURE SHELF on the GPU -- a GarmentShelf of storage "features" / "features-e4m3" (compact feature caches of many sizes in
page-locked host memory) as `cloth=` with `garment_index=`.  Kernel level: the one record form the feature relies on, a compact data run in
front of a destination and a zero ROW run over all rows behind it, through idmvton_kv_fill and idmvton_kv_place as they are, on framed
operands (tests/frames.py).  Engine level, on the tiny engine and the three garment sizes of tests/engine_support.py (latent 8x12,
16x16 = the slot's, 9x5 with padded token rows; 3 steps: blocks of 1 and 2): slot-sized garments against today's plain host-resident feature
cache, mixed sizes against the K / V^T shelf that engine.project_garment makes of the same garments, packed against its unpacked values,
slot reuse through one graph state whose staging lists and sets were filled with NaN in between, counters and link bytes, refusals, the
boundary pipeline.  Widening is exact: every bar is torch.equal plus isfinite."""
import pytest
import torch

from tests.engine_support import (DEV, GARMENT_HW, KEYS, STEPS, WEARS, H, W, assert_bits, base_call, boundary_inputs, boundary_pipeline, e4m3_bytes,
                                  encode_three, engine, engine_reference, gpu_shelf, ip_states, model, oracle_latents, pin_frame, reference_draws,
                                  run_on, three_garments)
from tests.garment_support import DTYPES, FORMS, PACKED, TRANSPORTS

pytestmark = pytest.mark.gpu
NBLOCKS = 2


# ------------------------------------------------------------------------------------------------------------------ kernel
ROWS, FRONT, WIDTH = 75, 5, 256                          # one destination of 75 rows x 256 columns (ld 256): 5 data rows, 70 zero rows


@DTYPES
@pytest.mark.parametrize("entry,workgroups", [("kv_fill", 1), ("kv_fill", 16), ("kv_place", None)], ids=["fill-wg1", "fill-wg16", "place"])
@pytest.mark.parametrize("copy", [False, True], ids=["widen", "copy"])
def test_a_compact_run_and_the_zero_row_run_behind_it(dtype, entry, workgroups, copy):
    """The geometry a compact F in a larger staging slot has: the data run's rows in front, ONE zero run over every row behind them --
    widening 70 x 256 / 16 = 1120 items, one full chunk of 1024 and one partial; copying twice that.  The data bits are the format's /
    the source's, the zero bits 0x0000, the frame intact, every element of the destination written."""
    from idm_vton_amd import ffi, ops
    from idm_vton_amd.garment_cache import unpack_values
    from tests import frames
    out = frames.framed_out((ROWS, WIDTH), dtype, DEV, WIDTH)
    e = -3
    x = torch.randn(FRONT, WIDTH, generator=torch.Generator().manual_seed(5)).to(dtype) if copy else e4m3_bytes(FRONT, WIDTH, seed=5)
    on_host = entry == "kv_fill"                         # kv_fill reads page-locked host memory, kv_place a staging arena in HBM
    src = pin_frame(frames.framed(x, WIDTH + 16)) if on_host else frames.framed(x.to(DEV), WIDTH + 16)
    exps = torch.tensor([e], dtype=torch.int32)
    exps = exps.pin_memory() if on_host else exps.to(DEV)
    descs = [(src, out[:FRONT], None if copy else exps[0:1]), (None, out[FRONT:], None)]
    mode = ffi.KVS_COPY if copy else ffi.KVS_WIDEN_E4M3
    table = ops.kv_fill(descs, dtype, mode=mode, workgroups=workgroups) if entry == "kv_fill" else ops.kv_place(descs, dtype, mode=mode)
    torch.cuda.synchronize()
    assert table.ENTRY == entry and table.items.tolist() == ([160, 2240] if copy else [80, 1120])
    assert table.first_host.tolist() == ([0, 1, 4] if copy else [0, 1, 3]) and table.host[:, 0].ne(0).tolist() == [True, False]
    assert table.host[1, 2] == 0 and table.link_bytes() == 16.0 * table.items[0].item()
    frames.assert_all_written(out, "destination")
    frames.assert_frame_intact(out, "destination")
    frames.assert_untouched(src, "source")
    if copy:
        assert torch.equal(frames.ints(out[:FRONT].cpu().contiguous()), frames.ints(x)), "the data run is not the source's bits"
    else:
        assert_bits(out[:FRONT], unpack_values(x, torch.tensor(e), dtype), x, "the data run is not the format's bits")
    tail = frames.ints(out[FRONT:].cpu().contiguous())
    assert (tail == 0).all(), f"a zero run's bits are 0x0000, got {sorted(set(tail.flatten().tolist()))[:4]}"


# ------------------------------------------------------------------------------------------------------------------ engine


def _storage(packed):
    return "features-e4m3" if packed else "features"


def _delta(eng, s0):
    return {key: eng.stats[key] - s0.get(key, 0) for key in eng.stats if key != "garment_stage_copies"}


def _per_block(transport):
    return dict(garment_batches=0, garment_set_copies=0, garment_projections=NBLOCKS, garment_stream_launches=NBLOCKS if transport == "kernel" else 0,
                garment_stage_launches=NBLOCKS if transport == "copy" else 0)


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
@PACKED
@DTYPES
def test_slot_sized_garments_equal_the_plain_host_resident_feature_cache(dtype, packed):
    """Three garments of the slot's own size: no zero run anywhere, and the shelf call moves what the call on cat(parts), pinned in host
    memory, moves -- today's path (idmvton_kv_stream, a plain indexed segment) -- into the same S slots."""
    from idm_vton_amd.garment_cache import GarmentCache
    eng = engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    g = torch.Generator().manual_seed(31)
    same = [dict(cloth=torch.randn(1, 3, H, W, generator=g).clamp(-1, 1), noise_cloth=torch.randn(1, 4, H // 8, W // 8, generator=g),
                 text_embeds_cloth=garments[j]["text_embeds_cloth"]) for j in range(3)]
    shelf = gpu_shelf(eng, encode_three(eng, same, storage="features"), _storage(packed))
    shelved, index = shelf.get([KEYS[j] for j in WEARS])
    assert shelved.features and shelved.sizes == [(16, 16)] * 3 and index == [0, 1, 2]
    plain = GarmentCache.cat(shelved.parts).to("cpu", pin_memory=True)
    assert plain.features and plain.sizes is None and plain.packed == packed and plain.host_resident and plain.nbytes == shelved.nbytes
    base = base_call(inp, STEPS)
    for form in FORMS:
        for transport in TRANSPORTS:
            lat_p = run_on(eng, base, plain, form, index, transport)
            s0 = dict(eng.stats)
            lat_s = run_on(eng, base, shelved, form, index, transport)
            d = _delta(eng, s0)
            assert torch.isfinite(lat_p).all() and torch.equal(lat_s, lat_p), (form, transport, (lat_s - lat_p).abs().max().item())
            # (a graph state's first call adds its warm-up fill to the launch counter of its transport, as ever)
            warm = {k: d[k] - v for k, v in _per_block(transport).items()}
            assert all(v == 0 for k, v in warm.items() if k not in ("garment_stream_launches", "garment_stage_launches")) and sum(warm.values()) in (0, 1), (form, transport, d)


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
@PACKED
@DTYPES
def test_mixed_sizes_equal_the_kv_shelf_of_the_same_garments(dtype, packed):
    """Persons wearing garments of three sizes: the feature-shelf call against the call on engine.project_garment(cache), the K / V^T shelf
    of the same garments (each part projected at its own size).  The shelf call projects at slot size, M = c * 3 * N_f rows: equality rests
    on a GEMM row not depending on M, asserted here with the difference printed; the per-person fp32 oracle bounds both at the bar of
    tests/test_garment_ragged_gpu.py (16-bit storage: the packed form is lossy by its format, not by this path)."""
    from tests import parity_utils as pu
    from tests.parity_checks import TOL
    eng = engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    shelf = gpu_shelf(eng, encode_three(eng, garments, storage="features"), _storage(packed))
    assert shelf.nbytes == sum(p.nbytes for p in shelf._parts.values()) < 3 * shelf._parts["g1"].nbytes
    shelved, index = shelf.get([KEYS[j] for j in WEARS])
    assert index == [0, 1, 2] and shelved.sizes == [(9, 5), (8, 12), (16, 16)] and shelved.features and shelved.packed == packed
    kv = eng.project_garment(shelved)
    assert not kv.features and not kv.packed and kv.sizes == shelved.sizes and kv.slot_shapes == shelved.slot_shapes and (kv.gh, kv.gw) == (16, 16)
    assert all(t.is_pinned() for p in kv.parts for e in p.kv for t in e)
    if not packed:
        assert kv.nbytes == 2 * shelved.nbytes           # exactly half the bytes of the compact K / V^T parts
    base = base_call(inp, STEPS)
    for form in FORMS:
        for transport in TRANSPORTS:
            lat_k = run_on(eng, base, kv, form, index, transport)
            states = len(eng._graphs)
            lat_f = run_on(eng, base, shelved, form, index, transport)
            print(f"{dtype} {'packed' if packed else '16bit'} {form} {transport}: max|feature shelf - kv shelf| = {(lat_f - lat_k).abs().max().item():.3e}")
            assert torch.isfinite(lat_k).all() and torch.isfinite(lat_f).all(), (form, transport)
            assert torch.equal(lat_f, lat_k), (form, transport, (lat_f - lat_k).abs().max().item())
            assert len(eng._graphs) == states, (form, transport)         # one graph state serves both kinds of shelf
    assert not torch.equal(run_on(eng, base, shelved, "serial_eager", [0, 0, 1]), lat_k)       # and the assignment is read
    if not packed:
        for i, ref in enumerate(oracle_latents(dtype)):
            err = pu.relerr(lat_f[i:i + 1], ref)
            print(f"{dtype} person {i} in garment {WEARS[i]} ({GARMENT_HW[WEARS[i]]}): feature shelf against the oracle {err:.3e} (bar {TOL[dtype]['latents']:.1e})")
            assert err <= TOL[dtype]["latents"], (i, err)


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
@DTYPES
def test_packed_shelf_equals_the_16bit_shelf_of_its_unpacked_parts(dtype):
    from idm_vton_amd.garment_cache import GarmentShelf
    eng = engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    ones = encode_three(eng, garments, storage="features")
    packed_shelf = gpu_shelf(eng, ones, "features-e4m3")
    wide = GarmentShelf(packed_shelf._parts["g1"], storage="features")    # (`like`: a G = 1 feature cache of the slot's size)
    assert wide.slot_shapes == packed_shelf.slot_shapes
    for key in KEYS:
        wide.add(key, packed_shelf._parts[key].unpack())
    assert not any(torch.equal(a[0], b[0].cpu()) for a, b in zip(wide._parts["g0"].kv, ones[0].kv))          # lossy: not the 16-bit original
    keys = [KEYS[j] for j in WEARS]
    (cp, index), (cw, index_w) = packed_shelf.get(keys), wide.get(keys)
    assert index == index_w and cp.packed and not cw.packed and cp.nbytes == cw.nbytes // 2 + 4 * 3 * len(cp.slot_shapes)
    base = base_call(inp, STEPS)
    for form in FORMS:
        for transport in TRANSPORTS:
            lat_p, lat_w = run_on(eng, base, cp, form, index, transport), run_on(eng, base, cw, form, index, transport)
            assert torch.isfinite(lat_w).all() and torch.equal(lat_p, lat_w), (form, transport, (lat_p - lat_w).abs().max().item())


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
@PACKED
def test_slot_reuse_through_one_graph_state_poisoned_between_calls(packed):
    """Slot 0 holds the largest garment, then -- through the same graph state, whose staging lists and sets are filled with NaN in between --
    the smallest.  Without the zero-row run the rows behind the small garment's F would keep NaN, its K rows and V^T tail would be NaN, and
    a NaN times a zero probability is NaN: the latents show it, where stale finite rows would not."""
    dtype = torch.float16
    eng, fresh = engine(model(dtype), dtype), engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    shelf = gpu_shelf(eng, encode_three(eng, garments, storage="features"), _storage(packed))
    base = base_call(inp, STEPS)
    nan = float("nan")
    for transport in TRANSPORTS:
        for form in ("graph", "graph_overlap"):
            for keys in (["g1"] * 3, ["g2"] * 3, ["g2", "g1", "g0"]):        # 16x16, then 9x5 in the same slot, then all three
                shelved, index = shelf.get(keys)
                lat = run_on(eng, base, shelved, form, index, transport)
                ref = run_on(fresh, base, shelved, "serial_eager", index)
                assert torch.isfinite(lat).all() and torch.equal(lat, ref), (transport, form, keys, (lat - ref).abs().max().item())
                torch.cuda.synchronize()
                assert len(eng._graphs) == 1
                for state in eng._graphs.values():
                    for fs in state["sets"]:
                        assert fs["feats"]
                        for t in fs["feats"] + [t for e in fs["kv"] for t in e]:
                            t.fill_(nan)
        for arena, _ in eng._arenas.values():                # the copy transport's staging arena too
            arena.fill_(0xff)


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
@PACKED
def test_counters_link_bytes_and_refusals(packed, monkeypatch):
    from idm_vton_amd import ops
    from idm_vton_amd.garment_cache import ShelvedGarmentCache
    dtype = torch.float16
    eng = engine(model(dtype), dtype)
    inp, garments = three_garments(dtype)
    shelf = gpu_shelf(eng, encode_three(eng, garments, storage="features"), _storage(packed))
    shelved, index = shelf.get([KEYS[j] for j in WEARS])
    base = base_call(inp, STEPS)
    tables = []
    for name in ("KvFillTable", "KvPlaceTable"):
        cls = getattr(ops, name)
        monkeypatch.setattr(ops, name, type(name, (cls,), {"__init__": lambda self, *a, _c=cls, **kw: (tables.append(self), _c.__init__(self, *a, **kw))[1]}))
    n = len(shelved.timesteps)
    own = sum(t.numel() * t.element_size() for p in shelved.parts for e in p.kv for t in e) // n          # compact source bytes per timestep
    tensors = sum(len(p.kv) for p in shelved.parts)
    blocks = eng._block_schedule(STEPS)[1]
    assert [c for _, c in blocks] == [1, 2]
    for transport in TRANSPORTS:
        for form in ("serial_eager", "overlap_eager"):
            del tables[:]
            s0 = dict(eng.stats)
            lat = run_on(eng, base, shelved, form, index, transport)
            assert torch.isfinite(lat).all()
            assert _delta(eng, s0) == _per_block(transport), (form, transport)
            if transport == "copy":                      # one copy per part tensor and block (the call's entries are consecutive)
                assert eng.stats["garment_stage_copies"] - s0.get("garment_stage_copies", 0) == NBLOCKS * tensors
            (table,) = tables
            assert type(table).__name__ == ("KvFillTable" if transport == "kernel" else "KvPlaceTable")
            per = table.slices[0][1]                     # the one-timestep block's slice: the records of a timestep
            pad = table.host[per - 1]                    # an odd record count is made even by repeating the smallest record: read twice if a data run
            twice = 16 * int(table.items[per - 1]) if bool((table.host[:per - 1] == pad).all(dim=1).any()) and int(pad[0]) != 0 else 0
            assert {c for _, c in table.slices} == {c * per for _, c in blocks}
            for f0, cnt in table.slices:
                assert table.link_bytes(f0, cnt) == (own + twice) * (cnt // per), (form, transport, f0, cnt)
            zero = table.host[:per][table.host[:per, 0] == 0]
            assert len(zero) and (zero[:, 2] == 0).all()
    torch.cuda.synchronize()
    eng._release_streamed()
    assert eng._streaming == []
    # refusals: before anything is launched, the counters untouched
    stats, launched = dict(eng.stats), []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda *a, **kw: (launched.append(a[0]), real(*a, **kw))[1])
    p1 = shelved.parts[1]
    clone = p1._like(kv=[(f.clone(),) for f, in p1.kv], **(dict(exps=p1.exps) if packed else {}))
    pageable = ShelvedGarmentCache([shelved.parts[0], clone, shelved.parts[2]], gh=shelved.gh, gw=shelved.gw, slot_shapes=shelved.slot_shapes)
    assert pageable.features and not pageable.parts[1].kv[0][0].is_pinned()
    with pytest.raises(ValueError, match="kv mismatch.*pageable.*pin_memory"):
        eng.prepare(**{**base, "cloth": pageable, "garment_index": index})
    with pytest.raises(ValueError, match="holds garments of several sizes: pass garment_index"):
        eng.prepare(**{**base, "cloth": shelved})
    with pytest.raises(ValueError, match="slotted: features"):
        shelved.slotted(DEV)
    assert eng.stats == stats and launched == []
    eng8 = engine(model(dtype, True), dtype)
    stats8 = dict(eng8.stats)
    with pytest.raises(ValueError, match="attn_fp8"):
        eng8.prepare(**{**base, "cloth": shelved, "garment_index": index})
    with pytest.raises(ValueError, match="attn_fp8"):
        eng8.project_garment(shelved)
    assert eng8.stats == stats8 and not eng8._graphs and launched == []


# ---- 7 ------------------------------------------------------------------------------------------------------------------------------------
def test_boundary_pipeline_passes_a_feature_shelf_cache_through():
    from idm_vton_amd.garment_cache import GarmentShelf, ShelvedGarmentCache
    DT = torch.float16
    pipe, enc, kw = boundary_pipeline(DT)
    B, steps = 3, 3
    inp, clip_pix, call = boundary_inputs(kw, B, H, W, steps, DT)
    small = torch.randn(1, 3, 64, 96, generator=torch.Generator().manual_seed(13)).clamp(-1, 1)
    cloths = {"small": (small, inp["text_embeds_cloth"][:1]), "full": (inp["cloth"][1:2], inp["text_embeds_cloth"][1:2])}
    encode = lambda key: pipe.encode_garment(cloths[key][0], cloths[key][1], steps, H, W, generator=torch.Generator(DEV).manual_seed(11), storage="features")
    shelf = GarmentShelf(pipe.empty_garment_cache(1, H, W, steps), storage="features-e4m3")
    cache, idx = shelf.get(["full", "small", "full"], encode)
    assert isinstance(cache, ShelvedGarmentCache) and cache.features and cache.packed and idx == [0, 1, 0] and cache.sizes == [(16, 16), (8, 12)]
    eng = pipe.hip_engine()
    # the engine-level call on the draws of the reference's order, on the same cache
    gen, noise = reference_draws(7, 123, B, H, W, steps, DT)
    ip = ip_states(enc, clip_pix)
    ref = engine_reference(eng, inp, noise, ip, steps, cloth=cache, garment_index=idx).clone()
    assert torch.isfinite(ref).all()
    for transport, counter in (("kernel", "garment_stream_launches"), ("copy", "garment_stage_launches")):
        pipe.host_transport = transport
        n_garm, n0, p0 = eng.stats["garment_batches"], eng.stats[counter], eng.stats["garment_projections"]
        torch.manual_seed(123)                                                     # the pose posterior uses the GLOBAL generator
        img = pipe(generator=torch.Generator(DEV).manual_seed(7), cloth=cache, text_embeds_cloth=None, garment_index=idx, **call)[0]
        assert eng.stats["garment_batches"] == n_garm and eng.stats[counter] > n0 and eng.stats["garment_projections"] > p0
        assert torch.isfinite(img).all() and torch.equal(img, ref), transport
    with pytest.raises(ValueError, match="holds garments of several sizes: pass garment_index"):
        pipe(generator=gen, cloth=cache, text_embeds_cloth=None, **call)
