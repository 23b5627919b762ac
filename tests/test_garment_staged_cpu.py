"""CPU tests of the copy-engine transport of host-resident garment caches: the host side of idmvton_kv_place -- exported, additive to ABI version
9, every refusal raised before a launch (no GPU: the pointers are made up and never dereferenced) --, KvPlaceTable's launch, and
garment_cache.staged_plan -- the staging arena, the copy list and the place tables of pipeline.py's _staged_fill -- carried out on CPU tensors:
the copies as tensor copies, the tables by the record interpreter of tests/garment_support.py, against the tables today's kernel
transport (_stream_fill / _shelf_fill) builds, interpreted the same way."""
import ctypes as C
import os

import pytest
import torch

from tests.garment_support import PACKED, SHELF_KINDS, SHELF_SLOT, apply_records, cache3, cpu_shelf, record_fields


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_kv_place_is_exported_declared_and_additive():
    from idm_vton_amd import ffi
    L = ffi.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "idmvton_hip.h")).read()
    assert ("int idmvton_kv_place(const idmvton_kv_stream_args* a, const idmvton_kv_stream_desc* host_desc, const int32_t* host_first, "
            "void* stream);") in header
    assert "idmvton_kv_place" in ffi.SYMBOLS and hasattr(L, "idmvton_kv_place") and callable(ffi.call_kv_place)
    assert L.idmvton_abi_version() == 9 == ffi.ABI_VERSION
    assert L.idmvton_sizeof(b"idmvton_kv_place_args") == -1 and "idmvton_kv_place_args" not in header
    assert L.idmvton_sizeof(b"idmvton_kv_stream_desc") == 40 == C.sizeof(ffi.KvStreamDesc)
    assert L.idmvton_sizeof(b"idmvton_kv_stream_args") == 32 == C.sizeof(ffi.KvStreamArgs)
    for name, st in ffi.STRUCTS.items():
        assert L.idmvton_sizeof(name.encode()) == C.sizeof(st), name


def _table(over=None):
    """tests/test_garment_shelf_cpu.py's widening table of 3 runs with made-up addresses -- a data run 32 x 64 (1 chunk), a ZERO run 600 x 64 (3
    chunks; src, exp NULL, lds 0), a data run 16 x 64 -- with workgroups = 0, the fields of `over` = {(index, field): value} changed."""
    from idm_vton_amd import ffi
    n, rows = 3, (32, 600, 16)
    host = (ffi.KvStreamDesc * n)()
    for i in range(n):
        host[i].src, host[i].dst, host[i].exp = 0x100000 + 0x100000 * i, 0x800000 + 0x100000 * i, 0x40000 + 4 * i
        host[i].rows, host[i].cols, host[i].lds, host[i].ldd = rows[i], 64, 64, 128
    host[1].src, host[1].exp, host[1].lds = None, None, 0
    for (i, field), v in (over or {}).items():
        setattr(host[i], field, v)
    first = (C.c_int32 * (n + 1))(0, 1, 4, 5)
    a = ffi.KvStreamArgs()
    a.dtype, a.mode, a.n, a.workgroups, a.desc, a.first = ffi.BF16, ffi.KVS_WIDEN_E4M3, n, 0, 0x200000, 0x300000
    return a, host, first


REFUSALS = [
    ("workgroups 16", {}, dict(workgroups=16), {}, -5, r"kv_place: workgroups=16 must be 0 \(the grid is the table's chunk count"),
    ("workgroups -1", {}, dict(workgroups=-1), {}, -5, "kv_place: workgroups=-1 must be 0"),
    ("dst null", {(0, "dst"): None}, {}, {}, -5, r"kv_place: descriptor 0 has a null pointer \(dst, or exp of a data run\)"),
    ("zero run dst null", {(1, "dst"): None}, {}, {}, -5, r"kv_place: descriptor 1 has a null pointer \(dst of a zero run\)"),
    ("dst alignment", {(2, "dst"): 0xa00008}, {}, {}, -3, "kv_place: descriptor 2: src / dst not 16-byte aligned"),
    ("zero run dst alignment", {(1, "dst"): 0x900008}, {}, {}, -3, "kv_place: descriptor 1: src / dst not 16-byte aligned"),
    ("src alignment", {(0, "src"): 0x100004}, {}, {}, -3, "kv_place: descriptor 0: src / dst not 16-byte aligned"),
    ("cols % 16", {(0, "cols"): 40}, {}, {}, -1, r"kv_place: descriptor 0: rows=32 cols=40 \(rows >= 1, cols a multiple of 16\)"),
    ("zero run cols % 16", {(1, "cols"): 40}, {}, {}, -1, "kv_place: descriptor 1: rows=600 cols=40"),
    ("rows 0", {(2, "rows"): 0}, {}, {}, -1, "kv_place: descriptor 2: rows=0 cols=64"),
    ("ldd < cols", {(0, "ldd"): 48}, {}, {}, -1, r"kv_place: descriptor 0: ldd=48 \(>= cols=64, a multiple of 8\)"),
    ("ldd % 16, copying", {(1, "ldd"): 72}, dict(mode=1), {}, -1, r"kv_place: descriptor 1: ldd=72 \(>= cols=64, a multiple of 16\)"),
    ("lds < cols", {(0, "lds"): 48}, {}, {}, -1, r"kv_place: descriptor 0: lds=48 \(>= cols=64"),
    ("host_first middle", {}, {}, {2: 3}, -5, r"kv_place: host_first\[2\]=3, the runs before descriptor 2 have 4 chunks"),
    ("host_first total", {}, {}, {3: 6}, -5, r"kv_place: host_first\[3\]=6, the table has 5 chunks"),
    ("data run exp null, widening", {(2, "exp"): None}, {}, {}, -5, "kv_place: descriptor 2 has a null pointer"),
    ("mode 7", {}, dict(mode=7), {}, -5, "kv_place: mode 7"),
    ("dtype f32", {}, dict(dtype=2), {}, -2, "kv_place: dtype 2"),
    ("n 0", {}, dict(n=0), {}, -5, r"kv_place: n=0 outside \[1, 1048576\]"),
]


@pytest.mark.parametrize("over,args,first_over,code,msg", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_kv_place_refuses_on_the_host(over, args, first_over, code, msg):
    from idm_vton_amd import ffi
    L = ffi.lib()
    a, host, first = _table(over)
    for k, v in args.items():
        setattr(a, k, v)
    for i, v in first_over.items():
        first[i] = v
    assert L.idmvton_kv_place(C.byref(a), C.cast(host, C.c_void_p), C.cast(first, C.c_void_p), None) == code
    with pytest.raises(RuntimeError, match=msg):
        ffi.call_kv_place(a, host, first, 0)


def test_a_table_of_zero_runs_only_is_valid_up_to_its_last_check():
    """Every field valid, the refusals end at the launch itself, which this machine cannot make: a table of zero runs only (src, exp NULL, lds 0,
    both modes) is checked up to its LAST check, the prefix total, by breaking only that."""
    from idm_vton_amd import ffi
    L = ffi.lib()
    for mode in (ffi.KVS_WIDEN_E4M3, ffi.KVS_COPY):
        a, host, first = _table({(i, f): v for i in (0, 2) for f, v in (("src", None), ("exp", None), ("lds", 0))})
        a.mode = mode
        first[3] = 9
        assert L.idmvton_kv_place(C.byref(a), C.cast(host, C.c_void_p), C.cast(first, C.c_void_p), None) == -5
        assert b"kv_place: host_first[3]=9, the table has 5 chunks" in L.idmvton_last_error()


def test_place_table_launches_its_entry_point_with_no_workgroup_count(monkeypatch):
    """KvPlaceTable launches idmvton_kv_place with workgroups == 0 whatever it is asked, and the slice's host and device addresses (the call is
    recorded, not made: no GPU)."""
    from idm_vton_amd import ffi, ops
    rec = torch.tensor([[4096, 8192, 64, 4 | (64 << 32), 64 | (64 << 32)], [0, 16384, 0, 2 | (16 << 32), 16 | (64 << 32)]] * 2)
    calls = []
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "PROFILE", None)
    for name in ("kv_stream", "kv_fill", "kv_place"):
        monkeypatch.setattr(ops.ffi, "call_" + name, lambda a, desc, first, stream, name=name: calls.append((name, a.n, a.mode, a.workgroups, a.desc, a.first, desc, first)))
    t = ops.KvPlaceTable(rec, "cpu", ffi.KVS_WIDEN_E4M3, [(0, 2), (2, 2)])
    assert isinstance(t, ops.KvFillTable) and t.ENTRY == "kv_place" and t.link_bytes() == 16.0 * 2 * 16
    t.launch(torch.float16, 1, 3)
    assert calls.pop() == ("kv_place", 2, ffi.KVS_WIDEN_E4M3, 0, t.dev.data_ptr() + 80, t.first_dev.data_ptr() + 12, t.host.data_ptr() + 80,
                           t.first_host.data_ptr() + 12)
    t.launch(torch.bfloat16)
    assert calls.pop()[:4] == ("kv_place", 2, ffi.KVS_WIDEN_E4M3, 0)
    assert ops.kv_place(t, torch.float16) is t and calls.pop()[:4] == ("kv_place", 2, ffi.KVS_WIDEN_E4M3, 0) and not calls


# ------------------------------------------------------------------------------------------------------------------ staged tables
def _sets(shapes, k, S, dtype, fill):
    """A 16-bit set of k timesteps of S slots of (N, C) features, every byte `fill`."""
    dst = [(torch.empty(k * S * N, Cc, dtype=dtype), torch.empty(k * S, Cc, N, dtype=dtype)) for N, Cc in shapes]
    for t in (t for kvf in dst for t in kvf):
        t.view(torch.uint8).fill_(fill)
    return dst


def _same_bytes(a, b):
    return all(torch.equal(x.view(torch.uint8), y.view(torch.uint8)) for pa, pb in zip(a, b) for x, y in zip(pa, pb))


def _stage_and_place(plan, packed, dtype, idx, p, k):
    """What _staged_fill's garment(bi, p) does to set p for the block of cache entries idx: the copies, then the block's prefix of the table."""
    pairs = plan["copies"](idx)
    for d, s in pairs:
        assert d.shape == s.shape and d.dtype == s.dtype and d.data_ptr() >= plan["arena"].data_ptr() and \
            d.data_ptr() + d.numel() * d.element_size() <= plan["arena"].data_ptr() + plan["nbytes"]
        d.copy_(s)
    f0 = p * k * plan["per"]
    apply_records(plan["rec"][f0:f0 + len(idx) * plan["per"]], packed, dtype)
    return len(pairs)


BLOCKS = {"consecutive": [[0], [1, 2], [3]], "by value": [[3], [0, 2], [1]]}


@pytest.mark.parametrize("order", list(BLOCKS), ids=list(BLOCKS))
@PACKED
def test_staged_plain_cache_with_an_index_fills_the_sets_as_the_kernel_transport_does(packed, order):
    """A G = 3 cache of three features and 4 timesteps, garment_index [1, 1, 0]: U = 2 garments in first-use order into slots 0, 1 of two 3-slot
    sets of k = 3 timesteps, blocks of 1, 2, 1 timesteps alternating between the sets.  Kernel transport: fill_records from the cache
    (_stream_fill's table).  Copy transport: the copy list into the arena, then the place table.  The sets start as 0x7f bytes and must end
    byte for byte alike -- the slot nobody fills and, in a one-timestep block, the timestep slots behind it included."""
    from idm_vton_amd import ffi, ops
    from idm_vton_amd.garment_cache import fill_records, staged_plan
    dtype, n, G, k, S, gindex = torch.float16, 4, 3, 3, 3, [1, 1, 0]
    cache = cache3(G, n, dtype)
    if packed:
        cache = cache.pack()
        cache.exps.copy_(torch.arange(-3, -3 + cache.exps.numel(), dtype=torch.int32).view_as(cache.exps) % 9 - 2)   # distinct per (garment, feature, K | V^T)
    shapes = [(192, 64), (48, 128), (1040, 16)]
    want, got = [_sets(shapes, k, S, dtype, 0x7f) for _ in range(2)], [_sets(shapes, k, S, dtype, 0x7f) for _ in range(2)]
    plan = staged_plan(cache, gindex, k, S, got, "cpu")
    esz = 1 if packed else 2
    per_step = sum(2 * N * Cc * esz for N, Cc in shapes)                                   # one garment's source bytes per timestep
    assert plan["nbytes"] == plan["arena"].numel() == k * 2 * per_step < cache.nbytes and plan["arena"].dtype == torch.uint8
    assert plan["per"] == 2 * 3 * 2 and tuple(plan["rec"].shape) == (2 * k * plan["per"], 5) and plan["rec"].dtype == torch.int64
    assert (plan["exps"] is not None) == packed
    for d, s in plan["exps_copies"]:
        d.copy_(s)
    if packed:
        assert len(plan["exps_copies"]) == 2 and torch.equal(plan["exps"], cache.exps[[1, 0]])
    # every source address of the table lies in the arena, every exponent address in the staged exponents
    lo, hi = plan["arena"].data_ptr(), plan["arena"].data_ptr() + plan["nbytes"]
    for src, _, exp, rows, cols, lds, _ in record_fields(plan["rec"]):
        assert lo <= src and src + (rows - 1) * lds + cols <= hi and src % 16 == 0
        assert (exp == 0) if not packed else plan["exps"].data_ptr() <= exp < plan["exps"].data_ptr() + 4 * plan["exps"].numel()
    table = ops.KvPlaceTable(plan["rec"], "cpu", ffi.KVS_WIDEN_E4M3 if packed else ffi.KVS_COPY,
                             [(p * k * plan["per"], c * plan["per"]) for p in range(2) for c in (1, 2)])
    assert all(f % 2 == 0 for f, _ in table.slices)
    garments = [1, 0]
    for bi, idx in enumerate(BLOCKS[order]):
        p = bi & 1
        apply_records(fill_records(cache.kv, n, G, want[p], k, S, cache.exps if packed else None, idx, list(range(len(idx))), garments, [0, 1]), packed, dtype)
        ncopies = _stage_and_place(plan, packed, dtype, idx, p, k)
        assert ncopies == len(idx) * 2 * 3 * 2                                             # per timestep and run of consecutive garments: [1], [0]
        assert _same_bytes(got[p], want[p]) and _same_bytes(got[1 - p], want[1 - p]), (order, bi)
    assert not (got[0][0][0][:192].view(torch.uint8) == 0x7f).all() and (got[0][0][0][2 * 192:3 * 192].view(torch.uint8) == 0x7f).all()
    # the arena and the exponents are used again by a later plan, and another index gives other copies into the same bytes
    again = staged_plan(cache, [0, 0, 0], k, S, got, "cpu", plan["arena"], None)
    assert again["arena"] is plan["arena"] and again["nbytes"] == k * per_step


def test_staged_plain_cache_without_an_index_copies_once_per_tensor():
    """No index, P = G = 2: a block of consecutive entries is ONE copy per cache tensor, a block by value one per timestep."""
    from idm_vton_amd.garment_cache import fill_records, staged_plan
    dtype, n, G, k = torch.bfloat16, 4, 2, 3
    cache = cache3(G, n, dtype)
    shapes = [(192, 64), (48, 128), (1040, 16)]
    want, got = _sets(shapes, k, G, dtype, 0x7f), _sets(shapes, k, G, dtype, 0x7f)
    plan = staged_plan(cache, None, k, G, [got], "cpu")
    assert plan["nbytes"] == k * G * sum(2 * N * Cc * 2 for N, Cc in shapes) == cache.nbytes * k // n and plan["exps"] is None and not plan["exps_copies"]
    for idx, ncopies in (([1, 2, 3], 6), ([2, 0], 12), ([3], 6)):
        apply_records(fill_records(cache.kv, n, G, want, k, G, None, idx, list(range(len(idx))), [0, 1], [0, 1]), False, dtype)
        assert _stage_and_place(plan, False, dtype, idx, 0, k) == ncopies
        assert _same_bytes(got, want), idx


@PACKED
def test_staged_shelf_of_three_sizes_fills_the_sets_as_the_kernel_transport_does(packed):
    """The three garments of tests/garment_support.py's shelf (smaller, the slot's size, smaller with ld' no multiple of 64), index [2, 0, 2, 1]:
    U = 3 parts in first-use order c, a, b into slots 0..2 of 4-slot sets.  Then a second call through the SAME sets and the same arena with
    the small garment c where the slot-sized b was: its zero tail has to replace b's values.  Against shelf_records from the parts (_shelf_fill's
    table), interpreted the same way."""
    from idm_vton_amd.garment_cache import shelf_records, staged_plan
    dtype, k, S = torch.float16, 3, 4
    shelf = cpu_shelf(packed)
    want, got = [_sets(SHELF_SLOT, k, S, dtype, 0x7f) for _ in range(2)], [_sets(SHELF_SLOT, k, S, dtype, 0x7f) for _ in range(2)]
    arena = exps = None
    esz = 1 if packed else 2
    sizes = []
    for keys in (["c", "a", "c", "b"], ["b", "c", "b", "b"], ["a", "c", "b", "b"]):
        cache, index = shelf.get(keys)
        U = cache.G
        plan = staged_plan(cache, index, k, S, got, "cpu", arena, exps if exps is not None and exps.shape[0] == U else None)
        need = k * sum(2 * N * Cc * esz for key in dict.fromkeys(keys) for N, Cc in SHELF_KINDS[key][1])
        assert plan["nbytes"] == need < cache.nbytes and plan["arena"].numel() >= need
        sizes.append(plan["arena"].numel())
        arena, exps = plan["arena"], plan["exps"]
        for d, s in plan["exps_copies"]:
            d.copy_(s)
        assert len(plan["exps_copies"]) == (U if packed else 0)
        zero = [r for r in record_fields(plan["rec"]) if r[0] == 0]
        assert zero and all(r[2] == 0 for r in zero) and plan["per"] % 2 == 0
        parts = [cache.parts[g] for g in dict.fromkeys(index)]
        for bi, idx in enumerate([[0], [1, 2], [3], [3, 1]]):
            p = bi & 1
            rec, per = shelf_records(parts, packed, want[p], k, S, idx, list(range(len(idx))), list(range(U)))
            assert per == plan["per"]
            apply_records(rec, packed, dtype)
            ncopies = _stage_and_place(plan, packed, dtype, idx, p, k)
            assert ncopies == U * 3 * 2 * (1 if idx != [3, 1] else 2)                    # one per part tensor; by value: per timestep
            assert _same_bytes(got[p], want[p]), (keys, bi)
    assert sizes[0] == sizes[1] and sizes[2] == sizes[0]                                   # c, a, b sized it; the smaller call and the same one use it again


# ------------------------------------------------------------------------------------------------------------------ the keyword
def test_host_transport_is_checked_before_anything_else():
    from idm_vton_amd.pipeline import TryonEngine
    eng = TryonEngine(None, None, None, device="cpu")
    assert TryonEngine.HOST_TRANSPORTS == ("kernel", "copy")
    assert eng.stats["garment_stage_copies"] == 0 == eng.stats["garment_stage_launches"] and eng.stats["garment_stream_launches"] == 0
    with pytest.raises(ValueError, match="host_transport='bogus'"):
        eng(host_transport="bogus")                          # (prepare's arguments are missing: it was not reached)
    with pytest.raises(ValueError, match="host_transport='staged'"):
        eng.denoise({}, host_transport="staged")
    with pytest.raises(ValueError, match="host_transport=None"):
        eng.denoise({}, use_graph=True, host_transport=None)
