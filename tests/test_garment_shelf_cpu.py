"""CPU tests of the garment shelf: the host side of idmvton_kv_fill -- exported, additive to ABI version 9, every refusal raised before a
launch (no GPU: the pointers are made up and never dereferenced) --, shelf_records against a plain-Python restatement AND against an
interpreter that applies a record table to CPU tensors by address, and GarmentShelf / ShelvedGarmentCache on CPU tensors (pageable there: the
logic is what is under test)."""
import ctypes as C
import os

import pytest
import torch

from tests.garment_support import N_T, PACKED, SHELF_KINDS, SHELF_SLOT, apply_records, cpu_shelf, record_fields, same_packed, shelf_like, shelf_one


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_kv_fill_is_exported_declared_and_additive():
    from idm_vton_amd import ffi
    L = ffi.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "idmvton_hip.h")).read()
    assert ("int idmvton_kv_fill(const idmvton_kv_stream_args* a, const idmvton_kv_stream_desc* host_desc, const int32_t* host_first, "
            "void* stream);") in header
    assert "idmvton_kv_fill" in ffi.SYMBOLS and hasattr(L, "idmvton_kv_fill") and callable(ffi.call_kv_fill)
    assert L.idmvton_abi_version() == 9 == ffi.ABI_VERSION
    # no new struct, and none changed its size: the sizes the earlier additions pinned
    assert L.idmvton_sizeof(b"idmvton_kv_stream_desc") == 40 == L.idmvton_sizeof(b"idmvton_kv_unpack_desc") == C.sizeof(ffi.KvStreamDesc)
    assert L.idmvton_sizeof(b"idmvton_kv_stream_args") == 32 == C.sizeof(ffi.KvStreamArgs)
    assert L.idmvton_sizeof(b"idmvton_kv_unpack_args") == C.sizeof(ffi.KvUnpackArgs)
    assert L.idmvton_sizeof(b"idmvton_kv_fill_args") == -1 and "idmvton_kv_fill_args" not in header
    for name, st in ffi.STRUCTS.items():
        assert L.idmvton_sizeof(name.encode()) == C.sizeof(st), name


def _table(over=None):
    """A valid widening table of 3 runs with made-up addresses -- a data run 32 x 64 (128 items, 1 chunk), a ZERO run 600 x 64 (2400 items, 3
    chunks; src, exp NULL, lds 0), a data run 16 x 64 -- with the fields of `over` = {(index, field): value} changed, and its prefix table."""
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
    a.dtype, a.mode, a.n, a.workgroups, a.desc, a.first = ffi.BF16, ffi.KVS_WIDEN_E4M3, n, 8, 0x200000, 0x300000
    return a, host, first


REFUSALS = [
    ("zero run rows 0", {(1, "rows"): 0}, {}, {}, -1, "kv_fill: descriptor 1: rows=0 cols=64"),
    ("zero run cols 8", {(1, "cols"): 8}, {}, {}, -1, r"kv_fill: descriptor 1: rows=600 cols=8 \(rows >= 1, cols a multiple of 16\)"),
    ("zero run cols % 16", {(1, "cols"): 40}, {}, {}, -1, "kv_fill: descriptor 1: rows=600 cols=40"),
    ("zero run ldd < cols", {(1, "ldd"): 48}, {}, {}, -1, r"kv_fill: descriptor 1: ldd=48 \(>= cols=64, a multiple of 8\)"),
    ("zero run ldd % 16, copying", {(1, "ldd"): 72}, dict(mode=1), {}, -1, r"kv_fill: descriptor 1: ldd=72 \(>= cols=64, a multiple of 16\)"),
    ("zero run dst alignment", {(1, "dst"): 0x900008}, {}, {}, -3, "kv_fill: descriptor 1: src / dst not 16-byte aligned"),
    ("zero run dst null", {(1, "dst"): None}, {}, {}, -5, r"kv_fill: descriptor 1 has a null pointer \(dst of a zero run\)"),
    ("data run exp null, widening", {(2, "exp"): None}, {}, {}, -5, "kv_fill: descriptor 2 has a null pointer"),
    ("data run lds % 16", {(0, "lds"): 72}, {}, {}, -1, r"kv_fill: descriptor 0: lds=72 \(>= cols=64"),
    ("host_first middle", {}, {}, {2: 3}, -5, r"kv_fill: host_first\[2\]=3, the runs before descriptor 2 have 4 chunks"),
    ("host_first total", {}, {}, {3: 6}, -5, r"kv_fill: host_first\[3\]=6, the table has 5 chunks"),
    ("workgroups 0", {}, dict(workgroups=0), {}, -5, r"kv_fill: workgroups=0 outside \[1, 1024\]"),
    ("mode 7", {}, dict(mode=7), {}, -5, "kv_fill: mode 7"),
]


@pytest.mark.parametrize("over,args,first_over,code,msg", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_kv_fill_refuses_on_the_host(over, args, first_over, code, msg):
    from idm_vton_amd import ffi
    L = ffi.lib()
    a, host, first = _table(over)
    for k, v in args.items():
        setattr(a, k, v)
    for i, v in first_over.items():
        first[i] = v
    assert L.idmvton_kv_fill(C.byref(a), C.cast(host, C.c_void_p), C.cast(first, C.c_void_p), None) == code
    with pytest.raises(RuntimeError, match=msg):
        ffi.call_kv_fill(a, host, first, 0)


def test_a_table_of_zero_runs_only_is_valid_up_to_its_last_check():
    """Every field valid, the refusals end at the launch itself, which this machine cannot make: so a table of zero runs only (src, exp NULL,
    lds 0, in both modes) is checked up to its LAST check, the prefix total, by breaking only that.  idmvton_kv_stream refuses the same table."""
    from idm_vton_amd import ffi
    L = ffi.lib()
    for mode in (ffi.KVS_WIDEN_E4M3, ffi.KVS_COPY):
        a, host, first = _table({(i, f): v for i in (0, 2) for f, v in (("src", None), ("exp", None), ("lds", 0))})
        a.mode = mode
        first[3] = 9
        assert L.idmvton_kv_fill(C.byref(a), C.cast(host, C.c_void_p), C.cast(first, C.c_void_p), None) == -5
        assert b"kv_fill: host_first[3]=9, the table has 5 chunks" in L.idmvton_last_error()
        assert L.idmvton_kv_stream(C.byref(a), C.cast(host, C.c_void_p), C.cast(first, C.c_void_p), None) == -5
        assert b"kv_stream: descriptor 0 has a null pointer" in L.idmvton_last_error()


# ------------------------------------------------------------------------------------------------------------------ garments


# ------------------------------------------------------------------------------------------------------------------ records
def _restated(parts, packed, dst, k, S, entries, tslots, gslots, address):
    """shelf_records in plain Python: (src, dst, exp, rows, cols, lds, ldd) per (timestep, garment, feature, K | V^T | zero tail), every
    timestep padded to an even count with its record of fewest items."""
    out = []
    esz = dst[0][0].element_size()
    su = 1 if packed else esz
    du = 1 if packed else esz                            # ldd: elements when widening, bytes when copying
    for i, j in zip(entries, tslots):
        step = []
        for part, u in zip(parts, gslots):
            n = len(part.timesteps)
            for f, ((sk, sv), (dk, dv)) in enumerate(zip(part.kv, dst)):
                Nf, Cc, ldf = sk.shape[0] // n, sk.shape[1], sv.shape[2]
                N, ld = dk.shape[0] // (k * S), dv.shape[2]
                ex = [address(part.exps) + 4 * (f * 2 + t) for t in range(2)] if packed else [0, 0]
                step.append((address(sk) + i * Nf * Cc * su, dk.data_ptr() + (j * S + u) * N * Cc * esz, ex[0], Nf, Cc * su, Cc * su, Cc * du))
                vdst = dv.data_ptr() + (j * S + u) * Cc * ld * esz
                step.append((address(sv) + i * Cc * ldf * su, vdst, ex[1], Cc, ldf * su, ldf * su, ld * du))
                if ldf < ld:
                    step.append((0, vdst + ldf * esz, 0, Cc, (ld - ldf) * su, (ld - ldf) * su, ld * du))
        if len(step) % 2:
            step.append(min(step, key=lambda r: r[3] * (r[4] // 16)))
        out += step
    return out


@PACKED
@pytest.mark.parametrize("garments", [[2, 0], [2, 1]], ids=["c,a", "c,b"])
def test_shelf_records_against_a_restatement_and_an_interpreter(packed, garments):
    """Three garments (smaller, the slot's size, smaller with ld' no multiple of 64), 4 timesteps, entries by value in non-consecutive order,
    garments [2, 0] into slots [0, 1] of a 3-slot set ([2, 1]: an odd record count per timestep, padded).  The interpreter's set against
    slotted(): V^T everywhere, K on a garment's own rows; K rows beyond and the slot nobody fills keep what the set held -- zeros, then 0x7f
    bytes (e4m3's NaN, a NaN pattern in fp16 too), so a record that wrote too much or too little shows."""
    from idm_vton_amd import ffi, ops
    from idm_vton_amd.garment_cache import shelf_records, slot_run
    dtype = torch.float16
    shelf = cpu_shelf(packed)
    cache, index = shelf.get(["a", "b", "c"])
    assert index == [0, 1, 2] and cache.G == 3 and cache.packed == packed
    k, S, entries, tslots, gslots = 3, 3, [3, 1, 2], [0, 1, 2], [0, 1]
    parts = [cache.parts[g] for g in garments]
    ref = cache.slotted()
    n = len(ref.timesteps)
    for fill in (0x00, 0x7f):
        dst = [(torch.empty(k * S * N, Cc, dtype=dtype), torch.empty(k * S, Cc, N, dtype=dtype)) for N, Cc in SHELF_SLOT]
        for t in (t for kvf in dst for t in kvf):
            t.view(torch.uint8).fill_(fill)
        asked = []

        def address(t):
            asked.append(t.data_ptr())
            return t.data_ptr()
        rec, per = shelf_records(parts, packed, dst, k, S, entries, tslots, gslots, address=address)
        want = sorted(t.data_ptr() for p in parts for kvf in p.kv for t in kvf) + ([p.exps.data_ptr() for p in parts] if packed else [])
        assert sorted(asked) == sorted(want)                                                 # once per tensor
        assert rec.dtype == torch.int64 and rec.is_contiguous() and per % 2 == 0 and tuple(rec.shape) == (len(entries) * per, 5)
        assert record_fields(rec) == _restated(parts, packed, dst, k, S, entries, tslots, gslots, lambda t: t.data_ptr())
        zero = [r for r in record_fields(rec) if r[0] == 0]
        assert zero and all(r[2] == 0 for r in zero)
        raw = sum(3 if ld1 < ld else 2 for g in garments for (ld1, _), (ld, _) in zip(SHELF_KINDS["abc"[g]][1], SHELF_SLOT))
        assert per == raw + raw % 2 and (raw % 2 == 1) == (garments == [2, 1])
        # every launched slice starts at an even record index, and the prefix tables count a zero run like a data run
        table = ops.KvFillTable(rec, "cpu", ffi.KVS_WIDEN_E4M3 if packed else ffi.KVS_COPY, [(t * per, per) for t in range(len(entries))])
        assert all(f % 2 == 0 for f, _ in table.slices) and table.ENTRY == "kv_fill"
        items = [r[3] * (r[4] // 16) for r in record_fields(rec)]
        assert table.items.tolist() == items
        assert table.first_host[:per + 1].tolist() == [sum((it + 1023) // 1024 for it in items[:m]) for m in range(per + 1)]
        data = sum(it for it, r in zip(items, record_fields(rec)) if r[0])
        assert table.link_bytes() == 16.0 * data and table.bytes_moved(0, table.n) == 16.0 * data + (32.0 if packed else 16.0) * sum(items)
        with pytest.raises(ValueError, match="an even first index"):
            ops.KvFillTable(rec, "cpu", ffi.KVS_COPY, [(1, 2)])
        apply_records(rec, packed, dtype)
        pattern = torch.full((1,), fill, dtype=torch.uint8)
        for i, j in zip(entries, tslots):
            for u in range(S):
                g = garments[u] if u < len(garments) else None
                for f, (dk, dv) in enumerate(slot_run(dst, k, S, j, u)):
                    if g is None:                            # a slot no garment of the call fills: untouched
                        assert (dk.view(torch.uint8) == pattern).all() and (dv.view(torch.uint8) == pattern).all()
                        continue
                    rk, rv = slot_run(ref.kv, n, ref.G, i, g)[f]
                    Nf = SHELF_KINDS["abc"[g]][1][f][0]
                    assert torch.equal(dv.view(torch.int16), rv.view(torch.int16)), (fill, i, u, f)
                    assert torch.equal(dk[:Nf].view(torch.int16), rk[:Nf].view(torch.int16)), (fill, i, u, f)
                    assert (dk[Nf:].view(torch.uint8) == pattern).all(), (fill, i, u, f)
                    assert (rv[..., Nf:] == 0).all()         # (the reference's own tail: what _put_slotted wrote)


def test_tables_launch_through_their_own_entry_point(monkeypatch):
    """KvStreamTable launches idmvton_kv_stream, KvFillTable idmvton_kv_fill, with the slice's host and device addresses (the calls are
    recorded, not made: no GPU)."""
    from idm_vton_amd import ffi, ops
    rec = torch.tensor([[4096, 8192, 64, 4 | (64 << 32), 64 | (64 << 32)], [0, 16384, 0, 2 | (16 << 32), 16 | (64 << 32)]] * 2)
    calls = []
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "PROFILE", None)
    for name in ("kv_stream", "kv_fill"):
        monkeypatch.setattr(ops.ffi, "call_" + name, lambda a, desc, first, stream, name=name: calls.append((name, a.n, a.mode, a.workgroups, desc, first)))
    for cls, name in ((ops.KvStreamTable, "kv_stream"), (ops.KvFillTable, "kv_fill")):
        t = cls(rec, "cpu", ffi.KVS_WIDEN_E4M3, [(0, 2), (2, 2)])
        t.launch(torch.float16, 1, 3)
        assert calls.pop() == (name, 2, ffi.KVS_WIDEN_E4M3, 3, t.host.data_ptr() + 80, t.first_host.data_ptr() + 12)
        t.launch(torch.bfloat16)
        assert calls.pop()[:4] == (name, 2, ffi.KVS_WIDEN_E4M3, ops.KV_STREAM_WORKGROUPS)


def test_kv_pad_even_repeats_the_smallest_record():
    from idm_vton_amd import ops
    rec = torch.tensor([[16, 32, 0, 4 | (64 << 32), 64 | (64 << 32)], [0, 64, 0, 2 | (16 << 32), 16 | (64 << 32)], [48, 96, 0, 3 | (32 << 32), 32 | (64 << 32)]])
    out = ops.kv_pad_even(rec)
    assert out.shape == (4, 5) and torch.equal(out[:3], rec) and torch.equal(out[3], rec[1])
    assert ops.kv_pad_even(out) is out


# ------------------------------------------------------------------------------------------------------------------ shelf
@PACKED
def test_shelf_add_get_lru_and_eviction(packed):
    from idm_vton_amd.garment_cache import GarmentShelf, PackedGarmentCache, ShelvedGarmentCache
    shelf = cpu_shelf(packed)
    assert len(shelf) == 3 and "a" in shelf and "z" not in shelf and shelf.keys() == ["a", "b", "c"]
    sizes = {key: shelf._parts[key].nbytes for key in "abc"}
    assert shelf.nbytes == sum(sizes.values()) and sizes["a"] < sizes["b"] and sizes["c"] < sizes["b"]
    esz = 1 if packed else 2
    for key in "abc":                                    # compact: the garment's own rows and positions, nothing of the slot
        want = sum(2 * N_T * N * Cc * esz for N, Cc in SHELF_KINDS[key][1]) + (4 * 3 * 2 if packed else 0)
        assert sizes[key] == want and isinstance(shelf._parts[key], PackedGarmentCache) == packed
    cache, index = shelf.get(["c", "a", "c"])
    assert isinstance(cache, ShelvedGarmentCache) and index == [0, 1, 0] and cache.G == 2 and cache.sizes == [(9, 5), (8, 12)]
    assert (cache.gh, cache.gw) == (16, 12) and cache.host_resident and cache.packed == packed and cache.kv == []
    assert cache.slot_shapes == [((N, Cc), (Cc, N)) for N, Cc in SHELF_SLOT]
    assert cache.nbytes == sizes["a"] + sizes["c"] < 2 * sizes["b"]                           # smaller than G x slot bytes
    assert shelf.keys() == ["b", "c", "a"] and shelf.stats == dict(hits=2, encoded=0, restored=0, evicted=0)
    assert "slots of 16x12" in repr(cache) and "ShelvedGarmentCache(G=2" in repr(cache)
    # encode: once per missing distinct key; KeyError without one, before anything changes
    calls = []
    enc = lambda key: (calls.append(key), shelf_one("a", seed=ord(key)))[1]
    with pytest.raises(KeyError, match="'x' is not on the shelf"):
        shelf.get(["a", "x"])
    cache2, index2 = shelf.get(["x", "b", "x", "y"], encode=enc)
    assert calls == ["x", "y"] and index2 == [0, 1, 0, 2] and shelf.keys() == ["c", "a", "x", "b", "y"] and shelf.stats["encoded"] == 2
    # nothing is added or evicted if encode raises

    def boom(key):
        raise RuntimeError("out of memory")
    before = (shelf.keys(), dict(shelf.stats), shelf.nbytes)
    with pytest.raises(RuntimeError, match="out of memory"):
        shelf.get(["c", "q"], encode=boom)
    assert (shelf.keys(), dict(shelf.stats), shelf.nbytes) == before
    # max_bytes: the least recently used garments the batch does not name go until the shelf fits
    small = GarmentShelf(shelf_like(), storage="e4m3" if packed else "native", max_bytes=2 * sizes["b"] + 100)
    for key in "abc":
        small.add(key, shelf_one(key))
    kept, _ = small.get(["a"])                               # a is now the most recently used
    _, idx = small.get(["d", "b"], encode=lambda key: shelf_one("c", seed=7))
    assert idx == [0, 1] and small.keys() == ["a", "d", "b"] and small.stats["evicted"] == 1 and small.nbytes <= small.max_bytes
    _, idx = small.get(["e"], encode=lambda key: shelf_one("b", seed=8))
    assert small.keys() == ["b", "e"] and small.stats["evicted"] == 3                         # a and d went, in that order; never e
    with pytest.raises(ValueError, match="the batch alone holds"):
        small.get(["f", "g", "b"], encode=lambda key: shelf_one("b", seed=9))
    assert small.keys() == ["b", "e"]
    # the cache keeps its parts alive whatever the shelf does
    part = kept.parts[0]
    small.remove("b"); small.remove("nothing")
    assert small.keys() == ["e"] and kept.parts[0] is part and torch.equal(kept.take(0).kv[0][0], part.kv[0][0])


def test_shelf_packs_a_16bit_garment_on_its_way_in_and_takes_packed_ones():
    from idm_vton_amd.garment_cache import GarmentShelf
    shelf = GarmentShelf(shelf_like(), storage="e4m3")
    shelf.add("a", shelf_one("a"))
    shelf.add("a2", shelf_one("a").pack())
    assert same_packed(shelf._parts["a"], shelf_one("a").pack()) and same_packed(shelf._parts["a2"], shelf._parts["a"])
    one_slot = shelf_like()                                   # a one-slot slotted cache holding a small garment: taken at its compact size
    one_slot.put(0, shelf_one("c"))
    shelf.add("c", one_slot)
    assert same_packed(shelf._parts["c"], shelf_one("c").pack()) and (shelf._parts["c"].gh, shelf._parts["c"].gw) == (9, 5)


def test_shelf_refusals():
    from idm_vton_amd.garment_cache import GarmentCache, GarmentShelf
    shelf = GarmentShelf(shelf_like(), storage="native")
    with pytest.raises(ValueError, match="storage='fp4'"):
        GarmentShelf(shelf_like(), storage="fp4")
    for field, kw in (("timesteps", dict(timesteps=[900, 700, 500, 100])), ("h", dict(h=32)), ("w", dict(w=8)), ("f8_exp", dict(f8_exp=(1, 2, 2))),
                      ("weights_id", dict(weights_id="w1"))):
        with pytest.raises(ValueError, match=f"GarmentShelf add: {field} mismatch"):
            shelf.add("x", shelf_one("a", **kw))
    with pytest.raises(ValueError, match="GarmentShelf add: dtype mismatch"):
        shelf.add("x", shelf_one("a", dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="GarmentShelf add: attn_fp8 mismatch"):
        shelf.add("x", shelf_one("a", attn_fp8=True))
    with pytest.raises(ValueError, match="GarmentShelf add: packed mismatch"):
        shelf.add("x", shelf_one("a").pack())
    with pytest.raises(ValueError, match="GarmentShelf add: G mismatch"):
        shelf.add("x", GarmentCache.cat([shelf_one("a"), shelf_one("a")]))
    big = shelf_one("b")
    big.kv[2] = (torch.zeros(N_T * 1056, 16, dtype=torch.float16), torch.zeros(N_T, 16, 1056, dtype=torch.float16))
    with pytest.raises(ValueError, match=r"does not fit \(feature 2: .*K rows 1056 x 16.*holds 1040 x 16"):
        shelf.add("x", big)
    wide = shelf_one("a")
    wide.kv[0] = (torch.zeros(N_T * 96, 80, dtype=torch.float16), torch.zeros(N_T, 80, 96, dtype=torch.float16))
    with pytest.raises(ValueError, match=r"does not fit \(feature 0"):
        shelf.add("x", wide)
    two = shelf_one("a")
    two.kv = two.kv[:2]
    with pytest.raises(ValueError, match=r"does not fit \(2 features against 3\)"):
        shelf.add("x", two)
    assert len(shelf) == 0 and shelf.nbytes == 0


@PACKED
def test_shelved_cache_methods(packed):
    from idm_vton_amd.garment_cache import GarmentCache
    shelf = cpu_shelf(packed)
    cache, _ = shelf.get(["a", "b", "c"])
    kw = dict(timesteps=[700, 300], h=16, w=12, dtype=torch.float16, attn_fp8=False, f8_exp=(2, 2, 2), weights_id="w0")
    assert cache.check(persons=4, garment_index=[2, 0, 2, 1], **kw) == ([1, 3], [2, 0, 2, 1])
    with pytest.raises(ValueError, match="resolution mismatch"):
        cache.check(persons=1, garment_index=[0], **{**kw, "h": 32})
    with pytest.raises(ValueError, match="garment_index mismatch"):
        cache.check(persons=1, garment_index=[3], **kw)
    assert cache.garment_ids([1, 1], 2) == [1, 1] and cache.garment_sizes([2, 0]) == [(9, 5), (8, 12)]
    other = cache.for_person_size(32, 24)
    assert (other.h, other.w) == (32, 24) and other.parts == cache.parts and other.sizes == cache.sizes
    assert other.check(persons=1, garment_index=[1], **{**kw, "h": 32, "w": 24}) == ([1, 3], [1])
    # methods that need one tensor list say so by name
    for name, args in (("put", (0, shelf_one("a"))), ("save", ("x.safetensors",)), ("pack", ()), ("unpack", ()), ("repeat_garments", (2,)), ("run", (0,)),
                       ("step", (0,)), ("to", ("cpu",)), ("cat", ([cache, cache],))):
        with pytest.raises(ValueError, match=f"ShelvedGarmentCache {name}:"):
            getattr(cache, name)(*args)
    # take: a copy of the part; select: the same parts in another order; slotted: empty slots + put(take(g))
    for g, key in enumerate("abc"):
        t = cache.take(g)
        assert t.G == 1 and t.packed == packed and (t.gh, t.gw) == SHELF_KINDS[key][0] and t.kv[0][0].data_ptr() != cache.parts[g].kv[0][0].data_ptr()
        assert all(torch.equal(x, y) and torch.equal(u, v) for (x, u), (y, v) in zip(t.kv, cache.parts[g].kv))
        assert not packed or torch.equal(t.exps, cache.parts[g].exps)
    with pytest.raises(ValueError, match="take: slot mismatch"):
        cache.take(3)
    sel = cache.select([2, 0, 2])
    assert sel.G == 3 and sel.sizes == [(9, 5), (8, 12), (9, 5)] and sel.parts[0] is cache.parts[2] and sel.parts[2] is cache.parts[2]
    ref = cache.slotted()
    assert type(ref) is GarmentCache
    assert ref.sizes == cache.sizes and (ref.gh, ref.gw) == (16, 12) and ref.G == 3 and not ref.packed and ref.kv[0][0].dtype == torch.float16
    by_hand = GarmentCache(**{**shelf_like()._args(), "G": 3, "sizes": [(16, 12)] * 3, "rows": None,
                              "kv": [(torch.zeros(N_T * 3 * N, Cc, dtype=torch.float16), torch.zeros(N_T * 3, Cc, N, dtype=torch.float16)) for N, Cc in SHELF_SLOT]})
    for g in range(3):
        one = cache.take(g)
        by_hand.put(g, one.unpack() if packed else one)
    assert all(torch.equal(x, y) and torch.equal(u, v) for (x, u), (y, v) in zip(ref.kv, by_hand.kv))
    s2 = sel.slotted()
    for f in range(3):                                   # select round trip: slot 0 of the selection is slot 2 of the cache, at every timestep
        for i in range(N_T):
            from idm_vton_amd.garment_cache import slot_run
            a, b = slot_run(s2.kv, N_T, 3, i, 0)[f], slot_run(ref.kv, N_T, 3, i, 2)[f]
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------------------ what stays
def test_the_locked_refusals_still_hold():
    from idm_vton_amd.garment_cache import GarmentPool
    one = shelf_one("b")
    with pytest.raises(ValueError, match=r'resident="host" cannot be combined with mixed_sizes'):
        GarmentPool(2, like=one, mixed_sizes=True, resident="host")
