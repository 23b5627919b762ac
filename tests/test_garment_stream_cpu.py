"""CPU tests of the host-resident garment cache: the host side of idmvton_kv_stream / idmvton_host_device_ptr -- exported, described by
idmvton_sizeof, additive to ABI version 9, every refusal raised before a launch (no GPU: the pointers are made up and never dereferenced) --,
the copy-mode descriptor records and the chunk prefix table against a plain-Python restatement, and GarmentPool(resident="host") on CPU
tensors (pageable there: the logic is what is under test)."""
import ctypes as C
import os

import pytest
import torch

from tests.garment_support import cache3, record_fields, same_packed


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_kv_stream_is_exported_described_and_additive():
    from idm_vton_amd import ffi
    L = ffi.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "idmvton_hip.h")).read()
    assert ("int idmvton_kv_stream(const idmvton_kv_stream_args* a, const idmvton_kv_stream_desc* host_desc, const int32_t* host_first, "
            "void* stream);") in header
    assert "int idmvton_host_device_ptr(const void* host, void** dev);" in header
    for sym in ("idmvton_kv_stream", "idmvton_host_device_ptr"):
        assert sym in ffi.SYMBOLS and hasattr(L, sym)
    assert L.idmvton_sizeof(b"idmvton_kv_stream_desc") == 40 == C.sizeof(ffi.KvStreamDesc) == C.sizeof(ffi.KvUnpackDesc)
    assert L.idmvton_sizeof(b"idmvton_kv_stream_args") == 32 == C.sizeof(ffi.KvStreamArgs)
    assert L.idmvton_abi_version() == 9 == ffi.ABI_VERSION
    assert (ffi.KVS_WIDEN_E4M3, ffi.KVS_COPY) == (0, 1) and "enum { IDMVTON_KVS_WIDEN_E4M3 = 0, IDMVTON_KVS_COPY = 1 };" in header


def _table(over=None, n=2, rows=(32, 600)):
    """A valid widening table of n runs rows[i] x 64 (made-up addresses; 128 and 2400 items: 1 and 3 chunks) with the fields of `over` =
    {(index, field): value} changed, and its prefix table."""
    from idm_vton_amd import ffi
    host = (ffi.KvStreamDesc * n)()
    for i in range(n):
        host[i].src, host[i].dst, host[i].exp = 0x100000 + 0x100000 * i, 0x800000 + 0x100000 * i, 0x40000 + 4 * i
        host[i].rows, host[i].cols, host[i].lds, host[i].ldd = rows[i], 64, 64, 64
    for (i, field), v in (over or {}).items():
        setattr(host[i], field, v)
    first = (C.c_int32 * (n + 1))(0, 1, 4)
    a = ffi.KvStreamArgs()
    a.dtype, a.mode, a.n, a.workgroups, a.desc, a.first = ffi.BF16, ffi.KVS_WIDEN_E4M3, n, 8, 0x200000, 0x300000
    return a, host, first


REFUSALS = [
    ("mode", {}, dict(mode=2), {}, -5, "mode 2"),
    ("mode negative", {}, dict(mode=-1), {}, -5, "mode -1"),
    ("workgroups 0", {}, dict(workgroups=0), {}, -5, r"workgroups=0 outside \[1, 1024\]"),
    ("workgroups 1025", {}, dict(workgroups=1025), {}, -5, r"workgroups=1025 outside \[1, 1024\]"),
    ("src alignment", {(1, "src"): 0x200008}, {}, {}, -3, "descriptor 1: src / dst not 16-byte aligned"),
    ("dst alignment", {(0, "dst"): 0x800002}, {}, {}, -3, "descriptor 0: src / dst not 16-byte aligned"),
    ("src null", {(1, "src"): None}, {}, {}, -5, "descriptor 1 has a null pointer"),
    ("exp null, widening", {(0, "exp"): None}, {}, {}, -5, "descriptor 0 has a null pointer"),
    ("cols % 16", {(1, "cols"): 40}, {}, {}, -1, "descriptor 1: rows=600 cols=40"),
    ("rows", {(0, "rows"): 0}, {}, {}, -1, "descriptor 0: rows=0 cols=64"),
    ("lds % 16", {(0, "lds"): 72}, {}, {}, -1, r"descriptor 0: lds=72 \(>= cols=64"),
    ("ldd % 8, widening", {(1, "ldd"): 68}, {}, {}, -1, r"descriptor 1: ldd=68 \(>= cols=64, a multiple of 8\)"),
    ("ldd % 16, copying", {(1, "ldd"): 72}, dict(mode=1), {}, -1, r"descriptor 1: ldd=72 \(>= cols=64, a multiple of 16\)"),
    ("host_first start", {}, {}, {0: 1}, -5, r"host_first\[0\]=1"),
    ("host_first middle", {}, {}, {1: 2}, -5, r"host_first\[1\]=2, the runs before descriptor 1 have 1 chunks"),
    ("host_first total", {}, {}, {2: 5}, -5, r"host_first\[2\]=5, the table has 4 chunks"),
    ("dtype", {}, dict(dtype=2), {}, -2, "dtype 2"),
    ("n", {}, dict(n=0), {}, -5, "n=0 outside"),
    ("device table null", {}, dict(desc=None), {}, -5, "null args / descriptor table / prefix table"),
    ("device prefix table null", {}, dict(first=None), {}, -5, "null args / descriptor table / prefix table"),
    ("device table alignment", {}, dict(desc=0x200008), {}, -3, "device descriptor table is not 16-byte aligned"),
]


@pytest.mark.parametrize("over,args,first_over,code,msg", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_kv_stream_refuses_on_the_host(over, args, first_over, code, msg):
    from idm_vton_amd import ffi
    L = ffi.lib()
    a, host, first = _table(over)
    for k, v in args.items():
        setattr(a, k, v)
    for i, v in first_over.items():
        first[i] = v
    assert L.idmvton_kv_stream(C.byref(a), C.cast(host, C.c_void_p), C.cast(first, C.c_void_p), None) == code
    with pytest.raises(RuntimeError, match=msg):
        ffi.call_kv_stream(a, host, first, 0)


def test_kv_stream_refuses_null_arguments():
    from idm_vton_amd import ffi
    L = ffi.lib()
    a, host, first = _table()
    h, f = C.cast(host, C.c_void_p), C.cast(first, C.c_void_p)
    assert L.idmvton_kv_stream(None, h, f, None) == -5
    assert L.idmvton_kv_stream(C.byref(a), None, f, None) == -5
    assert L.idmvton_kv_stream(C.byref(a), h, None, None) == -5 and b"null args" in L.idmvton_last_error()
    assert L.idmvton_host_device_ptr(None, None) == -5 and b"host_device_ptr: null argument" in L.idmvton_last_error()


def test_copy_mode_ignores_the_exponent_pointer():
    """In copy mode exp may be NULL and ldd is in bytes; with every other field valid the refusals end at the launch itself, which this
    machine cannot make -- so the table is checked up to its LAST check, the prefix total, by breaking only that."""
    from idm_vton_amd import ffi
    L = ffi.lib()
    a, host, first = _table({(0, "exp"): None, (1, "exp"): None})
    a.mode = ffi.KVS_COPY
    first[2] = 9
    assert L.idmvton_kv_stream(C.byref(a), C.cast(host, C.c_void_p), C.cast(first, C.c_void_p), None) == -5
    assert b"host_first[2]=9, the table has 4 chunks" in L.idmvton_last_error()


# ------------------------------------------------------------------------------------------------------------------ records


def _restated(src, dst, exps, n, G, k, S, entries, tslots, garments, gslots, address):
    """fill_records in plain Python: (src, dst, exp, rows, cols, lds, ldd) per (timestep, garment, feature, K | V^T)."""
    out = []
    esz = dst[0][0].element_size()
    for i, j in zip(entries, tslots):
        for g, u in zip(garments, gslots):
            for f, ((sk, sv), (dk, dv)) in enumerate(zip(src, dst)):
                for t, (s, d, rows, cols) in enumerate(((sk, dk, sk.shape[0] // (n * G), sk.shape[1]), (sv, dv, sv.shape[1], sv.shape[2]))):
                    unit = rows * cols
                    if exps is None:                     # copy mode: bytes
                        out.append((address(s) + (i * G + g) * unit * esz, d.data_ptr() + (j * S + u) * unit * esz, 0, rows, cols * esz, cols * esz, cols * esz))
                    else:
                        out.append((address(s) + (i * G + g) * unit, d.data_ptr() + (j * S + u) * unit * esz, address(exps) + 4 * ((g * len(src) + f) * 2 + t),
                                    rows, cols, cols, cols))
    return out


def test_copy_mode_records_and_prefix_table_against_a_restatement():
    """A 3-feature synthetic cache, P = 4 persons with garment_index [2, 0, 2, 1]: the U = 3 distinct garments in first-use order into slots
    0..2 of 4-slot sets, entries by value.  Copy form (16-bit source: byte units, no exponent) and widening form, with an `address` of the
    caller's (asked once per source tensor); the prefix table and KvStreamTable's per-slice tables against ceil(items / 1024) summed up."""
    from idm_vton_amd import ffi, ops
    from idm_vton_amd.garment_cache import alloc_kv, fill_records, kv_shapes, slot_run
    c = cache3()
    n, G, k, S = 4, 3, 3, 4
    garments = list(dict.fromkeys([2, 0, 2, 1]))
    assert garments == [2, 0, 1]
    gslots, entries, tslots = [0, 1, 2], [3, 1, 2], [0, 1, 2]
    dst = alloc_kv([((a[0] // G * S,) + a[1:], (b[0] // G * S,) + b[1:], torch.float16) for a, b, _ in kv_shapes(c.kv)], n, k, "cpu")
    asked = []

    def address(t):
        asked.append(t.data_ptr())
        return t.data_ptr() + 0x10000000                 # a device-visible address need not be the host one
    rec = fill_records(c.kv, n, G, dst, k, S, None, entries, tslots, garments, gslots, address=address)
    assert rec.dtype == torch.int64 and tuple(rec.shape) == (3 * 3 * 3 * 2, 5) and rec.is_contiguous()
    assert sorted(asked) == sorted(t.data_ptr() for kvf in c.kv for t in kvf)                # once per tensor
    assert record_fields(rec) == _restated(c.kv, dst, None, n, G, k, S, entries, tslots, garments, gslots, lambda t: t.data_ptr() + 0x10000000)
    # the default address is data_ptr(): the records name slot_run's views, in bytes
    rec0 = fill_records(c.kv, n, G, dst, k, S, None, entries, tslots, garments, gslots)
    descs = (ffi.KvStreamDesc * rec0.shape[0]).from_address(rec0.data_ptr())
    at = 0
    for i, j in zip(entries, tslots):
        for g, u in zip(garments, gslots):
            for (sk, sv), (dk, dv) in zip(slot_run(c.kv, n, G, i, g), slot_run(dst, k, S, j, u)):
                for s, d in ((sk, dk), (sv[0], dv[0])):
                    x = descs[at]
                    assert (x.src, x.dst, x.exp) == (s.data_ptr(), d.data_ptr(), None)
                    assert (x.rows, x.cols, x.lds, x.ldd) == (s.shape[0], 2 * s.shape[1], 2 * s.stride(0), 2 * d.stride(0))
                    at += 1
    # the widening form is what it was, with the caller's addresses for bytes and exponents
    p = c.pack()
    asked.clear()
    recw = fill_records(p.kv, n, G, dst, k, S, p.exps, entries, tslots, garments, gslots, address=address)
    assert len(asked) == 2 * len(p.kv) + 1
    assert record_fields(recw) == _restated(p.kv, dst, p.exps, n, G, k, S, entries, tslots, garments, gslots, lambda t: t.data_ptr() + 0x10000000)
    assert record_fields(fill_records(p.kv, n, G, dst, k, S, p.exps, entries, tslots, garments, gslots)) == \
        _restated(p.kv, dst, p.exps, n, G, k, S, entries, tslots, garments, gslots, lambda t: t.data_ptr())
    # prefix tables: 16-byte items per record -> chunks of 1024
    items = [r[3] * (r[4] // 16) for r in record_fields(rec)]
    chunks = [(it + 1023) // 1024 for it in items]
    assert max(chunks) > 1 and min(chunks) == 1
    want = [0]
    for ch in chunks:
        want.append(want[-1] + ch)
    assert ops.KV_STREAM_CHUNK == 1024
    assert ops.kv_stream_first(torch.tensor(items)).tolist() == want and ops.kv_stream_first(torch.tensor(items)).dtype == torch.int32
    per = 3 * 3 * 2                                      # records per timestep: garments x features x (K, V^T)
    table = ops.KvStreamTable(rec, "cpu", ffi.KVS_COPY, [(0, per), (per, 2 * per)])
    assert table.first_host.dtype == torch.int32 and table.first_at == [0, per + 1]
    assert table.first_host[:per + 1].tolist() == want[:per + 1]
    assert table.first_host[per + 1:].tolist() == [w - want[per] for w in want[per:]]
    assert ops.KvStreamTable(rec, "cpu", ffi.KVS_COPY).first_host.tolist() == want
    with pytest.raises(ValueError, match="an even first index"):
        ops.KvStreamTable(rec, "cpu", ffi.KVS_COPY, [(1, 4)])
    with pytest.raises(ValueError, match="an even first index"):
        ops.KvStreamTable(rec, "cpu", ffi.KVS_COPY, [(0, rec.shape[0] + 1)])


def test_a_pageable_tensor_never_gets_an_address():
    from idm_vton_amd import ops
    with pytest.raises(ValueError, match="pin_memory"):
        ops.stream_address(torch.zeros(64, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------------------------ cache and pool
def test_host_resident_flag_and_put_on_cpu_tensors():
    c = cache3()
    assert c.host_resident and c.pack().host_resident and c.select([1]).host_resident and c.take(0).host_resident
    q = c.select([0, 1, 2])
    ptrs = [k.data_ptr() for k, _ in q.kv]
    q.put(0, c.take(2))
    assert ptrs == [k.data_ptr() for k, _ in q.kv]
    assert all(torch.equal(a, b) and torch.equal(x, y) for (a, x), (b, y) in zip(q.kv, c.select([2, 1, 2]).kv))
    p = c.pack().select([0, 1, 2])
    p.put(1, c.take(0))                                  # a 16-bit source into a packed host cache: packed first
    assert same_packed(p, c.select([0, 0, 2]).pack())


@pytest.mark.parametrize("packed", [False, True], ids=["16bit", "packed"])
def test_host_pool_lru_equals_the_device_style_pool(packed):
    from idm_vton_amd.garment_cache import GarmentPool
    ones = {key: cache3(G=1, seed=s) for s, key in enumerate("abcde")}
    if packed:
        ones = {key: one.pack() for key, one in ones.items()}
    pools = [GarmentPool(3, like=ones["a"]), GarmentPool(3, like=ones["a"], resident="host")]
    assert pools[0].resident == "device" and pools[1].resident == "host" and pools[1].cache.host_resident and pools[1].cache.packed == packed
    assert pools[1].cache.G == 3 and pools[0].cache.nbytes == pools[1].cache.nbytes
    calls = [[], []]
    for batch in (["a", "b"], ["c", "a", "a"], ["d"], ["b", "d", "e"], ["a", "e"]):
        got = []
        for pool, log in zip(pools, calls):
            got.append(pool.get(batch, encode=lambda key, log=log: (log.append(key), ones[key])[1]))
        assert got[0] == got[1], batch
        assert pools[0].slots() == pools[1].slots() and list(pools[0].slots()) == list(pools[1].slots()), batch
        assert pools[0].stats == pools[1].stats
    assert calls[0] == calls[1] and pools[1].stats["evicted"] >= 2 and not pools[1].host
    for key, slot in pools[1].slots().items():
        a, b = pools[0].cache.take(slot), pools[1].cache.take(slot)
        assert all(torch.equal(x, y) and torch.equal(u, v) for (x, u), (y, v) in zip(a.kv, b.kv))
        assert all(torch.equal(x, y) and torch.equal(u, v) for (x, u), (y, v) in zip(b.kv, ones[key].kv)), key
        assert not packed or torch.equal(b.exps, ones[key].exps)
    with pytest.raises(ValueError, match="distinct garments"):
        pools[1].get(["a", "b", "c", "d"], encode=lambda key: ones[key])


def test_host_pool_refuses_spill_and_mixed_sizes():
    from idm_vton_amd.garment_cache import GarmentPool
    one = cache3(G=1)
    with pytest.raises(ValueError, match=r'resident="host" cannot be combined with spill'):
        GarmentPool(2, like=one, spill=True, resident="host")
    with pytest.raises(ValueError, match=r'resident="host" cannot be combined with spill'):
        GarmentPool(2, like=one, spill=1, resident="host")
    with pytest.raises(ValueError, match=r'resident="host" cannot be combined with mixed_sizes'):
        GarmentPool(2, like=one, mixed_sizes=True, resident="host")
    with pytest.raises(ValueError, match="resident='hbm'"):
        GarmentPool(2, like=one, resident="hbm")
    assert GarmentPool(2, like=one, spill=1, mixed_sizes=True).resident == "device"
