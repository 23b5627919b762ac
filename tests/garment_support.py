"""What the garment tests share on the host side: parametrisation marks and constants, the made-up attention argument structs of the
refusal tests, synthetic GarmentCache / GarmentShelf builders on CPU tensors, the record interpreter (`record_fields`, `apply_records`) and
the cache comparisons.  Importing this module needs no GPU and does not load the native library: everything of the package is imported inside the
function that uses it.  The GPU side (models, engines, operands, the boundary pipeline) is tests/engine_support.py."""
import ctypes as C
import types

import pytest
import torch

DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
PACKED = pytest.mark.parametrize("packed", [False, True], ids=["16bit", "packed"])
FINITE = torch.tensor([b for b in range(256) if b & 0x7f != 0x7f], dtype=torch.uint8)      # all but the two NaN bytes 0x7f / 0xff

# (Nq, garment keys): 320 query rows are not a multiple of any kernel's 64 / 128 / 256 workgroup rows; 200 keys are not a multiple of 64
SHAPES = [(320, 200), (256, 320)]
HEADS = 2
FORMS = {"serial_eager": dict(), "overlap_eager": dict(overlap=True), "graph": dict(use_graph=True),
         "graph_overlap": dict(use_graph=True, overlap=True), "on_step": dict(on_step=lambda i, t, lat: False)}
IDX = [2, 0, 2, 1]                                       # P = 4 persons on a pool of G >= 3 garments: a repeated value, not monotone
TRANSPORTS = ("kernel", "copy")
TABLE = 0x70000                                          # a stand-in device address: never read on the host
# The fp8 kernel against fp32 SDPA on the unquantised operands.  kernel_checks.TOL is the 16-bit kernels' bar (2e-3 / 1.6e-2: one 16-bit rounding
# of the output); e4m3 operands carry 3 mantissa bits (relative step 2^-3), so no fp8 launch can meet it.  This is the bar include/idmvton_hip.h
# states for idmvton_attn_f8 and tests/kernel_checks.py holds check_attn_f8 to (its `attn_f8_*` entries), written once here.
F8_SDPA_BAR = 1.2e-1


# ------------------------------------------------------------------------------------------------------------------ C ABI
def attn_args(mode, B=4, b0=2):
    from idm_vton_amd import ffi
    a = ffi.AttnArgs()
    a.dtype, a.mode, a.B, a.heads, a.Nq = ffi.BF16, mode, B, 2, 64
    a.q, a.ldq, a.out, a.ldo, a.nseg = 0x10000, 128, 0x20000, 128, 2
    for s in range(2):                                   # (the pointers are never dereferenced: every call of the tests is refused before a launch)
        a.k[s], a.vt[s], a.ldk[s], a.ldvt[s], a.nk[s], a.k_rows[s] = 0x30000 + s * 0x10000, 0x50000 + s * 0x10000, 128, 64, 64, 64
    a.seg_b0[0], a.seg_b0[1] = 0, b0
    return a


def attn_f8_args(B=4, b0=2):
    from idm_vton_amd import ffi
    a = ffi.AttnF8Args()
    a.out_dtype, a.B, a.heads, a.Nq = ffi.BF16, B, 2, 64
    a.q8, a.ldq, a.out, a.ldo, a.nseg = 0x10000, 128, 0x20000, 128, 2
    for s in range(2):
        a.k8[s], a.vt8[s], a.ldk[s], a.ldvt[s], a.nk[s], a.k_rows[s] = 0x30000 + s * 0x10000, 0x50000 + s * 0x10000, 128, 64, 64, 64
    a.seg_b0[0], a.seg_b0[1] = 0, b0
    a.qk_scale_exp, a.v_scale_exp = -4, -2
    return a


# ------------------------------------------------------------------------------------------------------------------ synthetic caches
def ask(c, **over):
    """c.check with the cache's own facts, `over` changed."""
    kw = dict(timesteps=c.timesteps, h=c.h, w=c.w, dtype=c.dtype, attn_fp8=c.attn_fp8, f8_exp=c.f8_exp, weights_id=c.weights_id, persons=c.G)
    kw.update(over)
    return c.check(**kw)


POOL_FEATS = ((12, 64), (6, 128))                        # (token rows, channels) of pool_cache's two features


def pool_cache(G=2, ts=(900, 700, 500, 300, 100), h=4, w=3, dtype=torch.float16, attn_fp8=False, f8_exp=(2, 2, 2), wid="w0", seed=0):
    """Every (timestep, garment, feature) block has values of its own (a seeded draw), so a misplaced block cannot compare equal."""
    from idm_vton_amd.garment_cache import GarmentCache
    n, kv = len(ts), []
    g = torch.Generator().manual_seed(seed)
    for N, Cc in POOL_FEATS:
        if dtype == torch.uint8:
            k = torch.randint(0, 256, (n * G * N, Cc), generator=g, dtype=torch.uint8)
            vt = torch.randint(0, 256, (n * G, Cc, N), generator=g, dtype=torch.uint8)
        else:
            k, vt = torch.randn(n * G * N, Cc, generator=g).to(dtype), torch.randn(n * G, Cc, N, generator=g).to(dtype)
        kv.append((k, vt))
    return GarmentCache(G=G, timesteps=ts, h=h, w=w, dtype=torch.float16 if dtype == torch.uint8 else dtype, attn_fp8=attn_fp8, f8_exp=f8_exp,
                        weights_id=wid, kv=kv)


def scaled_cache(G=2, n=5, h=16, w=12, dtype=torch.float16, seed=0, **kw):
    """Two features of different (N, C) with random values of a scale of their own per garment, feature and tensor (that one's values grow
    beyond fp16's range): what the packed format's per-tensor exponents are for."""
    from idm_vton_amd.garment_cache import GarmentCache
    g = torch.Generator().manual_seed(seed)
    kv = []
    for f, (N, Cc) in enumerate(((h * w, 64), (h * w // 4, 128))):
        sk = torch.tensor([10.0 ** (gi - f) for gi in range(G)]).view(1, G, 1)
        k = (torch.randn(n, G, N * Cc, generator=g) * sk).reshape(n * G * N, Cc).to(dtype)
        vt = (torch.randn(n, G, Cc * N, generator=g) * sk * 300.0).reshape(n * G, Cc, N).to(dtype)
        kv.append((k, vt))
    args = dict(G=G, timesteps=list(range(900, 900 - 200 * n, -200)), h=h, w=w, dtype=dtype, attn_fp8=False, f8_exp=(2, 2, 2), weights_id="w0", kv=kv)
    args.update(kw)
    return GarmentCache(**args)


def cache3(G=3, n=4, dtype=torch.float16, seed=0):
    """Three features of different (N, C): K [n * G * N][C], V^T [n * G][C][N]."""
    from idm_vton_amd.garment_cache import GarmentCache
    g = torch.Generator().manual_seed(seed)
    kv = [(torch.randn(n * G * N, Cc, generator=g).to(dtype), torch.randn(n * G, Cc, N, generator=g).to(dtype)) for N, Cc in ((192, 64), (48, 128), (1040, 16))]
    return GarmentCache(G=G, timesteps=list(range(900, 900 - 200 * n, -200)), h=16, w=12, dtype=dtype, attn_fp8=False, f8_exp=(2, 2, 2), weights_id="w0", kv=kv)


# the K / V^T shelf of the CPU tests: three kinds of garment in slots of the shapes of cache3's features
SHELF_SLOT = [(192, 64), (48, 128), (1040, 16)]          # (N_f, C_f) of the slot's three features; ld_f = N_f
# A smaller, B the slot's size, C smaller with V^T row lengths that are no multiple of 64 (80, 16, 528)
SHELF_KINDS = {"a": ((8, 12), [(96, 64), (32, 128), (512, 16)]), "b": ((16, 12), SHELF_SLOT), "c": ((9, 5), [(80, 64), (16, 128), (528, 16)])}
N_T = 4


def shelf_one(kind, seed=0, dtype=torch.float16, **kw):
    """A G = 1 cache of N_T timesteps at the compact size of SHELF_KINDS[kind]: K [n * N'][C], V^T [n][C][N']."""
    from idm_vton_amd.garment_cache import GarmentCache
    (gh, gw), feats = SHELF_KINDS[kind]
    g = torch.Generator().manual_seed(100 * seed + ord(kind))
    kv = [(torch.randn(N_T * N, Cc, generator=g).to(dtype), torch.randn(N_T, Cc, N, generator=g).to(dtype)) for N, Cc in feats]
    args = dict(G=1, timesteps=list(range(900, 900 - 200 * N_T, -200)), h=16, w=12, gh=gh, gw=gw, dtype=dtype, attn_fp8=False, f8_exp=(2, 2, 2),
                weights_id="w0", kv=kv)
    args.update(kw)
    return GarmentCache(**args)


def shelf_like(dtype=torch.float16):
    """What TryonEngine.empty_garment_cache gives: one uninitialised slot of the slot's shapes, with `sizes`."""
    from idm_vton_amd.garment_cache import GarmentCache
    kv = [(torch.empty(N_T * N, Cc, dtype=dtype), torch.empty(N_T, Cc, N, dtype=dtype)) for N, Cc in SHELF_SLOT]
    return GarmentCache(G=1, timesteps=list(range(900, 900 - 200 * N_T, -200)), h=16, w=12, gh=16, gw=12, dtype=dtype, attn_fp8=False, f8_exp=(2, 2, 2),
                        weights_id="w0", kv=kv, sizes=[(16, 12)])


def cpu_shelf(packed, dtype=torch.float16, **kw):
    from idm_vton_amd.garment_cache import GarmentShelf
    shelf = GarmentShelf(shelf_like(dtype), storage="e4m3" if packed else "native", **kw)
    for kind in "abc":
        shelf.add(kind, shelf_one(kind, dtype=dtype))
    return shelf


# ------------------------------------------------------------------------------------------------------------------ records
def record_fields(rec):
    """A record table's rows -> (src, dst, exp, rows, cols, lds, ldd)."""
    return [(int(r[0]), int(r[1]), int(r[2]), int(r[3]) & 0xffffffff, int(r[3]) >> 32, int(r[4]) & 0xffffffff, int(r[4]) >> 32) for r in rec]


def apply_records(rec, packed, dtype):
    """The interpreter: what idmvton_kv_fill does with a record table, on host memory, by address and by rows -- a byte copy, unpack_values
    for a widening data run (the exponent read through its address), zeros for a zero run."""
    from idm_vton_amd.garment_cache import unpack_values
    for src, dst, exp, rows, cols, lds, ldd in record_fields(rec):
        ldd_bytes = ldd * 2 if packed else ldd
        out_bytes = cols * 2 if packed else cols
        for r in range(rows):
            if src == 0:
                C.memset(dst + r * ldd_bytes, 0, out_bytes)
            elif not packed:
                C.memmove(dst + r * ldd_bytes, src + r * lds, cols)
            else:
                b = torch.frombuffer(bytearray(C.string_at(src + r * lds, cols)), dtype=torch.uint8)
                x = unpack_values(b, torch.tensor(C.c_int32.from_address(exp).value), dtype).contiguous()
                C.memmove(dst + r * ldd_bytes, x.data_ptr(), out_bytes)


# ------------------------------------------------------------------------------------------------------------------ comparisons
def caches_equal(a, b, sizes=False):
    """Two K / V^T caches: the same facts (with `sizes`: the slots' garment sizes too), dtypes and values."""
    facts = lambda c: (c.G, c.timesteps, c.h, c.w, c.gh, c.gw, c.dtype, c.attn_fp8, c.f8_exp, c.weights_id) + ((c.sizes,) if sizes else ())
    return facts(a) == facts(b) and len(a.kv) == len(b.kv) and \
        all(ka.dtype == kb.dtype and torch.equal(ka, kb) and torch.equal(va, vb) for (ka, va), (kb, vb) in zip(a.kv, b.kv))


def same_packed(a, b):
    """Two packed caches: the same type, bytes and exponents."""
    return (type(a) is type(b) and a.G == b.G and torch.equal(a.exps, b.exps) and
            all(torch.equal(x, y) and torch.equal(u, v) and x.dtype == torch.uint8 for (x, u), (y, v) in zip(a.kv, b.kv)))


def same_values(a, b):
    """Two K / V^T caches on any devices: the same values."""
    return len(a.kv) == len(b.kv) and all(torch.equal(ka.cpu(), kb.cpu()) and torch.equal(va.cpu(), vb.cpu()) for (ka, va), (kb, vb) in zip(a.kv, b.kv))


def same_features(a, b):
    """Two feature caches: asserts the same facts, dtypes, values and (packed) exponents."""
    assert (a.G, a.features, a.packed, a.timesteps, a.h, a.w, a.gh, a.gw, a.dtype, a.weights_id) == \
           (b.G, b.features, b.packed, b.timesteps, b.h, b.w, b.gh, b.gw, b.dtype, b.weights_id)
    assert len(a.kv) == len(b.kv)
    for ea, eb in zip(a.kv, b.kv):
        assert len(ea) == len(eb) == 1 and ea[0].dtype == eb[0].dtype and torch.equal(ea[0], eb[0])
    if a.packed:
        assert torch.equal(a.exps, b.exps)


# ------------------------------------------------------------------------------------------------------------------ _cached_fill on a CPU engine
# The grid of tests/test_garment_fill_cpu.py, tests/test_garment_features_cpu.py and tests/test_garment_feature_shelf_cpu.py: two features,
# n = 4 cached timesteps, k = 3, blocks of 1, 2, 1 timesteps, P = 3 persons with garment_index [2, 2, 0]
FEATS = [(32, 64), (16, 128)]                       # (N_f, C_f) of the two features; ld_f = N_f
K, P, BLOCKS, GINDEX, DTYPE = 3, 3, [(0, 1), (1, 2), (3, 1)], [2, 2, 0], torch.float16
ORDERS = {"consecutive": [0, 1, 2, 3], "by value": [3, 1, 0, 2]}
TS = list(range(900, 900 - 200 * N_T, -200))
META = dict(timesteps=TS, h=8, w=4, gh=8, gw=4, dtype=DTYPE, attn_fp8=False, f8_exp=(2, 2, 2), weights_id="w0")


class Event:
    """Stand-in for a torch.cuda.Event that has always completed."""

    def record(self, *a):
        pass

    def query(self):
        return True


def standin_unet(calls):
    """project_garment_kv as plain torch: K = F W_k^T, V^T = (F W_v^T)^T per batch element, rounded once -- one weight pair per feature, the
    rows of `out` beyond the batch untouched (unet.project_garment_kv's contract).  Weights in {-1, 0, 1} and fp64 accumulation: every sum of
    at most 128 fp16 values is then exact, so a row's result cannot depend on the batch it is computed in or on the matmul's blocking."""
    g = torch.Generator().manual_seed(99)
    W = [tuple(torch.randint(-1, 2, (Cc, Cc), generator=g).double() for _ in range(2)) for _, Cc in FEATS]

    def project_garment_kv(feats, out=None):
        calls.append([tuple(f.shape) for f in feats])
        res = []
        for i, (f, (wk, wv)) in enumerate(zip(feats, W)):
            Bg, N, Cc = f.shape
            k = (f.reshape(Bg * N, Cc).double() @ wk.t()).to(f.dtype)
            vt = (f.double() @ wv.t()).transpose(1, 2).to(f.dtype)
            if out is not None:
                out[i][0][:Bg * N].copy_(k)
                out[i][1][:Bg].copy_(vt)
                k, vt = out[i][0][:Bg * N], out[i][1][:Bg]
            res.append((k, vt))
        return res
    return types.SimpleNamespace(project_garment_kv=project_garment_kv, attn_fp8=False, f8_exp=(2, 2, 2))
