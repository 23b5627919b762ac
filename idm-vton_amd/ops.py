"""Thin torch-tensor front end over the C ABI (ffi.py).  Torch is used only for device memory and the current stream.

All activations are NHWC / token-major: a tensor of shape [..., C] with C contiguous.  Every function launches
asynchronously on `torch.cuda.current_stream()` and returns its output tensor(s).  No function has a CPU path.
"""
import ctypes as C
import json
import os

import torch

from . import ffi

_DT = {torch.float16: ffi.F16, torch.bfloat16: ffi.BF16}


def _dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"idm_vton_amd ops take float16/bfloat16 tensors, got {t.dtype}") from None


def _stream():
    return torch.cuda.current_stream().cuda_stream


# Optional per-launch instrumentation (bench.py roofline leg): when PROFILE is a list, every C-ABI launch is bracketed
# by HIP events on the launch stream and appended as (kernel family, start, end, flops, algorithmic bytes).
PROFILE = None


def _call(fn_name, args, flops=0.0, bytes_=0.0, seg_nb=None, seg_index=None, seg_nk=None):
    """seg_nb: the shared-segment attention entry points' extra argument (fn_name is then idmvton_attn_*_shared); seg_index: the indexed ones'
    second extra argument, two device addresses (fn_name is then idmvton_attn_*_indexed); seg_nk: the ragged ones' third, two device addresses
    (fn_name is then idmvton_attn_*_ragged)."""
    if seg_nk is not None:
        launch = lambda: ffi.call_ragged(fn_name, args, seg_nb, seg_index, seg_nk, _stream())
    elif seg_index is not None:
        launch = lambda: ffi.call_indexed(fn_name, args, seg_nb, seg_index, _stream())
    elif seg_nb is not None:
        launch = lambda: ffi.call_shared(fn_name, args, seg_nb, _stream())
    else:
        launch = lambda: ffi.call(fn_name, args, _stream())
    if PROFILE is None:
        launch()
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch()
    e1.record()
    PROFILE.append((fn_name, e0, e1, flops, bytes_))


# Per-shape kernel configuration table measured on an MI355X by tools/gpu_tune.py.  The tuner runs the bf16 engine and checks every entry
# against the default configuration's output on the real bf16 operands before admitting it; the fp16 keys are MIRRORS of those entries
# (load_tune below) and launches with IDMVTON_IO_OUT_F8 share the key of the plain launch, so for fp16 and e4m3 output the guarantee is not
# the tuner's but the suite's: tests/kernel_checks.py runs every (variant, BN, BM) of the table in both storage dtypes (RING_TILES) and with
# e4m3 output (gemm_f8_out_*), and tests/test_host_cpu.py checks that list against the table.  Missing file / missing key => the library's
# built-in heuristic (tile_hint / tune = 0).
# IDMVTON_TUNE_TABLE=<file>: another tuning table than the committed one (A/B of two tables on one box; measurement only)
TUNE_PATH = os.environ.get("IDMVTON_TUNE_TABLE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "tune_gfx950.json")
_TUNE = {"gemm": {}, "attn": {}}
RECORD = None          # tools/gpu_tune.py: list collecting (kind, key, args struct, keep-alive tensors) of every launch


def load_tune(path=TUNE_PATH):
    global _TUNE
    _TUNE = {"gemm": {}, "attn": {}}
    if path and os.path.exists(path):
        with open(path) as f:
            t = json.load(f)
        _TUNE = {"gemm": dict(t.get("gemm", {})), "attn": dict(t.get("attn", {}))}
        # The tuner runs the bf16 engine (keys "1,..."); fp16 launches of the same shapes ("0,...") run the same kernels with the other MFMA
        # opcode, so an entry measured for one storage type also serves the other unless that one has its own.  (Until round 5 the fp16
        # engine -- the reference's dtype, bench.py's `fp16` / `fp16_fp8` legs -- ran on the untuned heuristics.)
        for kind in ("gemm", "attn") if os.environ.get("IDMVTON_TUNE_NO_MIRROR") != "1" else ():     # (the env switch: A/B measurement only)
            for k, v in list(_TUNE[kind].items()):
                d, rest = k.split(",", 1)
                if d in ("0", "1"):
                    _TUNE[kind].setdefault(("1" if d == "0" else "0") + "," + rest, v)
    return _TUNE


def gemm_key(a):
    return "%d,%d,%d,%d,%d,%d,%d,%d,%d,%d" % (a.dtype, a.M, a.N, a.Ktot, a.nseg, a.Wo, a.stride, a.ups, a.mode, 1 if a.vt else 0)


def attn_key(a):
    return "%d,%d,%d,%d,%d,%d,%d,%d,%d" % (a.dtype, a.mode, a.B, a.heads, a.Nq, a.nseg, a.nk[0], a.nk[1] if a.nseg > 1 else 0,
                                          a.seg_b0[1] if a.nseg > 1 else 0)


def _dev(t):
    if not t.is_cuda:
        raise RuntimeError("idm_vton_amd ops run on the GPU only (tensor is on %s); there is no CPU fallback" % t.device)
    return t


def _ptr(t):
    return None if t is None else _dev(t).data_ptr()


class SegSpec:
    """One K-segment of the virtual activation matrix (see include/idmvton_hip.h, idmvton_seg)."""
    __slots__ = ("t", "coff", "len", "dy", "dx")

    def __init__(self, t, coff, length, dy=0, dx=0):
        self.t, self.coff, self.len, self.dy, self.dx = t, coff, length, dy, dx


def gemm_conv(segs, w, M, *, Ho=1, Wo=None, Hi=1, Wi=None, stride=1, ups=False, out=None, ldo=None, bias=None,
              rowbias=None, rowbias_ld=0, rows_per_group=1, res=None, ldr=None, geglu=False, gelu=False, quick_gelu=False, vt=None,
              vt_n0=0, vt_tokens=0, vt_perm=True, colscale_n=0, colscale=1.0, tile_hint=0, out_f32=False, xattn=None, f8=None):
    """out[M][N] = epilogue(X . W^T); X assembled from `segs` (list of SegSpec); w: [N][Ktot] contiguous.
    f8 = (out_scale, vt_scale): `out` ([M][n_out] uint8) and `vt` ([B][N - vt_n0][vt_tokens] uint8, fp8 slot order) are written as e4m3
    operands of attention_f8 (IDMVTON_IO_OUT_F8): value * scale, saturating, one rounding from the fp32 accumulator.
    fp32 residual stream: a float32 `res` is read as fp32; out_f32=True (or a float32 `out`) writes fp32 (io_flags).
    xattn = dict(segs=[dict(k=, vt=, nk=, ldk=, ldvt=, k_rows=)] * (1 | 2), tokens=rows per batch element, ip_scale=): the GEMM is a
    cross-attention's query projection and its epilogue is the attention (include/idmvton_hip.h, IDMVTON_EPI_XATTN); w's rows in
    accumulator order (xattn_q_weight()).
    vt: columns >= vt_n0 are written transposed ([B][N - vt_n0][vt_tokens]); vt_perm=True (default) writes them in the attention
    kernel's key order (see key_order()), False as a plain transpose."""
    if f8 is not None:
        # the C side's IDMVTON_IO_OUT_F8 contract (plain 16-byte epilogue): refuse here what would otherwise be silently dropped with the flags
        if res is not None or rowbias is not None or geglu or gelu or quick_gelu or (bias is not None and bias.dtype == torch.float32):
            raise ValueError("gemm_conv(f8=...): no residual / rowbias / activation, and the bias in the storage dtype (not fp32)")
        if vt is not None and vt_tokens % 64 != 0:
            raise ValueError(f"gemm_conv(f8=...): vt_tokens must be a multiple of 64 (got {vt_tokens})")
    a = ffi.GemmConvArgs()
    a.dtype = _dt(w)
    N, Ktot = w.shape
    a.w, a.N, a.Ktot = _ptr(w), N, Ktot
    a.nseg = len(segs)
    for i, s in enumerate(segs):
        t = _dev(s.t)
        g = a.seg[i]
        # channels per pixel = the stride of the innermost pixel dimension that has more than one entry (torch leaves the strides of
        # size-1 dimensions arbitrary: a [1][1][1][64] NHWC tensor can report stride(-2) == 1 -- found by the hypothesis sweep)
        pitch = t.shape[-1]
        for d in range(t.dim() - 2, -1, -1):
            if t.shape[d] > 1:
                pitch = t.stride(d)
                break
        extent = 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride()))     # elements reachable from data_ptr
        g.ptr, g.bytes, g.pitch = t.data_ptr(), extent * t.element_size(), pitch
        g.coff, g.len, g.dy, g.dx = s.coff, s.len, s.dy, s.dx
    Wo = M if Wo is None else Wo
    Wi = M if Wi is None else Wi
    a.M, a.Ho, a.Wo, a.Hi, a.Wi, a.stride, a.ups = M, Ho, Wo, Hi, Wi, stride, int(bool(ups))
    n_out = N // 2 if geglu else (vt_n0 if vt is not None else N)
    if out is None and n_out > 0:
        out = torch.empty((M, n_out), dtype=torch.uint8 if f8 is not None else (torch.float32 if out_f32 else w.dtype), device=w.device)
    if f8 is not None:
        if (out is not None and out.dtype != torch.uint8) or (vt is not None and vt.dtype != torch.uint8):
            raise TypeError("gemm_conv(f8=...): out / vt must be uint8 (e4m3 bytes)")
        a.f8_out_scale, a.f8_vt_scale = float(f8[0]), float(f8[1])
    a.io_flags = ffi.IO_OUT_F8 if f8 is not None else (
        (ffi.IO_RES_F32 if res is not None and res.dtype == torch.float32 else 0) |
        (ffi.IO_OUT_F32 if out is not None and out.dtype == torch.float32 else 0) |
        (ffi.IO_BIAS_F32 if bias is not None and bias.dtype == torch.float32 else 0))
    a.out = _ptr(out)
    a.ldo = (ldo if ldo is not None else (out.stride(-2) if out is not None else 0))
    a.bias = _ptr(bias)
    a.rowbias, a.rowbias_ld, a.rows_per_group = _ptr(rowbias), rowbias_ld, rows_per_group
    a.res = _ptr(res)
    a.ldr = (ldr if ldr is not None else (res.stride(-2) if res is not None else 0))
    a.mode = ffi.EPI_GEGLU if geglu else (ffi.EPI_GELU if gelu else (ffi.EPI_QUICKGELU if quick_gelu else ffi.EPI_NONE))
    xa, xflops = None, 0.0
    if xattn is not None:
        xa = ffi.XAttn()
        xa.nseg, xa.tokens, xa.ip_scale = len(xattn["segs"]), xattn["tokens"], xattn.get("ip_scale", 1.0)
        for i, sg in enumerate(xattn["segs"]):
            xa.k[i], xa.vt[i], xa.ldk[i], xa.ldvt[i], xa.nk[i], xa.k_rows[i] = _ptr(sg["k"]), _ptr(sg["vt"]), sg["ldk"], sg["ldvt"], sg["nk"], sg["k_rows"]
            xflops += 4.0 * M * N * sg["nk"]
        a.mode, a.xattn = ffi.EPI_XATTN, C.pointer(xa)
    a.vt, a.vt_n0, a.vt_tokens = _ptr(vt), vt_n0, vt_tokens
    a.vt_perm = int(bool(vt_perm)) if vt is not None else 0
    a.colscale_n, a.colscale = colscale_n, colscale
    a.tile_hint = tile_hint if tile_hint else _TUNE["gemm"].get(gemm_key(a), 0)
    if RECORD is not None:
        RECORD.append(("gemm", gemm_key(a), type(a).from_buffer_copy(a), (segs, w, out, bias, rowbias, res, vt, xa, xattn)))
    seen, xbytes = set(), 0                               # algorithmic bytes: every distinct operand tensor once
    for sg in segs:
        if sg.t.data_ptr() not in seen:
            seen.add(sg.t.data_ptr())
            xbytes += sg.t.numel() * sg.t.element_size()
    esz = w.element_size()
    obytes = (M * (N // 2 if geglu else N)) * (out.element_size() if out is not None else esz) + (M * N * res.element_size() if res is not None else 0)
    _call("idmvton_gemm_conv", a, flops=2.0 * M * N * Ktot + xflops, bytes_=float(xbytes + N * Ktot * esz + obytes))
    return out


def xattn_q_weight(w):
    """attn2.to_q weight [heads*64][K] -> rows in the ACCUMULATOR ORDER the fused cross-attention epilogue contracts in: inside every group of
    16 output channels, bits 2 and 3 of the channel index swapped (the same involution as key_order_index)."""
    return w.index_select(0, key_order_index(w.shape[0], w.device)).contiguous()


def key_order_index(n, device=None):
    """Position -> key index of the attention kernel's V^T key order: inside every group of 16 keys, bits 2 and 3 of the index
    are swapped (csrc/attention.hip: the 8 keys a half-wave contracts per PV MFMA become one aligned 16-byte read)."""
    if n % 16:
        raise ValueError("key order needs a multiple of 16 keys, got %d" % n)
    i = torch.arange(n, device=device)
    return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1)


def key_order(vt):
    """[..., keys] plain V^T -> the layout idmvton_attn_fwd consumes (the permutation is an involution)."""
    return vt.index_select(-1, key_order_index(vt.shape[-1], vt.device)).contiguous()


def round16(n):
    return (n + 15) // 16 * 16


def linear(x, w, **kw):
    """x: [M][K] (row stride x.stride(0), K contiguous)."""
    M, K = x.shape
    return gemm_conv([SegSpec(x, 0, K)], w, M, **kw)


def conv_segs(x, k, pad, coff=0, length=None):
    """K-segments of a k x k convolution over NHWC tensor x [B][H][W][C] (weights laid out [Cout][ky][kx][C])."""
    length = x.shape[-1] if length is None else length
    return [SegSpec(x, coff, length, ky - pad, kx - pad) for ky in range(k) for kx in range(k)]


QSCALE = 0.125 * 1.4426950408889634          # softmax_scale(d=64) * log2(e): what `q_prescaled` means


def attention(q, out, segs, heads, *, mode=ffi.ATTN_SELF, ip_scale=1.0, B=None, Nq=None, ldq=None, ldo=None, tune=0, q_prescaled=False):
    """q/out: [B][Nq][>=heads*64] views; segs: list of dict(k=, vt=, nk=, ldk=, ldvt=, k_rows=, b0=[, nb=][, index=][, nk_table=]).
    nb (absent or 0: one K / V^T element per query batch from b0 on): the segment holds nb elements and batch b reads (b - b0) % nb -- a shared
    garment segment, launched through idmvton_attn_fwd_shared.  index (with nb >= 1): an int32 device tensor of B - b0 entries, batch b reads
    element index[b - b0] of the nb -- a pooled garment segment, launched through idmvton_attn_fwd_indexed.  nk_table: an int32 device tensor of
    B entries (from batch 0 on), batch b has nk_table[b] of the segment's nk keys -- a ragged segment (slots of nk keys, each garment at the
    front of its own), launched through idmvton_attn_fwd_ragged; nk stays the capacity.  The tune-table key carries neither nb nor a table: same
    kernel choice as the materialised launch (the FLOP count of a profile uses the capacity too)."""
    a = ffi.AttnArgs()
    a.dtype, a.mode = _dt(q), mode
    a.B = q.shape[0] if B is None else B
    a.Nq = q.shape[1] if Nq is None else Nq
    a.heads = heads
    a.q, a.ldq = _ptr(q), (q.stride(-2) if ldq is None else ldq)
    a.out, a.ldo = _ptr(out), (out.stride(-2) if ldo is None else ldo)
    a.nseg = len(segs)
    for i, s in enumerate(segs):
        a.k[i], a.vt[i] = _ptr(s["k"]), _ptr(s["vt"])
        a.ldk[i], a.ldvt[i] = s["ldk"], s["ldvt"]
        a.nk[i], a.k_rows[i], a.seg_b0[i] = s["nk"], s.get("k_rows", 0), s.get("b0", 0)
    a.ip_scale = ip_scale
    a.q_prescaled = int(bool(q_prescaled))
    a.tune = tune
    if not tune:
        t = _TUNE["attn"].get(attn_key(a), 0)
        # the table is measured on the engine's launches, which pre-multiply q; kernels that REQUIRE that (7 / 8: attn_pf, 16: attn_sp) are not
        # applied to a launch with a raw q (the key does not carry the flag): the library's own rule picks a kernel for it
        a.tune = t if (q_prescaled or ((t >> 16) & 0xff) not in (7, 8, 16)) else 0
    if RECORD is not None:
        RECORD.append(("attn", attn_key(a), type(a).from_buffer_copy(a), (q, out, segs)))
    fl = 0.0
    for s in segs:
        fl += 4.0 * (a.B - s.get("b0", 0)) * heads * a.Nq * s["nk"] * 64
    nb, ix, nkt = _seg_nb(segs), _seg_index(segs, a.B), _seg_nk(segs, a.B)
    _call("idmvton_attn_fwd_ragged" if nkt else "idmvton_attn_fwd_indexed" if ix else "idmvton_attn_fwd_shared" if nb else "idmvton_attn_fwd", a, flops=fl,
          bytes_=2.0 * a.B * a.Nq * heads * 64 * q.element_size(), seg_nb=nb or ([0, 0] if ix or nkt else None), seg_index=ix, seg_nk=nkt)
    return out


def _seg_nb(segs):
    """None when no segment is shared (the old entry point is called), else the two seg_nb values."""
    nb = [int(s.get("nb", 0) or 0) for s in segs] + [0] * (2 - len(segs))
    return nb if any(nb) else None


def _seg_index(segs, B):
    """None when no segment carries an index table (the other entry points are called), else the two device addresses (0 = no table)."""
    ix = []
    for s in segs:
        t = s.get("index")
        if t is not None:
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == B - s.get("b0", 0)):
                raise ValueError(f"attention: a segment's index must be a contiguous int32 device tensor of B - b0 = {B - s.get('b0', 0)} entries")
            if int(s.get("nb", 0) or 0) < 1:
                raise ValueError("attention: a segment with index= needs nb= (the number of elements it holds)")
        ix.append(0 if t is None else t.data_ptr())
    ix += [0] * (2 - len(ix))
    return ix if any(ix) else None


def _seg_nk(segs, B):
    """None when no segment carries a key-count table (the other entry points are called), else the two device addresses (0 = no table)."""
    nk = []
    for s in segs:
        t = s.get("nk_table")
        if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and t.numel() == B):
            raise ValueError(f"attention: a segment's nk_table must be a contiguous int32 device tensor of B = {B} entries")
        nk.append(0 if t is None else t.data_ptr())
    nk += [0] * (2 - len(nk))
    return nk if any(nk) else None


def quant_f8(src, scale, mode=0, out=None):
    """16-bit -> e4m3 bytes (torch.uint8) times `scale` (a power of two).  mode 0: src [rows][cols] (row stride src.stride(0)) ->
    [rows][cols]; mode 1: src = V^T [rows][N] in the 16-bit kernels' key order -> [rows][roundup64(N)] in the fp8 kernel's slot order."""
    rows, cols = src.shape
    ldd = cols if mode == 0 else (cols + 63) // 64 * 64
    if out is None:
        out = torch.empty((rows, ldd), dtype=torch.uint8, device=src.device)
    a = ffi.QuantF8Args()
    a.dtype, a.mode, a.rows, a.cols = _dt(src), mode, rows, cols
    a.src, a.lds, a.dst, a.ldd, a.scale = _ptr(src), src.stride(0), _ptr(out), out.stride(0), scale
    _call("idmvton_quant_f8", a, bytes_=float(rows * cols * (src.element_size() + 1)))
    return out


KV_UNPACK_CHUNK = 1024                                   # 16-byte items one workgroup of idmvton_kv_unpack widens (csrc/kv_unpack.hip)
KV_UNPACK_MAX_N = 65534                                  # descriptors per launch (grid.y; even: a slice of a table stays 16-byte aligned)


def kv_items(rec):
    """Descriptor records int64 [n][5] -> int64 [n], the 16-byte items of each run: rows x cols / 16."""
    return (rec[:, 3] & 0xffffffff) * ((rec[:, 3] >> 32) >> 4)


class KvUnpackTable:
    """The descriptor table of idmvton_kv_unpack: `host` -- int64 CPU tensor [n][5] whose rows ARE idmvton_kv_unpack_desc records (src, dst,
    exp, rows | cols << 32, lds | ldd << 32: little-endian, 40 bytes) --, `dev` its device copy (one upload), and `items` the 16-byte items
    of each run.  launch(dtype, first, count) widens descriptors [first, first + count) in one launch; `first` must be even (40-byte
    records: the slice of the device copy has to start 16-byte aligned)."""

    def __init__(self, host, device):
        self.host = host.contiguous()
        self.n = self.host.shape[0]
        self.items = kv_items(self.host)
        self.dev = self.host.to(device)

    def launch(self, dtype, first=0, count=None):
        count = self.n - first if count is None else count
        if first % 2 or first < 0 or count < 1 or first + count > self.n:
            raise ValueError(f"kv_unpack: descriptors [{first}, {first + count}) of {self.n} (an even first index, at least one descriptor)")
        for f0 in range(first, first + count, KV_UNPACK_MAX_N):
            c = min(KV_UNPACK_MAX_N, first + count - f0)
            a = ffi.KvUnpackArgs()
            a.dtype, a.n, a.desc = _DT[dtype], c, self.dev.data_ptr() + 40 * f0
            a.max_chunks = (int(self.items[f0:f0 + c].max()) + KV_UNPACK_CHUNK - 1) // KV_UNPACK_CHUNK
            launch = lambda: ffi.call_kv_unpack(a, self.host.data_ptr() + 40 * f0, _stream())
            if PROFILE is None:
                launch()
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            launch()
            e1.record()
            PROFILE.append(("idmvton_kv_unpack", e0, e1, 0.0, 48.0 * float(self.items[f0:f0 + c].sum())))


def kv_unpack(descs, dtype, device=None):
    """e4m3 bytes -> 16-bit, exactly: dst = dtype(e4m3(src) * 2^-e) for every run of `descs`, in one launch (idmvton_kv_unpack).  descs: a
    KvUnpackTable (launched whole), or a list of (src, dst, exp) -- src a uint8 2-D tensor view (row stride src.stride(0) bytes), dst a 2-D
    view of `dtype` and the same shape, exp a one-element int32 device tensor view -- from which the table is built, checked and uploaded.
    -> the table."""
    if not isinstance(descs, KvUnpackTable):
        rec = []
        for src, dst, exp in descs:
            if src.dtype != torch.uint8 or dst.dtype != dtype or exp.dtype != torch.int32 or exp.numel() != 1 or src.dim() != 2 or src.shape != dst.shape or \
                    src.stride(1) != 1 or dst.stride(1) != 1:
                raise ValueError("kv_unpack: a run is (uint8 [rows][cols], %s [rows][cols], one int32), rows contiguous" % dtype)
            rows, cols = src.shape
            rec.append((_ptr(src), _ptr(dst), _ptr(exp), rows | (cols << 32), src.stride(0) | (dst.stride(0) << 32)))
        device = descs[0][0].device if device is None else device
        descs = KvUnpackTable(torch.tensor(rec, dtype=torch.int64).reshape(-1, 5), device)
    descs.launch(dtype)
    return descs


KV_STREAM_CHUNK = 1024                                   # 16-byte items of one chunk of idmvton_kv_stream (csrc/kv_stream.hip)
KV_STREAM_MAX_N = 1 << 20                                # descriptors per launch (IDMVTON_KVS_MAX_N)
# persistent workgroups of a fill from page-locked host memory: the smallest count within 3 % of the best measured host-link rate
# (tools/gpu_garment_stream.py --step fill; profiles/LOG.md: 56.5 GB/s from 16 workgroups on, 47.1 with 8, 26.2 with 4 -- and the count at
# which a call loses least, TryonNet running slower for as long as a fill is in flight)
KV_STREAM_WORKGROUPS = 16


def stream_address(t):
    """The address under which a kernel reads tensor t: data_ptr() of a device tensor, the device-visible address of a page-locked host tensor
    (idmvton_host_device_ptr: once per tensor, when a table is built).  ValueError for a pageable host tensor -- the GPU would fault on its
    address, so it never reaches a descriptor."""
    if t.is_cuda:
        return t.data_ptr()
    if not t.is_pinned():
        raise ValueError("kv_stream: a host tensor that a kernel reads must be page-locked (pin_memory=True); this one is pageable")
    return ffi.host_device_ptr(t.data_ptr())


def kv_stream_first(items):
    """int64 [n] 16-byte items per run -> int32 [n + 1], the exclusive prefix sum of chunks per run (idmvton_kv_stream's `first`)."""
    chunks = (items + KV_STREAM_CHUNK - 1) // KV_STREAM_CHUNK
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(chunks, 0)]).to(torch.int32)


class KvStreamTable:
    """The descriptor table of idmvton_kv_stream: `host` -- int64 CPU tensor [n][5] whose rows ARE idmvton_kv_stream_desc records, the layout
    of KvUnpackTable's (in copy mode cols, lds and ldd are bytes and exp is 0) -- and the `slices` [(first, count)] of it that will be
    launched (default: the whole table; `first` even, as a slice of the device copy has to start 16-byte aligned).  Every slice gets its own
    prefix table; records and prefix tables are uploaded ONCE, here.  launch(dtype, which, workgroups) moves slice `which` in one launch."""
    ENTRY = "kv_stream"                                      # launched through ffi.call_<ENTRY> (KvFillTable: kv_fill)

    def __init__(self, host, device, mode=ffi.KVS_WIDEN_E4M3, slices=None):
        self.host, self.mode = host.contiguous(), mode
        self.n = self.host.shape[0]
        self.slices = [(0, self.n)] if slices is None else [(int(f), int(c)) for f, c in slices]
        for f, c in self.slices:
            if f % 2 or f < 0 or c < 1 or c > KV_STREAM_MAX_N or f + c > self.n:
                raise ValueError(f"kv_stream: descriptors [{f}, {f + c}) of {self.n} (an even first index, 1 to {KV_STREAM_MAX_N} descriptors)")
        self.items = kv_items(self.host)
        firsts = [kv_stream_first(self.items[f:f + c]) for f, c in self.slices]
        self.first_at, at = [], 0
        for t in firsts:
            self.first_at.append(at)
            at += t.numel()
        self.first_host = torch.cat(firsts).contiguous()
        self.dev, self.first_dev = self.host.to(device), self.first_host.to(device)

    def launch(self, dtype, which=0, workgroups=None):
        f0, c = self.slices[which]
        a = ffi.KvStreamArgs()
        a.dtype, a.mode, a.n, a.workgroups = _DT[dtype], self.mode, c, KV_STREAM_WORKGROUPS if workgroups is None else workgroups
        a.desc, a.first = self.dev.data_ptr() + 40 * f0, self.first_dev.data_ptr() + 4 * self.first_at[which]
        call = getattr(ffi, "call_" + self.ENTRY)
        launch = lambda: call(a, self.host.data_ptr() + 40 * f0, self.first_host.data_ptr() + 4 * self.first_at[which], _stream())
        if PROFILE is None:
            return launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        PROFILE.append(("idmvton_" + self.ENTRY, e0, e1, 0.0, self.bytes_moved(f0, c)))

    def bytes_moved(self, f0, c):
        """Bytes loaded + stored by descriptors [f0, f0 + c): 16 in and 32 (widening) / 16 (copying) out per item."""
        return (48.0 if self.mode == ffi.KVS_WIDEN_E4M3 else 32.0) * float(self.items[f0:f0 + c].sum())


class KvFillTable(KvStreamTable):
    """KvStreamTable launched through idmvton_kv_fill: a record whose src is 0 is a ZERO RUN (rows x cols of +0 / zero bytes written, nothing
    loaded; exp and lds ignored).  Items and prefix tables are KvStreamTable's: a zero run counts like a data run."""
    ENTRY = "kv_fill"

    def link_bytes(self, f0=0, c=None):
        """Bytes descriptors [f0, f0 + c) LOAD: 16 per item of a data run, none for a zero run."""
        c = self.n - f0 if c is None else c
        return 16.0 * float(self.items[f0:f0 + c][self.host[f0:f0 + c, 0] != 0].sum())

    def bytes_moved(self, f0, c):                            # a zero run stores bytes and loads none
        return self.link_bytes(f0, c) + (32.0 if self.mode == ffi.KVS_WIDEN_E4M3 else 16.0) * float(self.items[f0:f0 + c].sum())


class KvPlaceTable(KvFillTable):
    """KvFillTable launched through idmvton_kv_place: the same records, zero runs, items and prefix tables, for sources that are already in
    HBM (a staging arena).  The grid is the slice's chunk count -- one workgroup per chunk --, so `workgroups` is always 0."""
    ENTRY = "kv_place"

    def launch(self, dtype, which=0, workgroups=None):
        return super().launch(dtype, which, 0)


def kv_pad_even(rec):
    """Descriptor records int64 [n][5] -> the same with the record of fewest items repeated at the end when n is odd: slices of a table start
    at even record indices (16-byte aligned device addresses), and writing identical bytes twice is what clamped lanes already do."""
    if rec.shape[0] % 2 == 0:
        return rec
    m = int(kv_items(rec).argmin())
    return torch.cat([rec, rec[m:m + 1]])


def _kv_table(cls, descs, dtype, mode, device):
    """A table of class `cls`, or a list of (src, dst, exp) 2-D tensor views from which one is built -> the table.  Where cls launches through
    an entry point with zero runs (every one but KvStreamTable's), a run whose src is None is one."""
    if isinstance(descs, KvStreamTable):
        return descs
    widen, zero_ok = mode == ffi.KVS_WIDEN_E4M3, cls is not KvStreamTable
    rec = []
    for src, dst, exp in descs:
        ok = dst.dim() == 2 and dst.stride(1) == 1 and dst.is_cuda and (not widen or dst.dtype == dtype) and (zero_ok or src is not None)
        if ok and src is not None:
            ok = src.dim() == 2 and src.shape == dst.shape and src.stride(1) == 1
            if widen:
                ok = ok and src.dtype == torch.uint8 and exp is not None and exp.dtype == torch.int32 and exp.numel() == 1
            else:
                ok = ok and src.dtype == dst.dtype
        if not ok:
            raise ValueError("%s: a run is (uint8 [rows][cols], %s [rows][cols], one int32) when widening, (x [rows][cols], x [rows][cols], None) "
                             "when copying%s; rows contiguous, the destination on the device"
                             % (cls.ENTRY, dtype, ", (None, dst [rows][cols], None) for a zero run" if zero_ok else ""))
        rows, cols = dst.shape
        sz = 1 if widen else dst.element_size()          # copy mode: byte units
        if src is None:
            rec.append((0, _ptr(dst), 0, rows | ((cols * sz) << 32), (cols * sz) | ((dst.stride(0) * sz) << 32)))
        else:
            rec.append((stream_address(src), _ptr(dst), stream_address(exp) if widen else 0, rows | ((cols * sz) << 32),
                        (src.stride(0) * sz) | ((dst.stride(0) * sz) << 32)))
    device = descs[0][1].device if device is None else device
    return cls(torch.tensor(rec, dtype=torch.int64).reshape(-1, 5), device, mode)


def kv_stream(descs, dtype, mode=ffi.KVS_WIDEN_E4M3, workgroups=None, device=None):
    """idmvton_kv_stream on every run of `descs`, in one launch of `workgroups` persistent workgroups.  descs: a KvStreamTable (its slice 0), or a
    list of (src, dst, exp) 2-D tensor views of equal shape, rows contiguous -- mode KVS_WIDEN_E4M3: src uint8 e4m3 bytes, dst of `dtype`, exp a
    one-element int32 view, dst = dtype(e4m3(src) * 2^-exp) exactly; mode KVS_COPY: src and dst of one dtype, exp None, a copy.  src and exp
    may each be a device tensor or a PAGE-LOCKED host tensor (stream_address: a pageable one is a ValueError), dst is a device tensor.
    -> the table."""
    descs = _kv_table(KvStreamTable, descs, dtype, mode, device)
    descs.launch(dtype, 0, workgroups)
    return descs


def kv_fill(descs, dtype, mode=ffi.KVS_WIDEN_E4M3, workgroups=None, device=None):
    """idmvton_kv_fill on every run of `descs`, in one launch: ops.kv_stream's arguments, and a run whose src is None is a ZERO RUN -- (None,
    dst, None) writes +0 (widening) / zero bytes (copying) over dst's [rows][cols] and loads nothing.  descs: a KvFillTable (its slice 0) or
    a list of (src | None, dst, exp | None) views.  -> the table."""
    descs = _kv_table(KvFillTable, descs, dtype, mode, device)
    descs.launch(dtype, 0, workgroups)
    return descs


def kv_place(descs, dtype, mode=ffi.KVS_WIDEN_E4M3, device=None):
    """idmvton_kv_place on every run of `descs`, in one launch of one workgroup per chunk: ops.kv_fill's arguments without `workgroups`, zero
    runs included.  descs: a KvPlaceTable (its slice 0) or a list of (src | None, dst, exp | None) views; src and exp may each be a device
    tensor -- what the entry point is built for -- or a page-locked host tensor.  -> the table."""
    descs = _kv_table(KvPlaceTable, descs, dtype, mode, device)
    descs.launch(dtype, 0)
    return descs


def attention_f8(q8, out, segs, heads, *, qk_scale_exp, v_scale_exp, B, Nq, ldq=None, ldo=None):
    """fp8 self-attention (csrc/attention_f8.hip).  q8: uint8 [B*Nq][>= heads*64]; segs: list of dict(k8=, vt8=, nk=, ldk=, ldvt=, k_rows=, b0=[, nb=][, index=][, nk_table=]);
    nb / index / nk_table as in attention() (idmvton_attn_f8_shared / idmvton_attn_f8_indexed / idmvton_attn_f8_ragged)."""
    a = ffi.AttnF8Args()
    a.out_dtype, a.B, a.heads, a.Nq = _dt(out), B, heads, Nq
    a.q8, a.ldq = _ptr(q8), (q8.stride(-2) if ldq is None else ldq)
    a.out, a.ldo = _ptr(out), (out.stride(-2) if ldo is None else ldo)
    a.nseg = len(segs)
    fl = 0.0
    for i, s in enumerate(segs):
        a.k8[i], a.vt8[i] = _ptr(s["k8"]), _ptr(s["vt8"])
        a.ldk[i], a.ldvt[i] = s["ldk"], s["ldvt"]
        a.nk[i], a.k_rows[i], a.seg_b0[i] = s["nk"], s.get("k_rows", 0), s.get("b0", 0)
        fl += 4.0 * (B - s.get("b0", 0)) * heads * Nq * s["nk"] * 64
    a.qk_scale_exp, a.v_scale_exp = qk_scale_exp, v_scale_exp
    nb, ix, nkt = _seg_nb(segs), _seg_index(segs, B), _seg_nk(segs, B)
    _call("idmvton_attn_f8_ragged" if nkt else "idmvton_attn_f8_indexed" if ix else "idmvton_attn_f8_shared" if nb else "idmvton_attn_f8", a, flops=fl,
          bytes_=float(B * Nq * heads * 64 * (1 + out.element_size())), seg_nb=nb or ([0, 0] if ix or nkt else None), seg_index=ix, seg_nk=nkt)
    return out


def attention_small(q, k, v, out, heads, d, *, scale, causal=False, B=None, Lq=None, Lk=None, ldq=None, ldk=None, ldv=None, ldo=None):
    """softmax(scale * q k^T [causal]) v, any even head_dim <= 128 (the CLIP towers).  q/out: [B][Lq][>= heads*d], k/v: [B][Lk][...]."""
    a = ffi.AttnSmallArgs()
    a.dtype = _dt(q)
    a.B = q.shape[0] if B is None else B
    a.heads, a.d = heads, d
    a.Lq = q.shape[1] if Lq is None else Lq
    a.Lk = k.shape[1] if Lk is None else Lk
    a.q, a.ldq = _ptr(q), (q.stride(-2) if ldq is None else ldq)
    a.k, a.ldk = _ptr(k), (k.stride(-2) if ldk is None else ldk)
    a.v, a.ldv = _ptr(v), (v.stride(-2) if ldv is None else ldv)
    a.out, a.ldo = _ptr(out), (out.stride(-2) if ldo is None else ldo)
    a.scale, a.causal = scale, int(bool(causal))
    _call("idmvton_attn_small", a, flops=4.0 * a.B * heads * a.Lq * a.Lk * d)
    return out


def layernorm(x, gamma, beta, eps=1e-5, out=None, out2=None):
    """x: [rows][C] (row stride x.stride(0)); float32 x = the fp32 residual stream (output in gamma's dtype)."""
    rows, Cc = x.shape
    if out is None:
        out = torch.empty((rows, Cc), dtype=gamma.dtype, device=x.device)
    a = ffi.LayerNormArgs()
    a.dtype, a.rows, a.C = _dt(gamma), rows, Cc
    a.x_f32 = int(x.dtype == torch.float32)
    a.x, a.ldx = _ptr(x), x.stride(0)
    a.gamma, a.beta, a.eps = _ptr(gamma), _ptr(beta), eps
    a.y, a.ldy = _ptr(out), out.stride(0)
    a.y2, a.ldy2 = _ptr(out2), (out2.stride(0) if out2 is not None else 0)
    _call("idmvton_layernorm", a, bytes_=(x.element_size() + (1.0 + (out2 is not None)) * out.element_size()) * rows * Cc)
    return out


def groupnorm(x, gamma, beta, groups, eps, silu, stats, x2=None, out=None, split_dtype=None):
    """x: [B][HW][C1] (+ optional x2 [B][HW][C2], virtually concatenated along C); stats: float64 scratch of at least
    gn_stats_doubles(B, HW, C, groups) elements (GN_STATS_DOUBLES covers every shape with B <= 64, groups <= 32).
    split_dtype (the split-precision VAE path): x, gamma, beta are float32 and the result is the pair [B][HW][2C] = [hi | lo] of that dtype."""
    B, HW, C1 = x.shape
    Cc = C1 + (x2.shape[-1] if x2 is not None else 0)
    prec = split_dtype is not None
    if prec and not (x.dtype == gamma.dtype == beta.dtype == torch.float32 and (x2 is None or x2.dtype == torch.float32)):
        raise TypeError("groupnorm(split_dtype=...): x, gamma and beta must be float32")
    if out is None:
        out = torch.empty((B, HW, 2 * Cc if prec else Cc), dtype=split_dtype if prec else x.dtype, device=x.device)
    a = ffi.GroupNormArgs()
    a.dtype, a.B, a.HW, a.C, a.groups = _dt(out), B, HW, Cc, groups
    a.flags = (ffi.GN_X_F32 | ffi.GN_Y_SPLIT | ffi.GN_AFFINE_F32) if prec else 0
    a.x, a.C1, a.x2 = _ptr(x), C1, _ptr(x2)
    a.gamma, a.beta, a.eps, a.silu = _ptr(gamma), _ptr(beta), eps, int(bool(silu))
    a.y, a.stats, a.stats_doubles = _ptr(out), _ptr(stats), stats.numel()
    _call("idmvton_groupnorm", a, bytes_=(2.0 * x.element_size() + (2 if prec else 1) * out.element_size()) * B * HW * Cc)
    return out


GN_STATS_DOUBLES = 2 * 32 * (2048 + 2 * 64 + 64)


def gn_stats_doubles(B, HW, C, groups):
    return ffi.lib().idmvton_groupnorm_stats_doubles(B, HW, C, groups)


def pack_input(latents, cond, out):
    a = ffi.PackInputArgs()
    B, hw = latents.shape[0], latents.shape[2] * latents.shape[3] if latents.dim() == 4 else latents.shape[2]
    a.dtype, a.B, a.hw, a.cpad = _dt(out), B, hw, out.shape[-1]
    a.latents, a.cond, a.out = _ptr(latents), _ptr(cond), _ptr(out)
    _call("idmvton_pack_input", a)
    return out


def cfg_step(eps_nhwc, latents, noise, coef):
    a = ffi.CfgStepArgs()
    B = latents.shape[0]
    hw = latents.numel() // (B * 4)
    a.dtype, a.B, a.hw, a.ldc = _dt(eps_nhwc), B, hw, eps_nhwc.shape[-1]
    a.eps_nhwc, a.latents, a.noise, a.coef = _ptr(eps_nhwc), _ptr(latents), _ptr(noise), _ptr(coef)
    _call("idmvton_cfg_step", a)
    return latents


def pack_input_cond(latents, cond, out):
    """pack_input for the conditional branch alone: out NHWC [B][hw][cpad] from cond [B][hw][9] (idmvton_pack_input_cond)."""
    a = ffi.PackInputArgs()
    B, hw = latents.shape[0], latents.shape[2] * latents.shape[3] if latents.dim() == 4 else latents.shape[2]
    if out.shape[0] != B or cond.shape[0] != B:
        raise ValueError(f"pack_input_cond: {B} persons, cond of {cond.shape[0]} rows, out of {out.shape[0]} rows (B rows each)")
    a.dtype, a.B, a.hw, a.cpad = _dt(out), B, hw, out.shape[-1]
    a.latents, a.cond, a.out = _ptr(latents), _ptr(cond), _ptr(out)
    _call("idmvton_pack_input_cond", a)
    return out


def guided_step_work_floats(B, hw):
    """Floats of the `work` buffer of guided_step for B persons of hw pixels (idmvton_guided_step_work_floats)."""
    n = ffi.lib().idmvton_guided_step_work_floats(int(B), int(hw))
    if n < 0:
        raise ValueError(f"guided_step_work_floats: B={B} hw={hw}")
    return n


def _step_operands(name, a, eps_nhwc, latents, noise, coef_row, work, width, branches=None):
    """What guided_step, person_step and row_step share: B and hw from the latents, the check of the coefficient row {c_x, c_eps, sigma,
    `width` columns of B} and of `work`, and the fields the three argument structs have in common.  branches: of an entry whose eps rows
    are [branches * B]; None: the rows are looked up, and `work` is always needed.  -> B"""
    B = latents.shape[0]
    hw = latents.numel() // (B * 4)
    if coef_row.numel() != 3 + width * B or coef_row.dtype != torch.float32:
        raise ValueError(f"{name}: coef_row holds {coef_row.numel()} {coef_row.dtype} values, needs 3 + {width}B = {3 + width * B} float32")
    if branches is not None:
        if eps_nhwc.shape[0] != branches * B:
            raise ValueError(f"{name}: eps of {eps_nhwc.shape[0]} rows for branches={branches} and {B} persons")
        a.branches = branches
    if (work is None and branches is None) or (work is not None and work.dtype != torch.float32):
        raise ValueError(f"{name}: work must be {'float32' if branches else 'a float32 tensor'}, got {None if work is None else work.dtype}")
    a.dtype, a.B, a.hw, a.ldc = _dt(eps_nhwc), B, hw, eps_nhwc.shape[-1]
    a.work, a.work_floats = _ptr(work), 0 if work is None else work.numel()
    a.eps_nhwc, a.latents, a.noise, a.coef = _ptr(eps_nhwc), _ptr(latents), _ptr(noise), _ptr(coef_row)
    return B


def guided_step(eps_nhwc, latents, noise, coef_row, work, branches=2):
    """The CFG combine + scheduler update with a guidance scale and a guidance_rescale per person (idmvton_guided_step).  eps_nhwc: NHWC
    [branches * B][hw][ldc]; coef_row: float32 device tensor {c_x, c_eps, sigma, g[0..B), phi[0..B)}; work: float32 device tensor of at
    least guided_step_work_floats(B, hw) elements (branches=1 takes None: the conditional rows alone, e = t).  Updates latents in place."""
    a = ffi.GuidedStepArgs()
    _step_operands("guided_step", a, eps_nhwc, latents, noise, coef_row, work, 2, branches)
    _call("idmvton_guided_step", a)
    return latents


def person_step(eps_nhwc, latents, noise, coef_row, work, branches=2):
    """guided_step with a strength per person (idmvton_person_step): coef_row is the float32 device tensor {c_x, c_eps, sigma, g[0..B),
    phi[0..B), active[0..B)}; person b takes the step when active[b] > 0, and is skipped otherwise -- its eps, latents, noise and part of
    `work` are neither read nor written.  The other operands are guided_step's.  Updates the active persons' latents in place."""
    a = ffi.PersonStepArgs()
    _step_operands("person_step", a, eps_nhwc, latents, noise, coef_row, work, 3, branches)
    _call("idmvton_person_step", a)
    return latents


def _int32_table(t, n, what):
    if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous():
        raise ValueError(f"{what} holds {t.numel()} {t.dtype} values, needs {n} contiguous int32")


def pack_rows(latents, cond, out, row_person):
    """The TryonNet input of a row plan (idmvton_pack_rows): out NHWC [R][hw][cpad], row r = cat(latents[p] | cond[p]) for p =
    row_person[r] -- an int32 DEVICE table of R entries, read by the kernel (clamped to [0, B - 1]); cond [B][hw][9], one row per person."""
    a = ffi.PackRowsArgs()
    B, hw = latents.shape[0], latents.shape[2] * latents.shape[3] if latents.dim() == 4 else latents.shape[2]
    R = out.shape[0]
    if cond.shape[0] != B:
        raise ValueError(f"pack_rows: {B} persons, cond of {cond.shape[0]} rows (one per person)")
    _int32_table(row_person, R, f"pack_rows: row_person for out of {R} rows")
    a.dtype, a.B, a.R, a.hw, a.cpad = _dt(out), B, R, hw, out.shape[-1]
    a.latents, a.cond, a.out, a.row_person = _ptr(latents), _ptr(cond), _ptr(out), _ptr(row_person)
    _call("idmvton_pack_rows", a)
    return out


def row_step(eps_nhwc, latents, noise, coef_row, work, rows):
    """person_step with a person's eps rows looked up (idmvton_row_step): eps_nhwc NHWC [R][hw][ldc]; rows: the int32 DEVICE table
    {urow[0..B), crow[0..B)} -- person b's unconditional / conditional row of eps, or -1: no conditional row = the person is skipped (eps,
    latents, noise and its part of `work` neither read nor written), no unconditional row = e = t.  coef_row is guided_step's
    {c_x, c_eps, sigma, g[0..B), phi[0..B)}; work: guided_step_work_floats(B, hw) float32, never None.  Updates latents in place."""
    a = ffi.RowStepArgs()
    B = _step_operands("row_step", a, eps_nhwc, latents, noise, coef_row, work, 2)
    _int32_table(rows, 2 * B, f"row_step: rows for {B} persons")
    a.R, a.rows = eps_nhwc.shape[0], _ptr(rows)
    _call("idmvton_row_step", a)
    return latents


def to_nhwc(src_nchw_f32, dtype, cpad=None, scale=1.0, shift=0.0, out=None, split=False):
    """fp32 NCHW -> NHWC [cpad] of `dtype`; split=True: NHWC [2*cpad] = [hi | lo] (the split-precision VAE path)."""
    B, Cc = src_nchw_f32.shape[:2]
    HW = src_nchw_f32.numel() // (B * Cc)
    cpad = Cc if cpad is None else cpad
    if out is None:
        out = torch.empty((B, HW, 2 * cpad if split else cpad), dtype=dtype, device=src_nchw_f32.device)
    a = ffi.LayoutArgs()
    a.flags = ffi.LAYOUT_SPLIT if split else 0
    a.dtype, a.B, a.C, a.HW, a.cpad, a.to_nhwc = _dt(out), B, Cc, HW, cpad, 1
    a.src, a.dst, a.scale, a.shift = _ptr(src_nchw_f32), _ptr(out), scale, shift
    _call("idmvton_layout", a)
    return out


def to_nchw(src_nhwc, Cc, shape_hw, scale=1.0, shift=0.0, out=None):
    B, HW, cpad = src_nhwc.shape
    if out is None:
        out = torch.empty((B, Cc) + tuple(shape_hw), dtype=torch.float32, device=src_nhwc.device)
    a = ffi.LayoutArgs()
    f32 = src_nhwc.dtype == torch.float32                  # the split-precision VAE path hands over an fp32 NHWC image
    a.flags = ffi.LAYOUT_NHWC_F32 if f32 else 0
    a.dtype, a.B, a.C, a.HW, a.cpad, a.to_nhwc = (ffi.BF16 if f32 else _dt(src_nhwc)), B, Cc, HW, cpad, 0
    a.src, a.dst, a.scale, a.shift = _ptr(src_nhwc), _ptr(out), scale, shift
    _call("idmvton_layout", a)
    return out


def vae_sample(moments_nhwc, noise, scale, out=None):
    B, hw, ldm = moments_nhwc.shape
    if out is None:
        out = torch.empty_like(noise)
    a = ffi.VaeSampleArgs()
    a.dtype, a.B, a.hw, a.ldm = _dt(moments_nhwc), B, hw, ldm
    a.moments, a.noise, a.z, a.scale = _ptr(moments_nhwc), _ptr(noise), _ptr(out), scale
    _call("idmvton_vae_sample", a)
    return out


def softmax_rows(x, scale, n_valid=0):
    """In-place softmax(scale * x) over the last dim of a 2-D tensor; n_valid: over its first n_valid columns, the rest set to 0."""
    a = ffi.SoftmaxArgs()
    a.dtype, a.rows, a.n, a.ld = _dt(x), x.shape[0], x.shape[1], x.stride(0)
    a.x, a.scale, a.n_valid = _ptr(x), scale, n_valid
    _call("idmvton_softmax_rows", a)
    return x


def softmax_rows_split(x, scale, dtype, n_valid=0, out=None):
    """softmax(scale * x) over the last dim of an fp32 2-D tensor -> the pair [rows][2n] = [hi | lo] of `dtype` (x is left as it is);
    n_valid: over the first n_valid columns, the rest 0.  out: a [rows][2n] tensor of `dtype` (row stride out.stride(0)) to write instead of a new one."""
    rows, n = x.shape
    if out is None:
        out = torch.empty((rows, 2 * n), dtype=dtype, device=x.device)
    elif tuple(out.shape) != (rows, 2 * n) or out.dtype != dtype:
        raise ValueError(f"softmax_rows_split(out=...): needs shape {(rows, 2 * n)} of {dtype}, got {tuple(out.shape)} of {out.dtype}")
    a = ffi.SoftmaxArgs()
    a.n_valid = n_valid
    a.dtype, a.rows, a.n, a.ld = _dt(out), rows, n, x.stride(0)
    a.x, a.scale, a.y_split, a.ldy = _ptr(x), scale, _ptr(out), out.stride(0)
    _call("idmvton_softmax_rows", a, bytes_=float(rows * n * (3 * 4 + 2 * out.element_size())))
    return out


def split(x, dtype, mode=ffi.SPLIT_ACT, out=None):
    """fp32 [rows][cols] -> operand pairs of the split-precision GEMMs: SPLIT_ACT [rows][2 cols] = [hi | lo]; SPLIT_W3 [rows][3 cols] =
    [hi | hi | lo]; SPLIT_W3T [cols][3 rows] = the W3 form of the transpose.  out: a tensor of that shape and `dtype` (row stride out.stride(0))
    to write instead of a new one."""
    rows, cols = x.shape
    shape = {ffi.SPLIT_ACT: (rows, 2 * cols), ffi.SPLIT_W3: (rows, 3 * cols), ffi.SPLIT_W3T: (cols, 3 * rows)}[mode]
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != dtype:
        raise ValueError(f"split(out=...): needs shape {shape} of {dtype}, got {tuple(out.shape)} of {out.dtype}")
    a = ffi.SplitArgs()
    a.dtype, a.mode, a.rows, a.cols = _dt(out), mode, rows, cols
    a.src, a.lds, a.dst, a.ldd = _ptr(x), x.stride(0), _ptr(out), out.stride(0)
    _call("idmvton_split", a, bytes_=float(rows * cols * 4 + out.numel() * out.element_size()))
    return out


def probe_mfma(which, a, b):
    c = torch.empty((64, 16), dtype=torch.float32, device=a.device)
    rc = ffi.lib().idmvton_probe_mfma(which, C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()),
                                      C.c_void_p(c.data_ptr()), C.c_void_p(_stream()))
    if rc != 0:
        raise RuntimeError(ffi.lib().idmvton_last_error().decode())
    return c


load_tune()
