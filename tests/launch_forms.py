"""The LAUNCH FORM of an idmvton_gemm_conv call: everything in its argument struct that selects a code path of the library, and no sizes.

idmvton_gemm_conv is one entry point whose behaviour is a product of options (the gather: plain Linear, k x k taps, stride, fused upsample,
several tensors, shortcut segments, the 1-D row re-pitch; the epilogue: bias, rowbias, colscale, activation, residual, the output type, the V^T
part, the access width).  gemm_form(args) reduces an ffi.GemmConvArgs -- what ops.RECORD stores for every launch -- to a hashable named tuple of
those choices.  Two launches that differ only in M, N, K, pointers, strides or the tile share a form; a launch that takes another branch of
csrc/gemm_conv.hip / csrc/gemm_common.cuh has another.  tests/test_launch_forms_gpu.py holds the set of forms the product issues against the set
the kernel checks launch.  Nothing here needs a GPU (tests/test_launch_forms_cpu.py builds the structs by hand)."""
import collections

from idm_vton_amd import ffi

GemmForm = collections.namedtuple("GemmForm", "gather taps stride ups tensors shortcut mode xattn_segs bias rowbias colscale res out vt width")
GemmForm.__doc__ = """gather     'lin' (one segment, no geometry), 'rows_pad' / 'rows_crop' (Ho == Hi == 1, one segment, Wo > Wi / Wo < Wi: an image row re-pitched to
           more rows -- the surplus reads outside the image -- or to fewer), 'conv' (anything else)
taps       distinct (dy, dx) of the segments (1 for lin / rows_*)
stride     the conv stride
ups        0, '2x' (the output grid is exactly 2Hi x 2Wi) or 'short' (one row and / or column short of it)
tensors    'one' or 'many' distinct tensors read by the segments
shortcut   centre-tap (0, 0) segments follow a k x k set with k > 1 (the fused 1x1 conv_shortcut)
mode       NONE / GEGLU / GELU / QUICKGELU / XATTN;  xattn_segs: key segments of an XATTN epilogue (0 otherwise)
bias, res  'none' / '16' / 'f32';  rowbias, colscale (colscale_n > 0): bool
out        'none' / '16' / 'f32' / 'e4m3'
vt         'none' or (vt_n0 'zero' | 'pos', key order, e4m3 slots) -- with e4m3 the library ignores vt_perm, so key order is False there
width      'wide' (16-byte epilogue accesses) or 'narrow' (8-byte), by the rule of include/idmvton_hip.h (tile_hint)"""

MODES = {ffi.EPI_NONE: "NONE", ffi.EPI_GEGLU: "GEGLU", ffi.EPI_GELU: "GELU", ffi.EPI_QUICKGELU: "QUICKGELU", ffi.EPI_XATTN: "XATTN"}


def _a16(p):
    return (p or 0) % 16 == 0


def epilogue_is_wide(a):
    """The header's rule (tile_hint): 16-byte accesses when N, the output's column count (N / 2 under GEGLU) and colscale_n are multiples of 8,
    every epilogue operand that is present (out, res, bias, rowbias) is 16-byte aligned with a stride that is a multiple of 8, and bit 15 of the
    hint is clear."""
    n_out = a.N // 2 if a.mode == ffi.EPI_GEGLU else a.N
    return bool(n_out % 8 == 0 and a.N % 8 == 0 and a.colscale_n % 8 == 0 and
                (not a.out or (a.ldo % 8 == 0 and _a16(a.out))) and (not a.res or (a.ldr % 8 == 0 and _a16(a.res))) and
                (not a.bias or _a16(a.bias)) and (not a.rowbias or (a.rowbias_ld % 8 == 0 and _a16(a.rowbias))) and
                (not a.vt or a.vt_n0 % 8 == 0) and not (a.tile_hint & 0x8000))


def gemm_form(a):
    """ffi.GemmConvArgs -> GemmForm.  `a.xattn`, when set, must still point at a live struct (reduce a record while its keep-alive tuple exists)."""
    segs = [a.seg[i] for i in range(a.nseg)]
    taps = []
    for s in segs:
        if (s.dy, s.dx) not in taps:
            taps.append((s.dy, s.dx))
    one_row = a.nseg == 1 and a.Ho == 1 and a.Hi == 1 and a.stride == 1 and not a.ups and taps == [(0, 0)]
    if one_row and a.Wo == a.M and a.Wi == a.M:
        gather = "lin"
    elif one_row and a.Wo > a.Wi:
        gather = "rows_pad"
    elif one_row and a.Wo < a.Wi:
        gather = "rows_crop"
    else:
        gather = "conv"
    ups = 0
    if a.ups:
        ups = "2x" if (a.Ho == 2 * a.Hi and a.Wo == 2 * a.Wi) else "short"
    # a k x k set (k > 1) is over once a (0, 0) segment follows a segment of another tap that is not followed by another tap of the set
    shortcut = False
    if len(taps) > 1:
        last_other = max(i for i, s in enumerate(segs) if (s.dy, s.dx) != (0, 0))
        shortcut = last_other < a.nseg - 1
    f8 = bool(a.io_flags & ffi.IO_OUT_F8)
    kind = lambda p, flag: "none" if not p else ("f32" if a.io_flags & flag else "16")
    out = "none" if not a.out else ("e4m3" if f8 else kind(a.out, ffi.IO_OUT_F32))
    vt = "none"
    if a.vt:
        vt = ("zero" if a.vt_n0 == 0 else "pos", bool(a.vt_perm) and not f8, f8)
    xs = a.xattn.contents.nseg if (a.mode == ffi.EPI_XATTN and a.xattn) else 0
    return GemmForm(gather=gather, taps=len(taps), stride=a.stride, ups=ups, tensors="one" if len({s.ptr for s in segs}) == 1 else "many",
                    shortcut=shortcut, mode=MODES.get(a.mode, a.mode), xattn_segs=xs, bias=kind(a.bias, ffi.IO_BIAS_F32), rowbias=bool(a.rowbias),
                    colscale=a.colscale_n > 0, res=kind(a.res, ffi.IO_RES_F32), out=out, vt=vt, width="wide" if epilogue_is_wide(a) else "narrow")


def describe(form):
    """One line per field: what the closure test prints for a form the checks do not launch."""
    return "\n".join(f"    {k:<10} = {v!r}" for k, v in form._asdict().items())


def recorded_forms(records):
    """ops.RECORD entries -> the set of GEMM forms among them (the keep-alive tuples are not kept)."""
    return {gemm_form(r[2]) for r in records if r[0] == "gemm"}
