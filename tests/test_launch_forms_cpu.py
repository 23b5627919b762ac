"""tests/launch_forms.py on hand-built ffi.GemmConvArgs: every field of the form follows the struct member that selects the code path, and
nothing else (M, N, K, pointers, strides that keep their alignment class, the tile) moves it.  No GPU, no library."""
import ctypes as C

import pytest

from idm_vton_amd import ffi
from tests.launch_forms import GemmForm, describe, epilogue_is_wide, gemm_form, recorded_forms

X, X2, W, OUT, BIAS, RB, RES, VT = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000, 0x80000   # 16-byte aligned addresses


def lin(M=512, N=256, K=128, **kw):
    a = ffi.GemmConvArgs()
    a.dtype, a.w, a.N, a.Ktot, a.nseg = ffi.F16, W, N, K, 1
    a.seg[0].ptr, a.seg[0].pitch, a.seg[0].len = X, K, K
    a.M, a.Ho, a.Wo, a.Hi, a.Wi, a.stride, a.ups = M, 1, M, 1, M, 1, 0
    a.out, a.ldo = OUT, N
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def conv(k=3, pad=1, stride=1, ups=0, H=8, Wd=8, Ho=None, Wo=None, C_=64, ptrs=(X,), extra=0, **kw):
    """k x k taps, each read from every tensor of `ptrs` (two pointers: the skip concat), then `extra` centre-tap segments of another tensor."""
    a = lin(**kw)
    taps = [(ky - pad, kx - pad) for ky in range(k) for kx in range(k)]
    i = 0
    for dy, dx in taps:
        for p in ptrs:
            s = a.seg[i]
            s.ptr, s.pitch, s.len, s.dy, s.dx = p, C_, C_, dy, dx
            i += 1
    for _ in range(extra):
        s = a.seg[i]
        s.ptr, s.pitch, s.len, s.dy, s.dx = X2, C_, C_, 0, 0
        i += 1
    a.nseg, a.Ktot = i, i * C_
    a.Hi, a.Wi, a.stride, a.ups = H, Wd, stride, ups
    a.Ho = Ho if Ho is not None else (2 * H if ups else (H + stride - 1) // stride)
    a.Wo = Wo if Wo is not None else (2 * Wd if ups else (Wd + stride - 1) // stride)
    a.M = 2 * a.Ho * a.Wo
    return a


BASE = GemmForm(gather="lin", taps=1, stride=1, ups=0, tensors="one", shortcut=False, mode="NONE", xattn_segs=0, bias="none", rowbias=False,
                colscale=False, res="none", out="16", vt="none", width="wide")


def test_plain_linear_is_the_base_form():
    assert gemm_form(lin()) == BASE
    assert "gather" in describe(BASE) and "'lin'" in describe(BASE)
    assert hash(gemm_form(lin())) == hash(BASE) and str(BASE).startswith("GemmForm(")


@pytest.mark.parametrize("kw", [dict(M=7), dict(M=100000, N=1280, K=5120), dict(N=8), dict(w=W + 4096), dict(out=OUT + 160, ldo=264),
                                dict(tile_hint=(1 << 28) | (128 << 16) | 64), dict(tile_hint=(6 << 28) | (320 << 16) | 192), dict(dtype=ffi.BF16),
                                dict(colscale=0.5), dict(f8_out_scale=4.0), dict(rows_per_group=9), dict(vt_tokens=64), dict(vt_perm=1)],
                         ids=lambda kw: ",".join(kw))
def test_sizes_pointers_and_tile_do_not_change_the_form(kw):
    assert gemm_form(lin(**kw)) == BASE


def test_two_convs_of_different_sizes_share_a_form():
    assert gemm_form(conv(H=8, Wd=8, C_=64)) == gemm_form(conv(H=33, Wd=25, C_=320, N=640, tile_hint=(1 << 28) | (64 << 16) | 64))


CHANGES = [
    ("bias16", dict(bias=BIAS), dict(bias="16")),
    ("bias_f32", dict(bias=BIAS, io_flags=ffi.IO_BIAS_F32), dict(bias="f32")),
    ("rowbias", dict(rowbias=RB, rowbias_ld=256, rows_per_group=4), dict(rowbias=True)),
    ("colscale", dict(colscale_n=64, colscale=0.18), dict(colscale=True)),
    ("res16", dict(res=RES, ldr=256), dict(res="16")),
    ("res_f32", dict(res=RES, ldr=256, io_flags=ffi.IO_RES_F32), dict(res="f32")),
    ("out_f32", dict(io_flags=ffi.IO_OUT_F32), dict(out="f32")),
    ("out_e4m3", dict(io_flags=ffi.IO_OUT_F8, f8_out_scale=4.0), dict(out="e4m3")),
    ("gelu", dict(mode=ffi.EPI_GELU), dict(mode="GELU")),
    ("quick_gelu", dict(mode=ffi.EPI_QUICKGELU), dict(mode="QUICKGELU")),
    ("geglu", dict(mode=ffi.EPI_GEGLU), dict(mode="GEGLU")),
    ("vt_plain", dict(vt=VT, vt_n0=128, vt_tokens=64, vt_perm=0), dict(vt=("pos", False, False))),
    ("vt_key_order", dict(vt=VT, vt_n0=128, vt_tokens=64, vt_perm=1), dict(vt=("pos", True, False))),
    ("vt_only", dict(vt=VT, vt_n0=0, vt_tokens=64, vt_perm=0, out=None, ldo=0), dict(vt=("zero", False, False), out="none")),
    ("vt_e4m3", dict(vt=VT, vt_n0=128, vt_tokens=64, vt_perm=1, io_flags=ffi.IO_OUT_F8), dict(vt=("pos", False, True), out="e4m3")),
    ("narrow_forced", dict(tile_hint=(1 << 28) | (128 << 16) | 64 | 0x8000), dict(width="narrow")),
    ("narrow_N", dict(N=132, ldo=132), dict(width="narrow")),
    ("narrow_ldo", dict(ldo=260), dict(width="narrow")),
    ("narrow_out_ptr", dict(out=OUT + 8), dict(width="narrow")),
    ("narrow_res_ptr", dict(res=RES + 8, ldr=256), dict(res="16", width="narrow")),
    ("narrow_ldr", dict(res=RES, ldr=260), dict(res="16", width="narrow")),
    ("narrow_bias_ptr", dict(bias=BIAS + 8), dict(bias="16", width="narrow")),
    ("narrow_rowbias_ld", dict(rowbias=RB, rowbias_ld=260, rows_per_group=4), dict(rowbias=True, width="narrow")),
    ("narrow_rowbias_ptr", dict(rowbias=RB + 8, rowbias_ld=256, rows_per_group=4), dict(rowbias=True, width="narrow")),
    ("narrow_colscale_n", dict(colscale_n=60, colscale=0.18), dict(colscale=True, width="narrow")),
    ("narrow_geglu_half", dict(mode=ffi.EPI_GEGLU, N=72, ldo=40), dict(mode="GEGLU", width="narrow")),
]


@pytest.mark.parametrize("name,kw,expect", CHANGES, ids=[c[0] for c in CHANGES])
def test_each_epilogue_member_changes_its_field_only(name, kw, expect):
    f = gemm_form(lin(**kw))
    assert f == BASE._replace(**expect), describe(f)
    assert f != BASE


def test_every_epilogue_change_gives_a_distinct_form():
    forms = [gemm_form(lin(**kw)) for _, kw, _ in CHANGES]
    assert len({f._replace(width="wide") for f in forms if f.width == "wide"}) == sum(f.width == "wide" for f in forms)


def test_xattn_counts_its_key_segments():
    for n in (1, 2):
        xa = ffi.XAttn()
        xa.nseg = n
        a = lin(mode=ffi.EPI_XATTN)
        a.xattn = C.pointer(xa)
        f = gemm_form(type(a).from_buffer_copy(a))              # what ops.RECORD keeps: a copy of the struct, the pointer still live
        assert f == BASE._replace(mode="XATTN", xattn_segs=n)


def test_gather_forms():
    M = 3 * 112
    pad = gemm_form(lin(M=M, Wo=112, Wi=100))
    crop = gemm_form(lin(M=300, Wo=100, Wi=112))
    assert pad == BASE._replace(gather="rows_pad") and crop == BASE._replace(gather="rows_crop")
    c3 = gemm_form(conv())
    assert c3 == BASE._replace(gather="conv", taps=9)
    assert gemm_form(conv(k=1, pad=0)) == BASE._replace(gather="conv")                       # a 1x1 conv with a geometry is not `lin`
    assert gemm_form(conv(stride=2)) == c3._replace(stride=2)
    assert gemm_form(conv(k=3, pad=0, stride=2)) == c3._replace(stride=2)                    # the VAE's pad-(0,1,0,1) downsample: taps 0..2
    assert gemm_form(conv(ups=1)) == c3._replace(ups="2x")
    assert gemm_form(conv(ups=1, H=9, Wd=13, Ho=17, Wo=26)) == c3._replace(ups="short")
    assert gemm_form(conv(ups=1, H=9, Wd=13, Ho=18, Wo=25)) == c3._replace(ups="short")
    assert gemm_form(conv(ptrs=(X, X2))) == c3._replace(tensors="many")
    assert gemm_form(conv(extra=1)) == c3._replace(tensors="many", shortcut=True)
    assert gemm_form(conv(ptrs=(X, X2), extra=2)) == c3._replace(tensors="many", shortcut=True)
    assert gemm_form(conv(k=1, pad=0, ptrs=(X, X2), extra=1)) == BASE._replace(gather="conv", tensors="many")   # all centre taps: no k x k set before
    two = lin(K=192)                                                                         # [hi | lo] operand pairs: one tensor read twice, no geometry
    two.nseg = 2
    two.seg[1].ptr, two.seg[1].pitch, two.seg[1].len = X, 128, 64
    assert gemm_form(two) == BASE._replace(gather="conv")
    forms = [pad, crop, c3, gemm_form(conv(stride=2)), gemm_form(conv(ups=1)), gemm_form(conv(ups=1, H=9, Wd=13, Ho=17, Wo=26)),
             gemm_form(conv(ptrs=(X, X2))), gemm_form(conv(extra=1)), BASE]
    assert len(set(forms)) == len(forms)


def test_width_rule_is_the_librarys():
    """epilogue_is_wide mirrors csrc/gemm_conv.hip (p.wide): each clause on its own."""
    assert epilogue_is_wide(lin())
    assert epilogue_is_wide(lin(out=None, ldo=0, vt=VT, vt_n0=0, vt_tokens=64))              # no `out`: its stride does not count
    assert not epilogue_is_wide(lin(N=260, ldo=264))
    assert epilogue_is_wide(lin(mode=ffi.EPI_GEGLU, N=128, ldo=64)) and not epilogue_is_wide(lin(mode=ffi.EPI_GEGLU, N=72, ldo=40))
    assert epilogue_is_wide(lin(colscale_n=64)) and not epilogue_is_wide(lin(colscale_n=68))
    assert not epilogue_is_wide(lin(tile_hint=0x8000 | (1 << 28) | (64 << 16) | 64))


def test_recorded_forms_reads_ops_record_entries():
    recs = [("gemm", "k", lin(), ()), ("attn", "k", object(), ()), ("gemm", "k", lin(M=9), ()), ("gemm", "k", lin(mode=ffi.EPI_GELU), ())]
    assert recorded_forms(recs) == {BASE, BASE._replace(mode="GELU")}
