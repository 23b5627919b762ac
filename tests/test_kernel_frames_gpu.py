"""-m gpu: every C-ABI op on FRAMED operands (tests/frames.py): each tensor at a row stride wider than its logical width, inside a buffer
whose gap columns and guard bands hold NaN, with what the header calls masked / not read poisoned too.  The reference arithmetic and the
bars are those of tests/kernel_checks.py (TOL, and the 1.2e-1 / 3e-2 of the fp8 kernel): framing changes no arithmetic, so no bar is new.
Per case:
  1. the result is finite and within the op's bar;
  2. every output's frame is bit-intact and every output element was written; every input buffer is bit-equal to what it was given;
  3. where the tile / kernel is named (a tile_hint, a tune word), the result is BIT-EQUAL to the tight launch of the same instantiation on
     the same values (the one exception: framing that itself selects the other epilogue width, see test_linear_epilogue_width_by_alignment).
Shapes are the smallest with an M tail, an N tail, a partial last key tile and more than one batch."""
import pytest
import torch
from hypothesis import HealthCheck, given, settings, strategies as st

from tests import kernel_checks as kc
from tests.engine_support import no_tune_table
from tests.frames import Framed, Tight
from tests.kernel_checks import TUNES

pytestmark = pytest.mark.gpu
DEV = "cuda"
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
F8_SDPA_BAR, F8_KERNEL_BAR = 1.2e-1, 3e-2                # stated in tests/kernel_checks.py (all_checks) and include/idmvton_hip.h
SPLIT_BAR = 2e-5                                         # the split-precision bar of all_checks

V0_TILES = (((128 << 16) | 128, "v0_128x128"), ((128 << 16) | 64, "v0_128x64"), ((64 << 16) | 64, "v0_64x64"))
TILES_A = ((0, "auto"),) + V0_TILES + tuple(kc.RING_TILES)
TILE = pytest.mark.parametrize("hint", [h for h, _ in TILES_A], ids=[t for _, t in TILES_A])
BN = lambda hint: (hint >> 16) & 0xfff


def run_both(check, tol, framed, equal=("out",), named=True, **kw):
    """check(alloc=Tight) and check(alloc=framed) on the same values: the framed error within `tol`, its frames verified, and (named: the
    instantiation is the caller's, not the library's choice) the named outputs bit-equal between the two."""
    tight = Tight()
    e_t = check(alloc=tight, **kw)
    e_f = check(alloc=framed, **kw)
    worst = max(e_f) if isinstance(e_f, tuple) else e_f
    print(f"{check.__name__} {kw}: tight {e_t}, framed {e_f} (bar {tol})")
    if isinstance(tol, tuple):
        assert all(e <= t for e, t in zip(e_f, tol)), (e_f, tol)
    else:
        assert worst <= tol, (worst, tol)
    framed.verify()
    if named:
        for name in equal:
            a, b = tight.outs[name], framed.outs[name]
            assert torch.equal(a, b), (name, (a.float() - b.float()).abs().max().item())
    return tight, framed


# ------------------------------------------------------------------------------------------------------------------ Family A: gemm_conv
LIN = dict(M=515, N=328, K=192, rowbias=True, groups=5)  # M tail of every tile, N tail of every tile, 5 row groups of 103 rows


@DTYPES
@TILE
def test_linear_ragged_every_epilogue_operand_strided(hint, dtype):
    """x at row stride K + 64, out at ldo = N + 8, res at ldr = N + 16, rowbias at rowbias_ld = N + 8 (all 16-byte aligned: the wide epilogue)."""
    run_both(kc.check_linear, kc.TOL[dtype], Framed(pads=dict(x=64, out=8, res=16, rowbias=8)), named=bool(hint), dtype=dtype, dev=DEV, tile_hint=hint, **LIN)


@DTYPES
@TILE
@pytest.mark.parametrize("which", ["out", "res", "rowbias"])
def test_linear_epilogue_width_by_alignment(which, hint, dtype):
    """ONE epilogue operand 8-byte but not 16-byte aligned -- `out` at ldo = N + 4 starting 4 elements in; only `res`; only `rowbias` -- so the
    alignment test of gemm_conv.hip must take the 8-byte epilogue by shape (the header: 16-byte accesses only when every epilogue operand is
    16-byte aligned).  The result must be bit-equal to the tight launch of the same tile with the 8-byte epilogue forced (bit 15 of the hint:
    the same instantiation), and to the tight launch with the 16-byte epilogue as well: both epilogues apply the same fp32 operations in the
    same order to the same accumulators and round once (the 320-column tile hands a launch it cannot take wide to the 128x256 ring tile, which
    walks K in the same 64-wide steps).  No bar is relaxed for the misaligned form: TOL."""
    pads = dict(x=64, out=8, res=16, rowbias=8)
    pads[which] = 4
    framed = Framed(pads=pads, leads={which: 4})
    tight, _ = run_both(kc.check_linear, kc.TOL[dtype], framed, named=bool(hint), dtype=dtype, dev=DEV, tile_hint=hint, **LIN)
    ptr = framed.outs["out"].data_ptr() if which == "out" else next(v for n, v in framed.inputs if n == which).data_ptr()
    assert ptr % 16 == 8                                 # the operand really is misaligned for 16-byte accesses
    if hint:
        narrow = Tight()
        kc.check_linear(alloc=narrow, dtype=dtype, dev=DEV, tile_hint=hint | 0x8000, **LIN)
        assert torch.equal(narrow.outs["out"], framed.outs["out"])


@DTYPES
@pytest.mark.parametrize("hint", [h for h, _ in TILES_A if h == 0 or BN(h) >= 128], ids=[t for h, t in TILES_A if h == 0 or BN(h) >= 128])
def test_geglu_ragged_200x64_wide_ldo(hint, dtype):
    run_both(kc.check_geglu, kc.TOL[dtype], Framed(pads=dict(x=8, out=24)), named=bool(hint), M=200, C=64, dtype=dtype, dev=DEV, tile_hint=hint)


@DTYPES
@pytest.mark.parametrize("hint", [h for h, _ in TILES_A if h == 0 or 256 % BN(h) == 0], ids=[t for h, t in TILES_A if h == 0 or 256 % BN(h) == 0])
def test_vt_projection_out_strided_vt_framed(hint, dtype):
    """B = 3, 80 tokens, C = 128: M = 240 is a tail for every tile; out at ldo = 2C + 8; V^T (contiguous by ABI) framed before and after, in
    both vt_perm forms.  (vt_n0 = 256 must be a multiple of the tile's BN: the library refuses the 320-column tile for this launch.)"""
    run_both(kc.check_vt, kc.TOL[dtype], Framed(pads=dict(x=8, out=8)), equal=("out", "vt", "vt_perm"), named=bool(hint), B=3, Ntok=80, C=128,
             dtype=dtype, dev=DEV, tile_hint=hint)


@DTYPES
@pytest.mark.parametrize("hint", [h for _, h in kc.F8_OUT_TILES], ids=[t for t, _ in kc.F8_OUT_TILES])
def test_vt_projection_e4m3_out_strided(hint, dtype):
    """IDMVTON_IO_OUT_F8 at 64 tokens per batch element: `out` bytes at ldo = 2C + 16 (byte pre-fill 0xff inside, 0x7f around: the kernels
    saturate and write neither), V^T bytes framed.  The check's own bar (0.0: within half an e4m3 ulp of the fp32 product)."""
    run_both(kc.check_gemm_f8_out, 0.0, Framed(pads=dict(x=8, out=16)), equal=("out", "vt"), named=bool(hint), dtype=dtype, dev=DEV, B=3, N=64,
             C=128, K=192, hint=hint)


ACTS = pytest.mark.parametrize("act", ["gelu", "quick_gelu"])


@DTYPES
@TILE
@ACTS
def test_activation_before_residual_out_res_rowbias_strided(act, hint, dtype):
    """The erf-GELU / quick-GELU epilogues with every operand strided: 16-bit output at the LIN shape (bias, rowbias, activation, then the
    residual), and fp32 output judged by the 2e-5 rule (check_linear scales it to TOL) -- the bar that tells the activations apart."""
    pads = dict(x=64, out=8, res=16, rowbias=8)
    run_both(kc.check_linear, kc.TOL[dtype], Framed(pads=pads), named=bool(hint), dtype=dtype, dev=DEV, tile_hint=hint, act=act, **LIN)
    run_both(kc.check_linear, kc.TOL[dtype], Framed(pads=pads), named=bool(hint), dtype=dtype, dev=DEV, tile_hint=hint, act=act, out_f32=True, **LIN)


@DTYPES
@TILE
@ACTS
def test_activation_narrow_by_shape_N132(act, hint, dtype):
    """N = 132 (N % 8 == 4): the 8-byte epilogue by shape, out at ldo = N + 4, res at ldr = N + 12."""
    run_both(kc.check_linear, kc.TOL[dtype], Framed(pads=dict(x=8, out=4, res=12)), named=bool(hint), dtype=dtype, dev=DEV, tile_hint=hint, act=act,
             **kc.ACT_SHAPE_N4)


VT_FORMS = [("bias", dict(bias=True)), ("colscale", dict(colscale=(128, kc.QS))), ("bias_colscale", dict(bias=True, colscale=(128, kc.QS))),
            ("colscale_n124_narrow", dict(bias=True, colscale=(124, kc.QS)))]


@DTYPES
@pytest.mark.parametrize("hint", [h for h, _ in TILES_A if h == 0 or 256 % BN(h) == 0], ids=[t for h, t in TILES_A if h == 0 or 256 % BN(h) == 0])
@pytest.mark.parametrize("form", [f for _, f in VT_FORMS], ids=[n for n, _ in VT_FORMS])
def test_vt_projection_with_bias_and_colscale(form, hint, dtype):
    """The engine's QKV projection (colscale on the q columns, V^T in both orders) and the boundary's (a bias on top): out at ldo = 2C + 8, V^T
    framed; colscale_n = C - 4 takes the 8-byte epilogue."""
    run_both(kc.check_vt, kc.TOL[dtype], Framed(pads=dict(x=8, out=8)), equal=("out", "vt", "vt_perm"), named=bool(hint), dtype=dtype, dev=DEV,
             tile_hint=hint, **kc.VT_SHAPE, **form)


@DTYPES
@TILE
def test_vt_only_projection_with_bias(hint, dtype):
    """vt_n0 = 0, out = NULL, plain transpose, bias: the 16-bit VAE mid-block's to_v.  V^T framed before and after."""
    run_both(kc.check_vt, kc.TOL[dtype], Framed(pads=dict(x=8)), equal=("vt",), named=bool(hint), dtype=dtype, dev=DEV, tile_hint=hint, bias=True,
             vt_n0_zero=True, **kc.VT_SHAPE)


@DTYPES
@TILE
@pytest.mark.parametrize("shape", [(100, 128, 192), (63, 64, 72)], ids=["N100_128_to_192", "N63_64_to_72"])
def test_row_repitch_pad_rows_hold_the_bias_crop_never_reads_them(shape, hint, dtype):
    """proj_in / proj_out of a latent whose H*W is no multiple of 16: the padded rows read outside the image (they must hold exactly the bias), the
    cropping launch reads a source whose pad rows are NaN; source, outputs and residual strided."""
    N, Cin, Cout = shape
    run_both(kc.check_row_repitch, kc.TOL[dtype], Framed(pads=dict(x=8, src=8, pad16=8, pad32=8, crop=8, res=16)), equal=("pad16", "pad32", "crop"),
             named=bool(hint), B=3, N=N, Cin=Cin, Cout=Cout, dtype=dtype, dev=DEV, tile_hint=hint)


CONVS = [("3x3", kc.check_conv, dict(B=2, Cin=128, Cout=136, H=9, W=7, temb=True)),
         ("3x3_s2", kc.check_conv, dict(B=2, Cin=128, Cout=192, H=17, W=13, stride=2)),
         ("3x3_ups", kc.check_conv, dict(B=2, Cin=128, Cout=128, H=9, W=7, ups=True)),
         ("3x3_ups_odd_grid", kc.check_conv_ups_odd, dict(B=1, Cin=64, Cout=192, H=9, W=13, Ho=17, Wo=26)),
         ("1x1_two_pointers_shortcut_temb_res", kc.check_conv, dict(B=2, Cin=320, Cout=72, H=12, W=10, k=1, split=192, shortcut=128, temb=True, res=True))]


@DTYPES
@TILE
def test_conv_segments_read_a_channel_sub_range(hint, dtype):
    """Every activation tensor wider than what its segments read (coff = 8 > 0, coff + len < pitch = len + 24), the unread channels NaN:
    the skip-concat and [hi | lo] pattern of the product.  out / res / rowbias strided."""
    for name, check, kw in CONVS:
        run_both(check, kc.TOL[dtype], Framed(pads=dict(out=8, res=16, rowbias=8)), named=bool(hint), dtype=dtype, dev=DEV, tile_hint=hint, **kw)


@DTYPES
@TILE
def test_fp32_stream_res_and_out_strided(hint, dtype):
    """fp32 res at ldr = N + 16 (fp32 elements), fp32 out at ldo = N + 8, then LayerNorm of the strided fp32 result."""
    run_both(kc.check_stream_f32, kc.TOL[dtype], Framed(pads=dict(x=64, out=8, out16=8, out32_res16=8, res=16, res16=16, ln_y=24)),
             equal=("out", "out16", "out32_res16", "ln_y"), named=bool(hint), M=515, N=328, K=192, dtype=dtype, dev=DEV, tile_hint=hint)


def test_split_precision_linear_and_conv_fp32_bias_in_a_frame():
    pads = dict(xp=16, xs=16, out=8, res=16)
    for kw in (dict(M=1000, N=64, K=128), dict(M=203, N=136, K=64, exact_w=True), dict(M=200, N=72, K=128, res=False),
               dict(M=203, N=136, K=64, res=False, colscale=(136, 136 ** -0.5)), dict(M=203, N=136, K=128, res=False, bias=False)):
        run_both(kc.check_plin, SPLIT_BAR, Framed(pads=pads), dev=DEV, **kw)
    for kw in (dict(B=1, Cin=128, Cout=128, H=16, W=12, shortcut=256), dict(B=2, Cin=128, Cout=136, H=9, W=7, ups=True),
               dict(B=1, Cin=128, Cout=64, H=8, W=8, shortcut=128, exact_w=True), dict(B=2, Cin=128, Cout=136, H=9, W=7, res=True)):
        run_both(kc.check_pconv, SPLIT_BAR, Framed(pads=pads), dev=DEV, **kw)


XATTN_TILES = ((0, "auto"), (kc._hint(1, 128, 64), "128x64"), (kc._hint(1, 128, 128), "128x128"), (kc._hint(1, 128, 256), "128x256"), (kc._hint(6, 128, 128), "w8_128x128"))


@DTYPES
@pytest.mark.parametrize("hint", [h for h, _ in XATTN_TILES], ids=[t for _, t in XATTN_TILES])
def test_fused_cross_attention_nan_key_rows_large_vt_filler(hint, dtype):
    """K rows nk..k_rows-1 NaN (masked), V^T positions of keys >= nk 1.0e4 (finite), K at ldk = C + 8, V^T at ldvt = k_rows + 16, out strided."""
    pads = dict(x=8, out=8, k0=8, k1=8, vt0=16, vt1=16)
    for kw in (dict(B=3, heads=2, N=160, K=128, n_text=33, n_ip=5), dict(B=2, heads=2, N=96, K=192, n_text=77, n_ip=16)):
        run_both(kc.check_xattn_fused, kc.TOL[dtype], Framed(pads=pads), named=bool(hint), dtype=dtype, dev=DEV, tile_hint=hint, **kw)


# ------------------------------------------------------------------------------------------------------------------ Family B: attention


@DTYPES
@pytest.mark.parametrize("entry", kc.ENTRIES)
@pytest.mark.parametrize("tune", list(TUNES), ids=list(TUNES))
def test_self_attention_in_the_products_geometry(tune, entry, dtype, monkeypatch):
    """q | k column halves of one buffer (ldq = ldk = 2C), out at ldo = C + 8, own segment B = 3, 2 heads, 200 queries, nk = 200 of k_rows = 208,
    garment segment 72 keys of 80 rows from batch 1 on, ldvt > round16(nk); NaN key rows, 1.0e4 in V^T beyond nk; through every entry point."""
    no_tune_table(monkeypatch)
    run_both(kc.check_attn_product, kc.TOL[dtype], Framed(pads=dict(out=8, kg=8)), named=bool(TUNES[tune]), dtype=dtype, dev=DEV, tune=TUNES[tune], entry=entry)


RAW_Q = [t for t in TUNES if ((TUNES[t] >> 16) & 0xff) not in (7, 8, 16)]       # kernels 7, 8 and 16 need a pre-multiplied q


@DTYPES
@pytest.mark.parametrize("tune", RAW_Q, ids=RAW_Q)
def test_self_attention_in_the_resamplers_geometry(tune, dtype, monkeypatch):
    """16 raw latent queries against 257 keys in 272 rows plus the 16 latent keys (Nq != round16(nk), q not pre-multiplied): key rows 257..271
    NaN -- in the Resampler they hold the projection of zero rows through a LayerNorm: finite, non-zero --, V^T 1.0e4 beyond the keys."""
    no_tune_table(monkeypatch)
    run_both(kc.check_attn_product, kc.TOL[dtype], Framed(pads=dict(out=8, kg=8)), named=bool(TUNES[tune]), dtype=dtype, dev=DEV, tune=TUNES[tune],
             **kc.RESAMPLER_GEOMETRY)


@DTYPES
@pytest.mark.parametrize("entry", kc.ENTRIES)
def test_fp8_attention_in_the_products_geometry(entry, dtype):
    """The same geometry in bytes; K rows >= nk e4m3 NaN, the V^T tail inside the last 64-key tile zero (the header says zero), NaN beyond it."""
    run_both(kc.check_attn_product, (F8_SDPA_BAR, F8_KERNEL_BAR), Framed(pads=dict(out=8)), dtype=dtype, dev=DEV, entry=entry, f8=True)


@DTYPES
@pytest.mark.parametrize("tune", ["auto", "k0_2stage_4w", "k0_ring3_4w", "k0_2stage_8w"])
def test_cross_attention_key_rows_96_and_32(tune, dtype, monkeypatch):
    """77 / 16 keys in K tables of 96 / 32 rows (rows from nk on NaN), V^T 1.0e4 beyond nk at ldvt = round16(nk) + 16, q / K / out strided."""
    no_tune_table(monkeypatch)
    run_both(kc.check_attn_cross, kc.TOL[dtype], Framed(pads=dict(q=8, out=8, k0=8, k1=8)), named=bool(TUNES[tune]), B=2, heads=2, N=200, dtype=dtype,
             dev=DEV, ip_scale=0.5, tune=TUNES[tune], k_rows=(96, 32))


@DTYPES
@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("d", [64, 80, 32])
def test_attn_small_fused_qkv_buffer_strided_out(d, causal, dtype):
    """q / k / v inside one [B][L][3H] buffer (itself at a wider row stride), out strided, fewer queries than keys."""
    run_both(kc.check_attn_small, kc.TOL[dtype], Framed(pads=dict(qkv=8, q=8, out=8)), B=3, heads=2, L=77, d=d, dtype=dtype, dev=DEV, causal=causal, Lq=37)


# ------------------------------------------------------------------------------------------------------------------ Family C: norms, softmax, split, quant
@DTYPES
@pytest.mark.parametrize("x_f32", [False, True], ids=["x16", "x_f32"])
@pytest.mark.parametrize("C", [64, 1280, 2048])
def test_layernorm_three_different_strides(C, x_f32, dtype):
    run_both(kc.check_layernorm, kc.TOL[dtype], Framed(pads=dict(x=8, y=16, y2=24)), equal=("y", "y2"), rows=37, Cc=C, dtype=dtype, dev=DEV, x_f32=x_f32)


@DTYPES
@pytest.mark.parametrize("shape", [dict(B=2, HW=300, Cc=320), dict(B=2, HW=300, Cc=1920, split=1280), dict(B=2, HW=192, Cc=2560, split=1280)],
                         ids=["320x300", "1920_split_1280", "2560_split_1280"])
def test_groupnorm_frames_and_exact_scratch(shape, dtype):
    """x, x2, y framed before and after; the stats scratch EXACTLY gn_stats_doubles(...) long inside a NaN frame: not one double more is written."""
    run_both(kc.check_groupnorm, kc.TOL[dtype], Framed(), equal=("y",), dtype=dtype, dev=DEV, **shape)


def test_groupnorm_precise_frames_and_exact_scratch():
    run_both(kc.check_gn_precise, SPLIT_BAR, Framed(), equal=("y",), B=2, HW=300, Cc=512, dev=DEV)


@DTYPES
@pytest.mark.parametrize("n_valid", [0, 825])
def test_softmax_rows_gap_columns_untouched(n_valid, dtype):
    """ld = n + 8: columns [n_valid, n) become 0 (the check's tail term), columns [n, ld) keep their NaN."""
    run_both(kc.check_softmax_rows, kc.TOL[dtype], Framed(), equal=("x",), rows=37, n=832, dtype=dtype, dev=DEV, n_valid=n_valid)


@pytest.mark.parametrize("n_valid", [0, 825])
def test_softmax_rows_split_fp32_source_intact(n_valid):
    """ld = n + 4 (fp32), ldy = 2n + 8; the fp32 source is an input of the policy: bit-intact after the launch, as the header promises."""
    run_both(kc.check_softmax_split, SPLIT_BAR, Framed(pads=dict(x=4, y=8)), equal=("y",), rows=37, n=832, dev=DEV, n_valid=n_valid)


@pytest.mark.parametrize("shape", [(200, 72), (768, 512)], ids=["200x72", "768x512"])
@pytest.mark.parametrize("mode", ["act", "w3", "w3t"])
def test_split_strided_source_and_destination(mode, shape):
    from idm_vton_amd import ffi
    m = dict(act=ffi.SPLIT_ACT, w3=ffi.SPLIT_W3, w3t=ffi.SPLIT_W3T)[mode]
    run_both(kc.check_split, 1e-7, Framed(pads=dict(src=4, dst=8)), equal=("dst",), rows=shape[0], cols=shape[1], dev=DEV, mode=m)


@DTYPES
def test_quant_f8_strided(dtype):
    """Mode 0 (lds = cols + 8, ldd = cols + 16: the gap bytes stay) and mode 1 with 208 keys at lds = 216, ldd = 320: the last 64-key tile of the
    keys is partial, and mode 1 writes its whole row of ldd bytes (zero from the key count on), so its destination has no gap, only a frame."""
    run_both(kc.check_quant_f8, 0.0, Framed(pads=dict(src=8, vt16=8, dst=16)), equal=("dst", "dst_vt"), dtype=dtype, dev=DEV, vt_ldd=320)


# ------------------------------------------------------------------------------------------------------------------ Family D: elementwise
@DTYPES
@pytest.mark.parametrize("null_noise", [False, True], ids=["noise", "null_noise"])
def test_elementwise_odd_grid_poisoned_pad_channels(null_noise, dtype):
    """B = 3, 15 x 13 pixels (B * hw is no multiple of the 256-thread block): pack_input cpad 64; cfg_step ldc 64 with channels 4.. NaN; to_nhwc /
    to_nchw with cpad 64 > C and NaN pad channels in the to_nchw source; vae_sample ldm 16 with columns 8.. NaN."""
    run_both(kc.check_elementwise, kc.TOL[dtype], Framed(), equal=("packed", "latents_step", "nhwc", "nchw_back", "z"), B=3, h=15, w=13, dtype=dtype,
             dev=DEV, ldm=16, null_noise=null_noise)


def test_layout_split_and_fp32_nhwc_flags():
    run_both(kc.check_layout_split, SPLIT_BAR, Framed(), equal=("nhwc_split", "nchw_back"), B=3, h=15, w=13, dev=DEV)


# ------------------------------------------------------------------------------------------------------------------ drawn shapes
CFG = settings(max_examples=30, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
DT = st.sampled_from([torch.float16, torch.bfloat16])
PAD = st.sampled_from([0, 4, 8, 24])


@CFG
@given(M=st.integers(1, 700), n4=st.integers(1, 120), k64=st.integers(1, 5), hint=st.sampled_from([h for h, _ in TILES_A]), pad_x=st.sampled_from([0, 8, 24]), pad_out=PAD,
       pad_res=PAD, lead_out=st.sampled_from([0, 4, 8]), dt=DT)
def test_framed_linear_any_shape(M, n4, k64, hint, pad_x, pad_out, pad_res, lead_out, dt):
    """(M, N, K, tile, pad_x, pad_out, pad_res, lead_out): pads from {0, 4, 8, 24}, lead from {0, 4, 8} elements; pad_x from the members of
    that set the ABI admits for a segment pitch (a multiple of 8: a pad of 4 is refused on the host)."""
    framed = Framed(pads=dict(x=pad_x, out=pad_out, res=pad_res, rowbias=pad_out), leads=dict(out=lead_out))
    e = kc.check_linear(M, 4 * n4, 64 * k64, dt, DEV, rowbias=True, tile_hint=hint, alloc=framed)
    assert e <= kc.TOL[dt], (M, 4 * n4, 64 * k64, dt, hint, e)
    framed.verify()


@CFG
@given(B=st.integers(2, 4), heads=st.integers(1, 3), nk=st.integers(17, 400), slack=st.integers(0, 2), n_garm=st.integers(1, 150), b0f=st.integers(0, 3),
       tune=st.sampled_from(list(TUNES)), entry=st.sampled_from(kc.ENTRIES), pad_out=st.sampled_from([0, 8, 24]), pad_kg=st.sampled_from([0, 8, 24]), dt=DT)
def test_framed_self_attention_any_shape(B, heads, nk, slack, n_garm, b0f, tune, entry, pad_out, pad_kg, dt):
    """(B, heads, own keys, k_rows, garment keys, b0, tune, entry point, pad_out, pad_k): the product's geometry on drawn sizes -- any key count
    (odd latent sizes), query rows = round16 of it, k_rows that or more (ldo, ldk multiples of 8)."""
    from idm_vton_amd import ops
    framed = Framed(pads=dict(out=pad_out, kg=pad_kg))
    N = ops.round16(nk)                                  # the product's rows: round16 of the real token count
    kw = dict(B=B, heads=heads, Nq=N, nk_own=nk, k_rows=N + 16 * slack, n_garm=n_garm, g_rows=ops.round16(n_garm) + 16, b0=min(b0f, B - 1))
    e = kc.check_attn_product(dt, DEV, tune=TUNES[tune], entry=entry, alloc=framed, **kw)
    assert e <= kc.TOL[dt], (kw, tune, entry, dt, e)
    framed.verify()
