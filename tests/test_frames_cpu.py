"""The framing harness (tests/frames.py) can fail: torch stand-ins for a kernel, addressed like one (flat memory, a start offset and a row
stride per operand), one of them right and the others wrong in exactly one way each.  The right one passes every assertion; every wrong one is
reported, at the element it got wrong.  No GPU, and no GPU test provokes anything: this file is the evidence that the checks bite."""
import pytest
import torch

from tests import frames as fr

M, N = 37, 24
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32, torch.float64], ids=["f16", "bf16", "f32", "f64"])


def _standin(x, y, bug=None):
    """y[r][c] = 2 x[r][c] + 1 over [M][N], through (memory, start, ld) triples as a kernel would."""
    xm, x0, ldx = x._frame.buf, x._frame.start, x._frame.ld
    ym, y0, ldy = y._frame.buf, y._frame.start, y._frame.ld
    f = lambda v: (2.0 * v.double() + 1.0).to(ym.dtype)
    for r in range(M):
        xs = x0 + r * (N if bug == "width_for_ldx" else ldx)
        ys = y0 + r * (N if bug == "width_for_ldy" else ldy)
        ym[ys:ys + N] = f(xm[xs:xs + N])
    if bug == "gap_store":
        ym[y0 + 5 * ldy + N] = 3.0                       # one element into the gap after column N of row 5
    elif bug == "row_past_M":
        ym[y0 + M * ldy:y0 + M * ldy + N] = f(xm[x0:x0 + N])
    elif bug == "store_before":
        ym[y0 - 1] = 3.0
    elif bug == "skip":
        fr.ints(ym)[y0 + 7 * ldy + 3] = y._frame.interior_bits
    elif bug == "gap_read":
        ym[y0 + 2 * ldy + N - 1] += xm[x0 + 2 * ldx + N].to(ym.dtype) * 0   # NaN * 0: the filler reaches the result even at weight zero
    elif bug == "input_store":
        xm[x0 + 4 * ldx + 1] = 0.5


def _operands(dtype, pad_x=8, pad_y=4, lead=0):
    g = torch.Generator().manual_seed(3)
    xv = torch.randn(M, N, generator=g).to(dtype)
    return xv, fr.framed(xv, ld=N + pad_x, lead=lead), fr.framed_out((M, N), dtype, "cpu", ld=N + pad_y, lead=lead)


def _all(x, y, xv, tol):
    fr.assert_close(y, 2.0 * xv.double() + 1.0, tol)
    fr.assert_all_written(y)
    fr.assert_frame_intact(y)
    fr.assert_untouched(x)


TOL = {torch.float16: 2e-3, torch.bfloat16: 1.6e-2, torch.float32: 1e-6, torch.float64: 1e-12}


@DTYPES
@pytest.mark.parametrize("lead", [0, 4])
def test_the_correct_standin_passes(dtype, lead):
    xv, x, y = _operands(dtype, lead=lead)
    assert x.shape == (M, N) and x.stride() == (N + 8, 1) and y.stride() == (N + 4, 1)
    assert x.storage_offset() == fr.GUARD_ROWS * (N + 8) + lead and x._frame.buf.numel() >= (2 * fr.GUARD_ROWS + M) * (N + 8)
    assert torch.equal(x, xv) and not torch.isfinite(y).any()
    _standin(x, y)
    _all(x, y, xv, TOL[dtype])


# (bug, the assertion that must fire, the location it must name)
WRONG = [("gap_store", "frame", f"(row 5, column {N})"),
         ("row_past_M", "frame", f"(row {M}, column 0)"),
         ("store_before", "frame", f"(row -1, column {N + 4 - 1})"),
         ("skip", "written", "(row 7, column 3)"),
         ("gap_read", "close", f"(row 2, column {N - 1})"),
         ("width_for_ldy", "frame", f"(row 0, column {N})"),           # row 1 lands in row 0's gap
         ("width_for_ldx", "close", "(row 1, column 0)"),                   # row 1 read from inside row 0's NaN gap
         ("input_store", "input", "(row 4, column 1)")]


@DTYPES
@pytest.mark.parametrize("bug,which,where", WRONG, ids=[w[0] for w in WRONG])
def test_every_wrong_standin_is_reported_where_it_went_wrong(bug, which, where, dtype):
    xv, x, y = _operands(dtype)
    _standin(x, y, bug)
    ref = 2.0 * xv.double() + 1.0
    checks = {"frame": lambda: fr.assert_frame_intact(y), "written": lambda: fr.assert_all_written(y),
              "close": lambda: fr.assert_close(y, ref, TOL[dtype]), "input": lambda: fr.assert_untouched(x)}
    with pytest.raises(AssertionError) as e:
        checks[which]()
    assert where in str(e.value), str(e.value)
    if which != "close" and bug != "width_for_ldy":      # one fault, one finding: the other checks stay quiet
        for k, c in checks.items():
            if k != which and not (bug == "skip" and k == "close"):
                c()


def test_width_for_the_input_stride_reads_the_poisoned_gap():
    """Row 1 read at offset N instead of ldx starts inside row 0's gap: NaN, at (row 1, column 0) -- no tolerance can absorb it."""
    xv, x, y = _operands(torch.float16)
    _standin(x, y, "width_for_ldx")
    assert not torch.isfinite(y[1, 0]) and torch.isfinite(y[0]).all()


def test_fill_patterns_are_nan_in_both_16_bit_types_and_distinct():
    for bits in (fr._IN[2], fr._OUT_INTERIOR[2], fr._OUT_FRAME[2]):
        i = torch.tensor([fr._signed(bits, 2)], dtype=torch.int16)
        assert torch.isnan(i.view(torch.float16)).all() and torch.isnan(i.view(torch.bfloat16)).all()
    assert torch.isfinite(torch.tensor([0x7e5a], dtype=torch.int16).view(torch.bfloat16)).all()      # why not just any fp16 NaN
    for size, ft in ((4, torch.float32), (8, torch.float64)):
        for tab in (fr._IN, fr._OUT_INTERIOR, fr._OUT_FRAME):
            assert torch.isnan(torch.tensor([tab[size]], dtype=fr._INT[size]).view(ft)).all()
    for size in (1, 2, 4, 8):
        assert fr._OUT_INTERIOR[size] != fr._OUT_FRAME[size]
    assert torch.isnan(torch.tensor([0x7f, 0xff], dtype=torch.uint8).view(torch.float8_e4m3fn).float()).all()


def test_batched_rows_bytes_fillers_and_vectors():
    t = torch.arange(3 * 5 * 8, dtype=torch.float32).view(3, 5, 8)
    v = fr.framed(t, ld=12)
    assert v.stride() == (5 * 12, 12, 1) and torch.equal(v, t)                      # [B][rows][ld]: batch stride rows * ld
    n = fr.framed(torch.zeros(2, 3, 4, 8), ld=16)
    assert n.stride() == (3 * 4 * 16, 4 * 16, 16, 1)                               # NHWC at a channel pitch
    big = fr.framed(t.to(torch.bfloat16), ld=16, fill=1.0e4)
    assert float(big._frame.buf[0]) == float(torch.tensor(1.0e4).to(torch.bfloat16)) and float(big._frame.buf[big._frame.start + 8]) > 9e3
    o = fr.framed_out((4, 16), torch.uint8, "cpu", ld=32)
    assert int(o[0, 0]) == 0xff and int(o._frame.buf[0]) == 0x7f
    o.fill_(1)
    fr.assert_all_written(o)
    fr.assert_frame_intact(o)
    o._frame.buf[o._frame.start + 16] = 0                                           # a byte store into the gap
    with pytest.raises(AssertionError, match=r"\(row 0, column 16\)"):
        fr.assert_frame_intact(o)
    b = fr.framed(torch.ones(10, dtype=torch.float64), ld=16, lead=2)
    assert b.shape == (10,) and b.storage_offset() == fr.GUARD_ROWS * 16 + 2
    with pytest.raises(ValueError):
        fr.framed(t, ld=4)


def test_policies_tight_is_plain_and_framed_verifies():
    t = fr.Tight()
    x = torch.ones(4, 8)
    assert t.inp("x", x) is x and t.out("o", (4, 8), torch.float32, "cpu").is_contiguous()
    assert t.out("own", (4, 8), torch.float32, "cpu", own=True) is None and t.done("own", x) is x and t.outs["own"] is x    # the wrapper's own allocation
    t.verify()
    f = fr.Framed(pad=8, pads={"o": 4}, leads={"o": 4})
    assert f.out("own", (4, 8), torch.float32, "cpu", own=True).stride(0) == 16 and f.done("own", f.outs["own"]) is f.outs["own"]
    f.outs["own"].fill_(0.0)
    xi, o = f.inp("x", x), f.out("o", (4, 8), torch.float16, "cpu")
    assert xi.stride(0) == 16 and o.stride(0) == 12 and o.storage_offset() % 8 == 4 and f.outs["o"] is o
    with pytest.raises(AssertionError, match="never written"):
        f.verify()
    o.copy_(xi)
    f.verify()
    xc, c0 = f.chan("xc", torch.ones(2, 3, 8))
    assert c0 == 8 and xc.shape == (2, 3, 32) and xc.stride() == (96, 32, 1) and torch.isnan(xc[..., :8]).all() and torch.isnan(xc[..., 16:]).all()
    assert torch.equal(xc[..., 8:16], torch.ones(2, 3, 8)) and t.chan("xc", x) == (x, 0)
    assert torch.isnan(f.poison(torch.zeros(3, dtype=torch.bfloat16))).all() and float(t.poison(torch.zeros(1))) == 0.0
    assert f.inp("w", x, contig=True).stride(0) == 8 and f.out("st", (5,), torch.float64, "cpu", contig=True, scratch=True).numel() == 5
    s = f.inout("s", torch.zeros(4, 8))
    s += 1
    f.verify()
    s._frame.buf[s._frame.start + 8] = 0.0
    with pytest.raises(AssertionError, match=r"s: .*\(row 0, column 8\)"):
        f.verify()
