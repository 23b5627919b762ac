"""Framed operands for the kernel checks: a tensor's values inside a larger flat buffer, at a row stride of the caller's choice, with a guard
band before and after and every element outside the logical ones holding a known bit pattern.  What a launch did to memory it does not own
is then a comparison of integers, and what it read from memory it should not look at shows in its result:

  framed(t, ld, lead, fill)   an INPUT: t's values, NaN (or `fill`) in the gap columns [width, ld) of every row and in both guard bands;
  framed_out(shape, ...)      an OUTPUT: the logical interior NaN (pattern A: an element nobody wrote is not finite), the frame NaN of a
                              second pattern (B: a store outside the extent changes it);
  assert_frame_intact(view)   the frame of an output (everything but the interior) bit for bit;
  assert_untouched(view)      an input: the whole buffer, interior included, bit for bit;
  assert_all_written(view)    no interior element of an output still holds pattern A.

Failures name the first changed element as (row, column) relative to the view: row < 0 lies before it, row >= rows after it, column >= width in
the gap of that row.  Tensors the ABI addresses as [B][rows][ld] get the batch stride rows * ld -- every leading dimension is folded into the
row index, no free 3-D stride.  Nothing here needs a GPU: tests/test_frames_cpu.py drives it with torch stand-ins that are wrong on purpose.

Tight / Framed are the allocation policies tests/kernel_checks.py takes its tensors from: one reference arithmetic, two memory layouts."""
import torch

GUARD_ROWS = 256                                         # one full tile of the largest GEMM tile, before and after
# NaN in fp16 AND in bf16 (0x7e5a, say, is NaN in fp16 but a finite bf16 number); e4m3 has one NaN magnitude, 0x7f / 0xff, and the kernels
# saturate: they produce neither byte
_IN = {1: 0x7f, 2: 0x7fc1, 4: 0x7fc00001, 8: 0x7ff8000000000001}
_OUT_INTERIOR = {1: 0xff, 2: 0x7fe3, 4: 0x7fc00002, 8: 0x7ff8000000000002}
_OUT_FRAME = {1: 0x7f, 2: 0x7fc5, 4: 0x7fc00003, 8: 0x7ff8000000000003}
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _signed(pattern, size):
    return pattern if size == 1 or pattern < 1 << (8 * size - 1) else pattern - (1 << (8 * size))


def _bits(fill, dtype):
    """fill: an int is a bit pattern, a float a value of `dtype` (the large finite filler of the attention checks)."""
    size = torch.empty((), dtype=dtype).element_size()
    if isinstance(fill, float):
        return int(torch.tensor([fill], dtype=dtype).view(_INT[size])[0])
    return _signed(fill, size)


def ints(t):
    """The same memory as integers of the element size (NaN payloads compare; -0.0 differs from 0.0)."""
    return t.view(_INT[t.element_size()])


class _Frame:
    def __init__(self, buf, start, shape, ld, interior_bits):
        self.buf, self.start, self.shape, self.ld = buf, start, tuple(shape), ld
        self.width = shape[-1]
        self.rows = 1
        for n in shape[:-1]:
            self.rows *= n
        self.interior_bits = interior_bits
        self.snapshot = ints(buf).clone()

    def where(self, offset):
        rel = offset - self.start
        return rel // self.ld, rel % self.ld

    def interior_mask(self):
        rel = torch.arange(self.buf.numel(), device=self.buf.device) - self.start
        return (rel >= 0) & (rel < self.rows * self.ld) & (rel % self.ld < self.width)


def _build(shape, dtype, device, ld, lead, frame_bits, interior_bits):
    shape = tuple(shape) if len(shape) > 1 else (1,) + tuple(shape)
    width = shape[-1]
    ld = width if ld is None else ld
    if ld < width or lead < 0:
        raise ValueError(f"framed: ld={ld} < width={width} or lead={lead} < 0")
    rows = 1
    for n in shape[:-1]:
        rows *= n
    size = torch.empty((), dtype=dtype).element_size()
    guard = GUARD_ROWS * ld
    start = guard + lead
    buf_i = torch.full((start + rows * ld + guard,), frame_bits, dtype=_INT[size], device=device)
    buf = buf_i.view(dtype)
    strides, s = [1], ld
    for n in reversed(shape[1:-1]):
        strides.insert(0, s)
        s *= n
    strides.insert(0, s)
    view = buf.as_strided(shape, strides, start)
    if interior_bits is not None:
        ints(view).fill_(interior_bits)
    return buf, view, start, shape, ld


def framed(t, ld=None, lead=0, fill=None):
    """An input: a view of t's shape and values at row stride `ld` (default: tight), starting `lead` elements after a guard band of GUARD_ROWS
    rows; gap columns and guard bands hold `fill` (default: NaN in every float type this size can be; an int is a bit pattern, a float a value).
    lead % (16 / element size) == 0 keeps the 16-byte alignment of the allocation.  A 1-D t is one row."""
    size = t.element_size()
    bits = _bits(_IN[size] if fill is None else fill, t.dtype)
    one_d = t.dim() == 1
    buf, view, start, shape, ld = _build(t.shape, t.dtype, t.device, ld, lead, bits, None)
    view.copy_(t.reshape(shape))
    fr = _Frame(buf, start, shape, ld, None)
    if one_d:
        view = view[0]
    view._frame = fr
    return view


def framed_out(shape, dtype, device, ld=None, lead=0):
    """An output: interior pre-filled with NaN pattern A, frame with NaN pattern B (uint8 = e4m3 bytes: 0xff inside, 0x7f around)."""
    size = torch.empty((), dtype=dtype).element_size()
    one_d = len(shape) == 1
    buf, view, start, shape, ld = _build(shape, dtype, device, ld, lead, _signed(_OUT_FRAME[size], size), _signed(_OUT_INTERIOR[size], size))
    fr = _Frame(buf, start, shape, ld, _signed(_OUT_INTERIOR[size], size))
    if one_d:
        view = view[0]
    view._frame = fr
    return view


def _first(fr, bad, what):
    off = int(torch.nonzero(bad.flatten())[0])
    row, col = fr.where(off)
    now, was = int(ints(fr.buf)[off]), int(fr.snapshot[off])
    mask = (1 << (8 * fr.buf.element_size())) - 1
    raise AssertionError(f"{what}: {int(bad.sum())} element(s) changed, the first at (row {row}, column {col}) of a [{fr.rows}][{fr.width}] view with "
                         f"ld {fr.ld}: bits {was & mask:#x} -> {now & mask:#x}")


def assert_frame_intact(view, what="frame"):
    """Guard bands and gap columns of `view` hold the bits they were given."""
    fr = view._frame
    bad = (ints(fr.buf) != fr.snapshot) & ~fr.interior_mask()
    if bool(bad.any()):
        _first(fr, bad, f"{what}: a store outside the logical extent")


def assert_untouched(view, what="input"):
    """The whole buffer of an input, its values included, holds the bits it was given."""
    fr = view._frame
    bad = ints(fr.buf) != fr.snapshot
    if bool(bad.any()):
        _first(fr, bad, f"{what}: an input buffer was written")


def assert_all_written(view, what="output"):
    """No interior element of an output made by framed_out still holds its pre-fill."""
    fr = view._frame
    bad = (ints(fr.buf) == fr.interior_bits) & fr.interior_mask()
    if bool(bad.any()):
        off = int(torch.nonzero(bad)[0])
        row, col = fr.where(off)
        raise AssertionError(f"{what}: {int(bad.sum())} element(s) never written, the first at (row {row}, column {col}) of a [{fr.rows}][{fr.width}] view")


def assert_close(view, ref, tol, what="output"):
    """max|x - ref| / max|ref| <= tol (the metric of tests/kernel_checks.py), and every element finite; names the worst (row, column)."""
    x, ref = view.double().reshape(-1, view.shape[-1]), ref.double().reshape(-1, view.shape[-1])
    fin = torch.isfinite(x)
    if not bool(fin.all()):
        off = int(torch.nonzero(~fin.flatten())[0])
        raise AssertionError(f"{what}: not finite at (row {off // x.shape[1]}, column {off % x.shape[1]})")
    d = (x - ref).abs()
    err = float(d.max() / ref.abs().max().clamp_min(1e-300))
    if not err <= tol:
        off = int(d.argmax())
        raise AssertionError(f"{what}: max-rel error {err:.3e} > {tol:.1e}, the worst at (row {off // x.shape[1]}, column {off % x.shape[1]})")
    return err


# ---------------------------------------------------------------------------------------------------------------- allocation policies
class Tight:
    """tests/kernel_checks.py as it always ran: inputs as they are, outputs torch.empty of the logical shape, zero wherever an operand is padded.
    `outs` keeps every output by name (the last launch's); `verify` has nothing to check."""
    k_pad = 0.0                                          # K rows nk..k_rows-1 (the header: masked)
    vt_pad = 0.0                                         # V^T positions of keys >= nk (the header: finite)
    framed = False

    def __init__(self):
        self.outs = {}

    def inp(self, name, t, contig=False, fill=None):
        return t

    def chan(self, name, x):
        """An NHWC activation a conv segment reads: (tensor, first channel read)."""
        return x, 0

    def poison(self, t):
        """What no launch may look at: left as it is here, NaN in a frame."""
        return t

    def out(self, name, shape, dtype, device, contig=False, init=None, scratch=False, own=False):
        """own: the op's wrapper allocates this output itself when given none -- here it is given none (that path stays exercised), and the
        check hands what the wrapper returned to done()."""
        if own:
            return None
        shape = tuple(shape)
        o = torch.empty(shape, dtype=dtype, device=device) if init is None else torch.full(shape, init, dtype=dtype, device=device)
        self.outs[name] = o
        return o

    def inout(self, name, t, contig=False):
        self.outs[name] = t
        return t

    def done(self, name, t):
        """What a wrapper returned for the output `name` (its own allocation, or the tensor out() gave it)."""
        self.outs[name] = t
        return t

    def verify(self):
        pass


class Framed(Tight):
    """Every tensor inside a frame.  pads[name] = extra elements of that tensor's row stride (default `pad`; a tensor the ABI takes
    contiguous gets none, only the guard bands), leads[name] = its start offset in elements (default 0: 16-byte aligned), fills[name] = the
    filler of an input (default NaN).  K rows the header calls masked hold NaN, V^T positions it asks to be finite hold 1.0e4: a key whose
    weight is not exactly 0 shows in the result.  verify(): every output's frame intact and every element of it written, every scratch and
    in-place tensor's frame intact, every input buffer bit-equal to what it was given."""
    k_pad = float("nan")
    vt_pad = 1.0e4
    framed = True

    def __init__(self, pad=8, pads=None, leads=None, fills=None, coff=8, ctail=16):
        super().__init__()
        self.pad, self.pads, self.leads, self.fills, self.coff, self.ctail = pad, dict(pads or {}), dict(leads or {}), dict(fills or {}), coff, ctail
        self.inputs, self.outputs, self.frames_only = [], [], []

    def _ld(self, name, width, contig):
        return width + self.pads.get(name, 0 if contig else self.pad)

    def inp(self, name, t, contig=False, fill=None):
        v = framed(t, self._ld(name, t.shape[-1], contig), self.leads.get(name, 0), self.fills.get(name, fill))
        self.inputs.append((name, v))
        return v

    def chan(self, name, x):
        """x's channels at [coff, coff + C) of a pixel `coff + C + ctail` channels wide, the channels not read NaN: the skip-concat and
        [hi | lo] pattern of the product (coff > 0, coff + len < pitch)."""
        C = x.shape[-1]
        wide = torch.empty(x.shape[:-1] + (self.coff + C + self.ctail,), dtype=x.dtype, device=x.device)
        ints(wide).fill_(_bits(_IN[x.element_size()], x.dtype))
        wide[..., self.coff:self.coff + C] = x
        return self.inp(name, wide, contig=True), self.coff

    def poison(self, t):
        ints(t).fill_(_bits(_IN[t.element_size()], t.dtype))
        return t

    def out(self, name, shape, dtype, device, contig=False, init=None, scratch=False, own=False):
        v = framed_out(tuple(shape), dtype, device, self._ld(name, shape[-1], contig), self.leads.get(name, 0))
        (self.frames_only if scratch else self.outputs).append((name, v))
        self.outs[name] = v
        return v

    def inout(self, name, t, contig=False):
        """A tensor the op updates in place: values in, frame of the INPUT kind (NaN that a read of the gap would pick up), frame checked after."""
        v = framed(t, self._ld(name, t.shape[-1], contig), self.leads.get(name, 0))
        self.frames_only.append((name, v))
        self.outs[name] = v
        return v

    def verify(self):
        if any(v.is_cuda for _, v in self.outputs + self.frames_only + self.inputs):
            torch.cuda.synchronize()
        for name, v in self.outputs:
            assert_frame_intact(v, name)
            assert_all_written(v, name)
        for name, v in self.frames_only:
            assert_frame_intact(v, name)
        for name, v in self.inputs:
            assert_untouched(v, name)
