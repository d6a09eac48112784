"""Bit-exact tests of the matrix-core convs: operands on a lattice where every fp32 partial sum is exact (tests/lattice_ref.py).

A tolerance relative to the output's maximum leaves a factor of ~20 in which a three-term kernel can be wrong unseen (a lo*hi term missing
in one k-step, a lo half from the neighbouring lane, a weight record with the lo of the wrong cout, lo*lo added).  Here the kernel's
result is ONE bit pattern whatever order the MFMAs accumulate in -- the exact value of
    MDTILE_PRECISION_BF16X3:          sum (hh + hl + lh) + bias + residual     (lo*lo is not in it)
    MDTILE_PRECISION_BF16:            sum hh + bias + residual
    MDTILE_PRECISION_F32 / exact=True sum a b + bias + residual                (integer operands, and conv_in's K <= 36)
-- and every assertion is torch.equal against lattice_ref.expected_conv (fp64).  tests/test_lattice_host.py proves the instrument: the
orders agree, the wrong kernels above change bits.  Two operand classes: the lattice (hi in +-{1 .. 1.75}, lo = j 2^-10; hi sets chosen
from K, the precondition asserted on the actual tensors) and small integers (lo = 0: every mode must return the same bits).
Shapes: the smallest that reach every block variant and a ragged edge (lattice_ref's case tables), not the workload's.
A mismatch message gives the count of differing elements, the first index and the difference in units of the grain g.
The fp16 kernels of MDTILE_PRECISION_F16 have a module of their own, tests/test_gpu_f16_exact.py: they form the whole product, lo*lo
included, so there the fine bits go to one operand only and sub-ulp bits probe the conversion (tests/f16_exact_ref.py).  The fused GroupNorm + SiLU input, the activated record
output and the statistics epilogues have a module of their own, tests/test_gpu_gn_exact.py: SiLU is the identity on a saturated set, and
the statistics are exact on small integers.  The attention has a module of its own, tests/test_gpu_attn_exact.py: its softmax is exact where the live keys
of a query tie and every other key lies 160 below in the log2 domain.  Every test leaves the default precision mode behind."""
import functools

import pytest
import torch

import lattice_ref as lr

pytestmark = pytest.mark.gpu

TERMS_OF_MODE = {"bf16x3": "hh+hl+lh", "bf16": "hh", "f32": "full", "exact": "full"}


@pytest.fixture(autouse=True)
def _default_mode_after(plugin):
    E = plugin.engine
    assert E.get_precision() == E.PRECISION_BF16X3
    yield
    mode = E.get_precision()
    E.set_precision(E.PRECISION_BF16X3)
    assert mode == E.PRECISION_BF16X3, "a test leaked its precision mode"


def _mode(E, mode):
    """the precision context of a mode name ("exact" is the default mode with exact=True on the call)"""
    return E.precision({"bf16x3": E.PRECISION_BF16X3, "bf16": E.PRECISION_BF16, "f32": E.PRECISION_F32, "exact": E.PRECISION_BF16X3}[mode])


def _assert_equal(got, want, g, what):
    got = got.cpu()
    assert torch.equal(got, want), f"{what}: {lr.mismatch_report(got, want, g)}"


class Ops:
    """operands of one case in one class, on the CPU; the precondition is asserted before any value is expected"""

    def __init__(self, cls, terms_class, B, cin, cout, hin, win, hout, wout, res, k, up, stride, seed):
        K = k * k * cin
        self.k, self.up, self.stride, self.cls = k, up, stride, cls
        if cls == "lattice":
            make = lambda shape, role: lr.lattice_operands(shape, K, seed, role, terms_class)      # noqa: E731
            self.g = lr.lattice_plan(K, terms_class).g
        else:
            make = lambda shape, role: lr.integer_operands(shape, seed, role)      # noqa: E731
            self.g = 1.0
        self.x = make((B, cin, hin, win), "x")
        self.w = make((cout, cin, k, k), "w_up" if up else "w")
        self.bias = make((cout,), "bias")
        self.res = make((B, cout, hout, wout), "residual") if res else None
        # integers: lo = 0, so one check with every product in it covers all modes
        self.ratio = lr.assert_exact_in_fp32(self.x, self.w, self.bias, self.res, self.g, terms=terms_class if cls == "lattice" else "full",
                                             stride=stride, up=up, k=k)
        self._want = {}

    def want(self, terms):
        if terms not in self._want:
            self._want[terms] = lr.expected_conv(self.x, self.w, self.bias, self.res, terms=terms, stride=self.stride, up=self.up, k=self.k)
        return self._want[terms]


@functools.lru_cache(maxsize=None)
def _ops(cls, terms_class, case, k, up=False, stride=1):
    """case = (B, cin, cout, H, W, residual) with H, W the OUTPUT size (stride 2: the INPUT size).  Computed once, shared, never changed."""
    B, cin, cout, H, W, res = case
    hin, win = (H // 2, W // 2) if up else (H, W)
    hout, wout = ((H - 2) // 2 + 1, (W - 2) // 2 + 1) if stride == 2 else (H, W)
    ops = Ops(cls, terms_class, B, cin, cout, hin, win, hout, wout, res, k, up, stride, seed=cin + 3 * cout + H)
    print(f"precondition {cls} {case} k={k} up={up} stride={stride}: sum|terms| / (2^24 g) = {ops.ratio:.4f}")
    if cls == "lattice" and terms_class != "full":
        # the lo terms are in nearly every expected value: a kernel that lost them could not pass by accident
        assert (ops.want("hh+hl+lh") != ops.want("hh")).float().mean() > 0.9
    return ops


def _class_modes(split_kernel, lattice_ok=True):
    """(class, mode) pairs a kernel allows: the lattice where no lo*lo is formed (three- and one-term modes of a split kernel) or where its
    own plan fits (conv_in); integers in every mode"""
    out = []
    if split_kernel:
        out += [("lattice", "bf16x3"), ("lattice", "bf16")]
    elif lattice_ok:
        out += [("lattice", "bf16x3"), ("lattice", "bf16"), ("lattice", "f32")]
    return out + [("integer", m) for m in ("bf16x3", "bf16", "f32", "exact")]


def _params(cases, **kw):
    return [pytest.param(c, cls, mode, id=f"{'x'.join(str(v) for v in c[:5])}-{cls}-{mode}") for c in cases for cls, mode in _class_modes(**kw)]


def _handover(plugin, cuda, case, cls, mode, *, k, up=False, split_kernel=True, token_major=False):
    """E.PackedConv(w, b)(x, ...) of one case against its exact value.  split_kernel: a matrix-core split-bf16 kernel takes the shape (the
    mode decides the terms); otherwise an fp32 kernel runs in every mode and every product is whole."""
    E = plugin.engine
    terms = TERMS_OF_MODE[mode] if split_kernel else "full"
    ops = _ops(cls, "hh+hl+lh" if split_kernel else "full", case, k, up)
    pc = E.PackedConv(ops.w.to(cuda), ops.bias.to(cuda))
    with _mode(E, mode):
        y = pc(ops.x.to(cuda), residual=None if ops.res is None else ops.res.to(cuda), upsample2x=up, token_major=token_major, exact=mode == "exact")
        torch.cuda.synchronize()
    want = ops.want(terms)
    if token_major:
        want = want.flatten(2).transpose(1, 2).contiguous()
    _assert_equal(y, want, ops.g, f"{case} {cls} {mode}")


# ---- hand-over convs (fp32 in, fp32 out) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,cls,mode", _params(lr.HANDOVER_3X3, split_kernel=True))
def test_lattice_conv3x3_handover(plugin, cuda, case, cls, mode):
    _handover(plugin, cuda, case, cls, mode, k=3)


@pytest.mark.parametrize("case,cls,mode", _params([lr.HANDOVER_NARROW], split_kernel=False, lattice_ok=False))
def test_lattice_conv3x3_handover_narrow_output(plugin, cuda, case, cls, mode):
    """cout < 32 outside the record path: the exact-fp32 kernel in every mode (K = 1152 fits no lo*lo lattice: integers)."""
    _handover(plugin, cuda, case, cls, mode, k=3, split_kernel=False)


@pytest.mark.parametrize("case,cls,mode", _params(lr.HANDOVER_UP, split_kernel=True))
def test_lattice_upconv_handover(plugin, cuda, case, cls, mode):
    """Sub-pixel upsample: the merged weights are what is split (lattice_ref: role "w_up")."""
    _handover(plugin, cuda, case, cls, mode, k=3, up=True)


@pytest.mark.parametrize("case,cls,mode", [pytest.param(c, cls, mode, id=f"{'x'.join(str(v) for v in c)}-{cls}-{mode}") for c in lr.DOWN2
                                           for cls, mode in [("lattice", "bf16x3"), ("lattice", "bf16"), ("integer", "bf16x3"), ("integer", "bf16"), ("integer", "f32")]])
def test_lattice_downsample_stride2(plugin, cuda, case, cls, mode):
    """ldm Downsample through the engine's down-conv call (mdtile_conv2d_down2): pad right 1, bottom 1, stride 2; odd and even inputs."""
    E = plugin.engine
    B, cin, cout, Hin, Win = case
    ops = _ops(cls, "hh+hl+lh", (B, cin, cout, Hin, Win, False), 3, False, 2)
    pc = E.PackedConv(ops.w.to(cuda), ops.bias.to(cuda))
    with _mode(E, mode):
        y = pc.down2(ops.x.to(cuda))
        torch.cuda.synchronize()
    _assert_equal(y, ops.want(TERMS_OF_MODE[mode]), ops.g, f"down2 {case} {cls} {mode}")


@pytest.mark.parametrize("case,cls,mode", _params(lr.CONV_IN, split_kernel=False))
def test_lattice_conv_in_few_cin(plugin, cuda, case, cls, mode):
    """conv_in (cin 3 / 4): fp32 FMAs in every mode, K <= 36 -- exact on both classes (the lattice plan of "full": hi = +-1, lo = +-2^-9 or 0)."""
    _handover(plugin, cuda, case, cls, mode, k=3, split_kernel=False)


@pytest.mark.parametrize("case,cls,mode", _params(lr.CONV1X1, split_kernel=True))
def test_lattice_conv1x1(plugin, cuda, case, cls, mode):
    _handover(plugin, cuda, case, cls, mode, k=1)


@pytest.mark.parametrize("case,cls,mode", _params([lr.CONV1X1_TOKEN_MAJOR], split_kernel=False, lattice_ok=False))
def test_lattice_conv1x1_token_major(plugin, cuda, case, cls, mode):
    """[B, H W, cout] output (the attention's V operand): the exact-fp32 kernel in every mode."""
    _handover(plugin, cuda, case, cls, mode, k=1, split_kernel=False, token_major=True)


@pytest.mark.parametrize("case,cls,mode", _params(lr.CONV1X1_STREAM, split_kernel=True))
def test_lattice_conv1x1_streaming(plugin, cuda, case, cls, mode):
    _handover(plugin, cuda, case, cls, mode, k=1)


# ---- record convs ------------------------------------------------------------------------------------------------------------------------
def _border_is_zero(rec):
    r = rec.records()
    return not (r[:, :, :, 0].any() or r[:, :, :, -1].any() or r[:, :, :, :, 0].any() or r[:, :, :, :, -1].any())


def _record_of(E, cuda, ops):
    """the raw record image of x; it holds hi and lo exactly, inside a ring of zeros"""
    xrec = E.rec_from_f32(ops.x.to(cuda))
    _assert_equal(xrec.to_f32(), ops.x, ops.g, "record image of x")
    assert _border_is_zero(xrec), "the border ring of the record image is not zero"
    return xrec


REC_MODES = [("lattice", "bf16x3"), ("lattice", "bf16"), ("integer", "bf16x3"), ("integer", "bf16")]


@pytest.mark.parametrize("family", ["one_block", "two_blocks"])
@pytest.mark.parametrize("case,up,cls,mode", [pytest.param(c, up, cls, mode, id=f"{'x'.join(str(v) for v in c[:5])}{'-up' if up else ''}-{cls}-{mode}")
                                              for c, up in [(c, False) for c in lr.REC_DIRECT] + [(lr.REC_UP, True)] for cls, mode in REC_MODES])
def test_lattice_conv_rec(plugin, cuda, case, up, cls, mode, family):
    """Record 3x3 and sub-pixel record conv, both kernel families: the fp32 output, the raw record output (hi + lo of the same values), and the
    two written by one launch."""
    E = plugin.engine
    ops = _ops(cls, "hh+hl+lh", case, 3, up)
    pc = E.PackedConv(ops.w.to(cuda), ops.bias.to(cuda))
    assert pc.takes_rec(up)
    xrec = _record_of(E, cuda, ops)
    rr = None if ops.res is None else ops.res.to(cuda)
    fam = E.CONV_REC_ONE_BLOCK if family == "one_block" else E.CONV_REC_TWO_BLOCKS
    with _mode(E, mode):
        y, yr = pc.call_rec(xrec, residual=rr, upsample2x=up, want_f32=True, want_rec=True, family=fam)
        y1, none = pc.call_rec(xrec, residual=rr, upsample2x=up, want_f32=True, family=fam)
        none2, yr2 = pc.call_rec(xrec, residual=rr, upsample2x=up, want_f32=False, want_rec=True, family=fam)
        torch.cuda.synchronize()
    assert none is None and none2 is None
    want = ops.want(TERMS_OF_MODE[mode])
    what = f"{case} up={up} {cls} {mode} {family}"
    _assert_equal(y, want, ops.g, f"{what}: fp32 output (with a record output)")
    _assert_equal(y1, want, ops.g, f"{what}: fp32 output alone")
    _assert_equal(yr.to_f32(), lr.expected_split(y.cpu()), ops.g, f"{what}: the record output against the fp32 output of the same launch")
    _assert_equal(yr.to_f32(), lr.expected_split(want), ops.g, f"{what}: record output (with an fp32 output)")
    _assert_equal(yr2.to_f32(), lr.expected_split(want), ops.g, f"{what}: record output alone")
    assert _border_is_zero(yr) and _border_is_zero(yr2), f"{what}: the border ring of the record output is not zero"


@pytest.mark.parametrize("cls,mode", REC_MODES)
def test_lattice_conv_rec_narrow_output(plugin, cuda, cls, mode):
    """conv_out on records: one 32-cout tile, fp32 output for the real couts only."""
    E = plugin.engine
    ops = _ops(cls, "hh+hl+lh", lr.REC_NARROW, 3)
    pc = E.PackedConv(ops.w.to(cuda), ops.bias.to(cuda))
    assert pc.takes_rec()
    xrec = _record_of(E, cuda, ops)
    with _mode(E, mode):
        y, yr = pc.call_rec(xrec, want_f32=True)
        torch.cuda.synchronize()
    assert yr is None
    _assert_equal(y, ops.want(TERMS_OF_MODE[mode]), ops.g, f"{lr.REC_NARROW} {cls} {mode}")


@pytest.mark.parametrize("family", ["one_block", "two_blocks"])
@pytest.mark.parametrize("cls,mode", REC_MODES)
def test_lattice_upconv_rec_window(plugin, cuda, cls, mode, family):
    """mdtile_upconv2d_rec_window, two images with different origins.  A window edge inside the image reads the image's real neighbours
    (tests/test_gpu_rec.py::test_upconv_window_equals_the_same_pixels_of_the_whole_image_call): every window pixel equals the same pixel
    of the whole image's exact value.  Against the exact value of the CROPPED input, which has zeros there, the outermost ring of output
    pixels is comparable only along edges where the window touches the image border; everything inside the ring always is."""
    E = plugin.engine
    B, cin, cout, Hin, Win, h, w, y0s, x0s = lr.REC_WINDOW
    ops = _ops(cls, "hh+hl+lh", (B, cin, cout, 2 * Hin, 2 * Win, False), 3, True)
    terms = TERMS_OF_MODE[mode]
    pc = E.PackedConv(ops.w.to(cuda), ops.bias.to(cuda))
    xrec = _record_of(E, cuda, ops)
    fam = E.CONV_REC_ONE_BLOCK if family == "one_block" else E.CONV_REC_TWO_BLOCKS
    with _mode(E, mode):
        y, yr = pc.call_rec(xrec, upsample2x=True, want_f32=True, want_rec=True, window=(list(y0s), list(x0s), h, w), family=fam)
        torch.cuda.synchronize()
    y, yr32 = y.cpu(), yr.to_f32().cpu()
    whole = ops.want(terms)
    for b in range(B):
        y0, x0 = y0s[b], x0s[b]
        what = f"window image {b} at ({y0}, {x0}) {cls} {mode} {family}"
        want = whole[b:b + 1, :, 2 * y0:2 * (y0 + h), 2 * x0:2 * (x0 + w)]
        _assert_equal(y[b:b + 1], want, ops.g, f"{what}: against the whole image's value")
        _assert_equal(yr32[b:b + 1], lr.expected_split(want), ops.g, f"{what}: record output")
        crop = lr.expected_conv(ops.x[b:b + 1, :, y0:y0 + h, x0:x0 + w], ops.w, ops.bias, None, terms=terms, up=True, k=3)
        top, left = (0 if y0 == 0 else 1), (0 if x0 == 0 else 1)
        bottom, right = 2 * h - (0 if y0 + h == Hin else 1), 2 * w - (0 if x0 + w == Win else 1)
        _assert_equal(y[b:b + 1, :, top:bottom, left:right], crop[:, :, top:bottom, left:right], ops.g, f"{what}: against the cropped input's value")
    assert _border_is_zero(yr)


# ---- cross-mode ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["conv3x3", "conv1x1", "record"])
def test_integer_operands_give_the_same_bits_in_every_mode(plugin, cuda, kind):
    """lo = 0 and every sum is an integer below 2^24: BF16X3, BF16 and F32 must return identical tensors.  The record kernels do not exist
    in MDTILE_PRECISION_F32 (the engine runs the hand-over kernel there): the record conv's two modes are compared with that."""
    E = plugin.engine
    case, k = {"conv3x3": (lr.HANDOVER_3X3[0], 3), "conv1x1": (lr.CONV1X1[0], 1), "record": (lr.REC_DIRECT[1], 3)}[kind]
    ops = _ops("integer", "hh+hl+lh", case, k)
    pc = E.PackedConv(ops.w.to(cuda), ops.bias.to(cuda))
    x, rr = ops.x.to(cuda), ops.res.to(cuda)
    out = {}
    for mode in ("bf16x3", "bf16", "f32"):
        with _mode(E, mode):
            if kind == "record" and mode != "f32":
                out[mode] = pc.call_rec(E.rec_from_f32(x), residual=rr, want_f32=True)[0]
            else:
                out[mode] = pc(x, residual=rr)
            torch.cuda.synchronize()
    _assert_equal(out["bf16"], out["bf16x3"].cpu(), 1.0, f"{kind}: BF16 against BF16X3")
    _assert_equal(out["f32"], out["bf16x3"].cpu(), 1.0, f"{kind}: F32 against BF16X3")
    _assert_equal(out["bf16x3"], ops.want("full"), 1.0, f"{kind}: against the integer value")


# ---- tanh (the decoder's last op, behind conv_out) ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 3 * 7 * 11 * 13])
def test_tanh_vs_torch_fp64(plugin, cuda, n):
    """mdtile_tanh against torch.tanh in fp64 over +-12 (saturation on both sides), sizes around the 4-wide vector path and its tail;
    1e-6 absolute, the bound of mdtile_silu in test_gn_pool_silu_add.  Also from a pointer that is not 16-byte aligned (scalar path)."""
    E = plugin.engine
    x = torch.linspace(-12.0, 12.0, n) if n > 1 else torch.tensor([0.75])
    if n >= 4:
        x[n // 2] = 0.0
    want = torch.tanh(x.double())
    got = E.tanh(x.to(cuda)).cpu()
    err = (got.double() - want).abs().max().item()
    print(f"tanh n={n}: max abs err {err:.3e}")
    assert err <= 1e-6
    assert (got.abs() <= 1.0).all()
    buf = torch.zeros(n + 1, device=cuda)
    buf[1:] = x.to(cuda)
    got2 = E.tanh(buf[1:]).cpu()
    assert torch.equal(got2, got), "the scalar path (unaligned pointer) differs from the vector path"
