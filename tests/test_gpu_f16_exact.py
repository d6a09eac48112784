"""Bit-exact tests of the fp16 operand mode, MDTILE_PRECISION_F16 (tests/f16_exact_ref.py): the conversion, the fp16 record forms and
every conv kernel that multiplies fp16 operands.

The contract (csrc/f16_convert.h): operands are h(v) = fp16_rn(clamp(v, +-65504)), products are exact, the MFMA adds them in fp32.  On the
operand classes of f16_exact_ref (fine bits on ONE operand, sub-ulp bits with ties on both; small integers; subnormal weights) every partial
sum in every order is an fp32 number, so the kernel's result is ONE bit pattern and every assertion is torch.equal against an fp64
evaluation on the ROUNDED operands -- nothing is read back from the library to form an expected value.  The expected conv differs from
the three-term and the one-term bf16 value of the same inputs, and from a truncating conversion, in over 99 % of the elements: equality
proves that the fp16 kernel ran, that it rounded to nearest even and that every product reached the right accumulator.  A mismatch message
names the case, the count of differing elements, the first index and the difference in grains.  There is no tolerance in this module.
tests/test_f16_exact_host.py proves the instrument.

The first tests probe what the rest supposes about the hardware: an identity conv returns fp16 numbers unchanged, and the fp32 accumulation
of v_mfma_f32_32x32x16_f16 keeps every multiple of g below 2^24 g (a sum that climbs to 0.894 of 2^24 g in steps that include single grains).

Kernels reached (by name): k_rec_from_f32_f16, k_rec_to_f32_f16; k_conv3x3_rec_f16<2, 2, 4>, k_conv3x3_rec_f16s<2, 2, 4> and <1, 1, 2>
(conv_out), k_conv3x3_rec_f16_st<2, 2, 4>; k_conv3x3_rec2_f16, k_conv3x3_rec2_f16s; k_conv3x3_f16<4, true>, <2, true> and
<4, true, 1, true> (statistics) with the weight plane of k_conv_pack_f16; k_upconv_rec_o16 and k_upconv_rec2_o16, whole image and window.
Left to other modules: the attention and the 1x1 convs in mode 5 are mode 2's arithmetic (tests/test_gpu_attn_exact.py, the conv lattice
module; test_attn_proj_flag_only_matters_in_mode_5 ties the routes together); end to end, range safety and stability stay in
tests/test_gpu_precision_f16.py.  Every test leaves the default precision mode behind."""
import pytest
import torch

import f16_exact_ref as fx
import gn_exact_ref as gx
import lattice_ref as lr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _default_mode_after(plugin):
    E = plugin.engine
    assert E.get_precision() == E.PRECISION_BF16X3
    yield
    mode = E.get_precision()
    E.set_precision(E.PRECISION_BF16X3)
    assert mode == E.PRECISION_BF16X3, "a test leaked its precision mode"


def _m5(E):
    return E.precision(E.PRECISION_F16)


def _assert_equal(got, want, g, what):
    got = got.cpu()
    assert torch.equal(got, want), f"{what}: {lr.mismatch_report(got, want, g)}"


def _dev(t, cuda):
    return None if t is None else t.to(cuda)


def _fam(E, family):
    return E.CONV_REC_ONE_BLOCK if family == "one_block" else E.CONV_REC_TWO_BLOCKS


def _ident(s):
    return "x".join(str(int(v)) for v in s[:5])


def _hi_border_is_zero(rec):
    """the border ring of the hi half (the fp16 form does not write the lo half)"""
    r = rec.records()[:, 0]
    return not (r[:, :, 0].any() or r[:, :, -1].any() or r[:, :, :, 0].any() or r[:, :, :, -1].any())


def _border_is_zero(rec):
    r = rec.records()
    return not (r[:, :, :, 0].any() or r[:, :, :, -1].any() or r[:, :, :, :, 0].any() or r[:, :, :, :, -1].any())


def _f16_record(E, cuda, c, what):
    """(inside mode 5) the activated fp16 record of a case: it must read back as h(act), inside a ring of zeros"""
    rec = E.rec_from_f32(c.x.to(cuda), c.co.coef.to(cuda))
    assert rec.fmt == E.REC_F16
    _assert_equal(rec.to_f32(), c.h_act, c.scale * 2.0 ** -10, f"{what}: fp16 record of the activation")
    assert _hi_border_is_zero(rec), f"{what}: the border ring of the input record is not zero"
    return rec


def _conv(E, cuda, c):
    return E.PackedConv(c.w.to(cuda), _dev(c.bias, cuda))


# ---- 1. probes --------------------------------------------------------------------------------------------------------------------------------
def _probe_tensor(C, H, W):
    vals = torch.tensor(gx.PROBE_VALUES)
    idx = (torch.arange(C).view(C, 1, 1) + torch.arange(H).view(1, H, 1) * W + torch.arange(W).view(1, 1, W)) % len(vals)
    x = vals[idx].view(1, C, H, W).contiguous()
    gx.assert_saturated(x)
    assert torch.equal(fx.h(x), x)
    return x


@pytest.mark.parametrize("route", ["record_one_block", "record_two_blocks", "handover"])
def test_probe_identity_conv_returns_fp16_numbers_unchanged(plugin, cuda, route):
    """gn_exact_ref.PROBE_VALUES are fp16 numbers: in mode 5 the identity conv returns them as they are, through the record kernels of both
    families (fp32 output and activated fp16 record output) and through the hand-over kernel."""
    E = plugin.engine
    C, H, W = 128, 8, 12
    x = _probe_tensor(C, H, W)
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    pc = E.PackedConv(w.to(cuda), None)
    unit = gx.unit_coef(1, C).to(cuda)
    with _m5(E):
        if route == "handover":
            assert pc.fuses_pre_gn()
            got = pc(x.to(cuda), pre_gn=unit)
        else:
            rec = E.rec_from_f32(x.to(cuda), unit)
            assert rec.fmt == E.REC_F16 and _hi_border_is_zero(rec)
            _assert_equal(rec.to_f32(), x, 2.0 ** -5, "fp16 record of the probe values")
            got, yr = pc.call_rec(rec, want_f32=True, want_rec=True, rec_coef=unit, family=_fam(E, route[7:]))
            assert yr.fmt == E.REC_F16 and _hi_border_is_zero(yr)
            _assert_equal(yr.to_f32(), x, 2.0 ** -5, f"{route}: activated fp16 record output")
        torch.cuda.synchronize()
    _assert_equal(got, x, 2.0 ** -5, route)


@pytest.mark.parametrize("route", ["record_one_block", "record_two_blocks", "handover"])
def test_probe_fp16_mfma_accumulation_keeps_every_grain(plugin, cuda, route):
    """The supposition everything below rests on: v_mfma_f32_32x32x16_f16 accumulates in fp32 without losing a multiple of g below 2^24 g.
    f16_exact_ref.accumulation_probe: all products positive, the sum climbs to 0.894 of 2^24 g, steps of 1, 2 and 3 grains among steps of
    ~13900; every operand is an fp16 number already, so nothing but the accumulation is probed.  Found on an MI355X: exact (this test)."""
    E = plugin.engine
    p = fx.accumulation_probe()
    pc = E.PackedConv(p.w.to(cuda), None)
    with _m5(E):
        if route == "handover":
            got = pc(p.x.to(cuda), pre_gn=p.co.coef.to(cuda))
        else:
            rec = E.rec_from_f32(p.x.to(cuda), p.co.coef.to(cuda))
            _assert_equal(rec.to_f32(), p.act, 2.0 ** -5, "fp16 record of the probe activation")
            got = pc.call_rec(rec, want_f32=True, family=_fam(E, route[7:]))[0]
        torch.cuda.synchronize()
    report = lr.mismatch_report(got, p.want, p.g)
    print(f"fp16 MFMA accumulation probe ({route}): largest sum {p.ratio:.3f} of 2^24 g: {report}")
    assert torch.equal(got.cpu(), p.want), f"accumulation probe {route}: {report}"


# ---- 2. producers -----------------------------------------------------------------------------------------------------------------------------
def _producer(E, cuda, x, coef, want, what):
    xd, cd = x.to(cuda), coef.to(cuda)
    base = E.rec_from_f32(xd)
    assert E.rec_from_f32(xd, cd).fmt == E.REC_BF16X2
    with _m5(E):
        rec = E.rec_from_f32(xd, cd)
        raw = E.rec_from_f32(xd)
        got = rec.to_f32()
        torch.cuda.synchronize()
    assert rec.fmt == E.REC_F16 and raw.fmt == E.REC_BF16X2
    assert bool(torch.isfinite(got).all()), f"{what}: Inf / NaN in an fp16 record"
    _assert_equal(got, want, 2.0 ** -10, what)
    assert _hi_border_is_zero(rec), f"{what}: the border ring of the hi half is not zero"
    assert torch.equal(raw.records(), base.records()), f"{what}: a raw record written in mode 5 differs from the default mode's"
    assert torch.equal(raw.to_f32(), base.to_f32())


def test_fp16_record_of_the_conversion_table(plugin, cuda):
    """rec_from_f32(x, coef) in mode 5 on f16_exact_ref.CONVERSION_TABLE: exact fp16 values, quarter ulps, ties with an even and an odd
    neighbour, ulps of 2 and more, 65504 ... 3e38 (all of which read back as exactly 65504) and 0.  fmaf(x, a, s) is the target exactly and
    SiLU the identity on it, so the one rounding is the conversion."""
    c = fx.conversion_case()
    assert bool((c.want[c.t >= 65504.0] == 65504.0).all()) and int((c.t > 65504.0).sum()) > 0
    _producer(plugin.engine, cuda, c.x, c.coef, c.want, "conversion table")


@pytest.mark.parametrize("shape", gx.REC_FROM_SHAPES, ids=_ident)
def test_fp16_record_of_fine_activations(plugin, cuda, shape):
    """32 (|lattice x| + r 2^-12): 80 % of the values change under h, 40 % are ties"""
    c = fx.rec_from_case(shape)
    _producer(plugin.engine, cuda, c.x, c.co.coef, c.want, f"rec_from_f32(x, coef) {shape}")


# ---- 3. record convs (and 7: their activated fp16 record output) ------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["one_block", "two_blocks"])
@pytest.mark.parametrize("cls", fx.CLASSES)
@pytest.mark.parametrize("case", fx.REC_CASES, ids=_ident)
def test_record_conv_f16(plugin, cuda, case, cls, family):
    """k_conv3x3_rec_f16s (fp32 output alone; with a raw split record output), k_conv3x3_rec_f16 (with an activated fp16 record output) and
    their two-blocks-per-CU twins: one fp32 tensor in all calls, the exact value; the raw record is split(y); the fp16 record is h(a y + s)
    (f16_exact_ref.record_output: more than half of the values change under h, ties occur) inside a ring of zeros."""
    E = plugin.engine
    c = fx.conv_case(case, cls)
    what = f"record conv {case} {cls} {family}"
    pc = _conv(E, cuda, c)
    assert pc.takes_rec()
    r, fam = _dev(c.res, cuda), _fam(E, family)
    B, cout = case[0], case[2]
    ycoef = (c.out.coef if c.out is not None else torch.stack([torch.ones(B, cout), torch.full((B, cout), 64.0)], dim=1).contiguous()).to(cuda)
    with _m5(E):
        xrec = _f16_record(E, cuda, c, what)
        y, none = pc.call_rec(xrec, residual=r, want_f32=True, family=fam)
        y2, yrec = pc.call_rec(xrec, residual=r, want_f32=True, want_rec=True, rec_coef=ycoef, family=fam)
        y3, yraw = pc.call_rec(xrec, residual=r, want_f32=True, want_rec=True, family=fam)
        none2, yraw2 = pc.call_rec(xrec, residual=r, want_f32=False, want_rec=True, family=fam)
        _, yrec2 = pc.call_rec(xrec, residual=r, want_f32=False, want_rec=True, rec_coef=ycoef, family=fam)
        torch.cuda.synchronize()
    assert none is None and none2 is None
    _assert_equal(y, c.want, c.g, f"{what}: fp32 output alone")
    _assert_equal(y2, c.want, c.g, f"{what}: fp32 output beside an fp16 record output")
    _assert_equal(y3, c.want, c.g, f"{what}: fp32 output beside a raw record output")
    assert torch.equal(y, y2) and torch.equal(y, y3)
    assert yrec.fmt == E.REC_F16 and yrec2.fmt == E.REC_F16 and yraw.fmt == E.REC_BF16X2 and yraw2.fmt == E.REC_BF16X2
    split = lr.expected_split(c.want)
    _assert_equal(yraw.to_f32(), split, c.g, f"{what}: raw split record output (beside an fp32 output)")
    _assert_equal(yraw2.to_f32(), split, c.g, f"{what}: raw split record output alone")
    assert _border_is_zero(yraw) and _border_is_zero(yraw2), f"{what}: the border ring of the raw record output is not zero"
    assert _hi_border_is_zero(yrec) and _hi_border_is_zero(yrec2), f"{what}: the border ring of the fp16 record output is not zero"
    assert torch.equal(yrec.to_f32(), yrec2.to_f32()), f"{what}: the fp16 record output depends on the fp32 output"
    if c.out is not None:
        _assert_equal(yrec.to_f32(), c.out.rec, c.out.g, f"{what}: activated fp16 record output")


# ---- 4. conv_out on an fp16 record ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", fx.CLASSES)
def test_record_conv_out_f16(plugin, cuda, cls):
    """k_conv3x3_rec_f16s<1, 1, 2>: one 32-cout tile, fp32 output for the 3 real couts"""
    E = plugin.engine
    c = fx.conv_case(fx.NARROW_CASE, cls)
    what = f"conv_out {fx.NARROW_CASE} {cls}"
    pc = _conv(E, cuda, c)
    assert pc.takes_rec()
    with _m5(E):
        y, yr = pc.call_rec(_f16_record(E, cuda, c, what), want_f32=True)
        torch.cuda.synchronize()
    assert yr is None
    _assert_equal(y, c.want, c.g, what)


# ---- 5. statistics epilogue -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fx.STATS_CASES, ids=_ident)
def test_record_conv_statistics_f16(plugin, cuda, case):
    """k_conv3x3_rec_f16_st through call_rec_stats (family 1; the last row leaves the choice to the launcher): activated fp16 record in
    {0, 32, 64}, sparse integer weights; y and (var, mean) are single bit patterns (gn_exact_ref.expected_stats, lane sums asserted exact)."""
    E = plugin.engine
    c = fx.rec_stats_case(case)
    what = f"fp16 record statistics {case}"
    pc = E.PackedConv(c.w.to(cuda), c.bias.to(cuda))
    assert pc.leaves_stats(32, rec=True)
    r = _dev(c.res, cuda)
    fam = E.CONV_REC_ONE_BLOCK if case[7] == 1 else 0
    with _m5(E):
        xrec = E.rec_from_f32(c.x.to(cuda), c.co.coef.to(cuda))
        assert xrec.fmt == E.REC_F16
        _assert_equal(xrec.to_f32(), c.act, 32.0, f"{what}: fp16 record of the activation")
        y0 = pc.call_rec(xrec, residual=r, want_f32=True, family=fam)[0]
        y1, (var, mean) = pc.call_rec_stats(xrec, residual=r, family=fam, groups=32)
        torch.cuda.synchronize()
    _assert_equal(y1, c.y, c.g, f"{what}: y")
    _assert_equal(y0, c.y, c.g, f"{what}: y of the call without statistics")
    _assert_equal(mean, c.mean, 2.0 ** -23, f"{what}: mean")
    _assert_equal(var, c.var, 2.0 ** -23, f"{what}: var")


# ---- 6. hand-over conv with pre_gn ------------------------------------------------------------------------------------------------------------
def test_handover_cases_reach_every_fp16_form(plugin, cuda):
    E = plugin.engine
    forms = set()
    with _m5(E):
        for case in fx.HANDOVER_CASES:
            pc = E.PackedConv(torch.zeros(case[2], case[1], 3, 3, device=cuda), None)
            assert pc.fuses_pre_gn(), f"{case}: the fp16 hand-over kernel does not take this row"
            forms.add("MT = 2" if case[2] <= 64 else "MT = 4")
            if pc.leaves_stats(32):
                forms.add("statistics")
            if case[2] % 128:
                forms.add("padded couts")
            if case[1] % 32:
                forms.add("unpermuted K order")
    assert forms == {"MT = 2", "MT = 4", "statistics", "padded couts", "unpermuted K order"}


@pytest.mark.parametrize("cls", fx.CLASSES)
@pytest.mark.parametrize("case", fx.HANDOVER_CASES, ids=_ident)
def test_handover_conv_f16(plugin, cuda, case, cls):
    """k_conv3x3_f16<4, true> / <2, true> and, where the shape has one, the statistics form <4, true, 1, true>: fp32 raw input, activated and
    rounded to fp16 while staging -- the operand must be h(act).  Where the record kernels take the shape too, their result on the same case
    is the same tensor: both equal the one exact value."""
    E = plugin.engine
    c = fx.conv_case(case, cls)
    what = f"hand-over conv {case} {cls}"
    pc = _conv(E, cuda, c)
    x, coef, r = c.x.to(cuda), c.co.coef.to(cuda), _dev(c.res, cuda)
    ys = yr = None
    with _m5(E):
        assert pc.fuses_pre_gn()
        y = pc(x, residual=r, pre_gn=coef)
        if pc.leaves_stats(32):
            ys = pc.call_stats(x, coef, residual=r, groups=32)[0]
        if pc.takes_rec():
            yr = pc.call_rec(E.rec_from_f32(x, coef), residual=r, want_f32=True)[0]
        torch.cuda.synchronize()
    _assert_equal(y, c.want, c.g, what)
    if ys is not None:
        _assert_equal(ys, c.want, c.g, f"{what}: statistics form")
    if yr is not None:
        _assert_equal(yr, c.want, c.g, f"{what}: the record kernel on the same case")
        assert torch.equal(yr, y)
    assert (ys is not None) == (case[2] % 128 == 0) and (yr is not None) == (case[2] % 128 == 0 and case[1] % 32 == 0)


@pytest.mark.parametrize("case", gx.HANDOVER_STATS, ids=_ident)
def test_handover_statistics_f16(plugin, cuda, case):
    """The statistics the fp16 hand-over kernel leaves: gn_exact_ref.handover_stats_case ({0, 32, 64} x sparse integers: fp16 numbers, so
    mode 5 must return the bits of the default mode's test)."""
    E = plugin.engine
    c = gx.handover_stats_case(case)
    assert torch.equal(fx.h(c.act), c.act) and torch.equal(fx.h(c.w), c.w)
    pc = E.PackedConv(c.w.to(cuda), c.bias.to(cuda))
    x, coef, r = c.x.to(cuda), c.co.coef.to(cuda), _dev(c.res, cuda)
    with _m5(E):
        assert pc.leaves_stats(32)
        y, (var, mean) = pc.call_stats(x, coef, residual=r, groups=32)
        torch.cuda.synchronize()
    what = f"fp16 hand-over statistics {case}"
    _assert_equal(y, c.y, c.g, f"{what}: y")
    _assert_equal(mean, c.mean, 2.0 ** -23, f"{what}: mean")
    _assert_equal(var, c.var, 2.0 ** -23, f"{what}: var")


# ---- 7. activated fp16 record output of the sub-pixel upsample convs ---------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["one_block", "two_blocks"])
def test_upconv_f16_record_output(plugin, cuda, family):
    """k_upconv_rec_o16 / k_upconv_rec2_o16 on the whole image: three-term MFMAs on the raw lattice record (the fp32 output is the BF16X3 value
    in mode 5), the activated record output is h(a y + s) of that value."""
    E = plugin.engine
    c = fx.up_record_case(lr.REC_UP)
    what = f"upsample conv {lr.REC_UP} {family}"
    pc = E.PackedConv(c.w.to(cuda), c.bias.to(cuda))
    assert pc.takes_rec(True)
    xrec = E.rec_from_f32(c.x.to(cuda))
    _assert_equal(xrec.to_f32(), c.x, c.g, "raw record of x")
    with _m5(E):
        y, yr = pc.call_rec(xrec, upsample2x=True, want_f32=True, want_rec=True, rec_coef=c.out.coef.to(cuda), family=_fam(E, family))
        _, yr2 = pc.call_rec(xrec, upsample2x=True, want_f32=False, want_rec=True, rec_coef=c.out.coef.to(cuda), family=_fam(E, family))
        torch.cuda.synchronize()
    assert yr.fmt == E.REC_F16 and yr2.fmt == E.REC_F16
    _assert_equal(y, c.y, c.g, f"{what}: fp32 output (three terms)")
    _assert_equal(yr.to_f32(), c.out.rec, c.out.g, f"{what}: activated fp16 record output")
    _assert_equal(yr2.to_f32(), c.out.rec, c.out.g, f"{what}: activated fp16 record output alone")
    assert _hi_border_is_zero(yr) and _hi_border_is_zero(yr2), f"{what}: the border ring is not zero"


@pytest.mark.parametrize("family", ["one_block", "two_blocks"])
def test_upconv_window_f16_record_output(plugin, cuda, family):
    """The window entry of the same kernels, two images with different origins: every window pixel is the same pixel of the whole image's
    exact value, in the fp32 output and in the fp16 record."""
    E = plugin.engine
    B, cin, cout, Hin, Win, h, w, y0s, x0s = lr.REC_WINDOW
    c = fx.up_record_case(fx.UP_WINDOW_WHOLE)
    pc = E.PackedConv(c.w.to(cuda), c.bias.to(cuda))
    xrec = E.rec_from_f32(c.x.to(cuda))
    with _m5(E):
        y, yr = pc.call_rec(xrec, upsample2x=True, want_f32=True, want_rec=True, rec_coef=c.out.coef.to(cuda), window=(list(y0s), list(x0s), h, w), family=_fam(E, family))
        torch.cuda.synchronize()
    assert yr.fmt == E.REC_F16
    y, yr32 = y.cpu(), yr.to_f32().cpu()
    for b in range(B):
        y0, x0 = y0s[b], x0s[b]
        what = f"upsample window image {b} at ({y0}, {x0}) {family}"
        rows, cols = slice(2 * y0, 2 * (y0 + h)), slice(2 * x0, 2 * (x0 + w))
        _assert_equal(y[b:b + 1], c.y[b:b + 1, :, rows, cols], c.g, f"{what}: fp32 output")
        _assert_equal(yr32[b:b + 1], c.out.rec[b:b + 1, :, rows, cols], c.out.g, f"{what}: activated fp16 record output")
    assert _hi_border_is_zero(yr)


def test_direct_conv_refuses_an_fp16_record_output_from_a_split_input(plugin, cuda):
    """No direct kernel pairs a bf16 split input with the fp16 record-out epilogue.  The launcher used to run the three-term kernel, which
    wrote a bf16 split into an image the caller held as the fp16 form (found while writing this module); now the call is refused."""
    E = plugin.engine
    c = fx.up_record_case(lr.REC_UP)
    pc = E.PackedConv(c.w.to(cuda), c.bias.to(cuda))
    xrec = E.rec_from_f32(c.x.to(cuda))
    B, cout = c.out.coef.shape[0], c.out.coef.shape[2]
    coef = torch.stack([torch.ones(B, cout), torch.full((B, cout), 64.0)], dim=1).contiguous().to(cuda)
    with _m5(E):
        with pytest.raises(E.MdtileError, match="record format mismatch"):
            pc.call_rec(xrec, want_f32=True, want_rec=True, rec_coef=coef)
        y, yr = pc.call_rec(xrec, want_f32=True, want_rec=True)      # a raw record output is a bf16 split in every mode: still taken
        torch.cuda.synchronize()
    assert yr.fmt == E.REC_BF16X2


# ---- 8. cross-mode ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["record", "handover"])
def test_integer_class_gives_the_same_bits_in_mode_5_bf16x3_and_bf16(plugin, cuda, route):
    """{0, 32, 64} x small integers are fp16 and bf16 numbers: one fp16 term, three bf16 terms and one bf16 term are the same sum."""
    E = plugin.engine
    case = lr.REC_DIRECT[1] if route == "record" else lr.HANDOVER_3X3[0]
    c = fx.conv_case(case, "integer")
    pc = _conv(E, cuda, c)
    x, coef, r = c.x.to(cuda), c.co.coef.to(cuda), _dev(c.res, cuda)
    out = {}
    for name, mode in (("F16", E.PRECISION_F16), ("BF16X3", E.PRECISION_BF16X3), ("BF16", E.PRECISION_BF16)):
        with E.precision(mode):
            if route == "record":
                rec = E.rec_from_f32(x, coef)
                assert rec.fmt == (E.REC_F16 if name == "F16" else E.REC_BF16X2)
                out[name] = pc.call_rec(rec, residual=r, want_f32=True)[0]
            else:
                out[name] = pc(x, residual=r, pre_gn=coef)
            torch.cuda.synchronize()
    for name, y in out.items():
        _assert_equal(y, c.want, c.g, f"{route} {case} integer class in {name}")
    assert torch.equal(out["F16"], out["BF16X3"]) and torch.equal(out["F16"], out["BF16"])
