"""Bit-exact tests of the GroupNorm chain the decoder runs at every block (tests/gn_exact_ref.py): the statistics pass, its row-band and
pooled forms, the statistics the conv epilogues leave (hand-over and record kernels), the fixed-statistics apply, the fused
GroupNorm + SiLU input of the hand-over conv, rec_from_f32(x, coef) and the activated record output.

tests/test_gpu_conv_lattice.py left these out because SiLU leaves the lattice and sum y^2 needs ~60 bits.  Two observations lift that:
statistics are exact on small integers (|y| <= 255 grains: every fp32 lane partial and every fp64 sum is exact, so (var, mean) is one bit
pattern), and every SiLU of the project is the identity on a saturated set (t >= 24: 1.0f + e^-t == 1.0f) and 0 at 0.  Inputs are built
backwards from the activation they must produce (gn_exact_ref.raw_for: a = +-2^m, dyadic s), so every link has one expected bit pattern
and every assertion is torch.equal; a mismatch message gives the count of differing elements, the first index and the difference in
grains.  The only tolerance in the module is the derived 4 ulp bound of the unsaturated SiLU.  tests/test_gn_exact_host.py proves the
instrument: the orders agree, every precondition holds for every case row, the wrong kernels a tolerance lets through change bits.
The first two tests probe what the rest supposes about the hardware: rcp(1.0f) == 1.0f, and an exact sqrtf / division on powers of 4 / 2.
MDTILE_PRECISION_F16 runs the same chain on fp16 operands: tests/test_gpu_f16_exact.py covers it on operand classes of its own
(tests/f16_exact_ref.py).  Out of scope: mdtile vae_fast_input (its renormalisation divides by a standard deviation: no exact class).  Every test leaves the default precision mode behind."""
import pytest
import torch

import gn_exact_ref as gx
import lattice_ref as lr

pytestmark = pytest.mark.gpu

TERMS_OF_MODE = {"bf16x3": "hh+hl+lh", "bf16": "hh"}


@pytest.fixture(autouse=True)
def _default_mode_after(plugin):
    E = plugin.engine
    assert E.get_precision() == E.PRECISION_BF16X3
    yield
    mode = E.get_precision()
    E.set_precision(E.PRECISION_BF16X3)
    assert mode == E.PRECISION_BF16X3, "a test leaked its precision mode"


def _mode(E, mode):
    return E.precision({"bf16x3": E.PRECISION_BF16X3, "bf16": E.PRECISION_BF16}[mode])


def _assert_equal(got, want, g, what):
    got = got.cpu()
    assert torch.equal(got, want), f"{what}: {lr.mismatch_report(got, want, g)}"


def _assert_stats(got, want_var, want_mean, what):
    """(var, mean) against the expected pair; the 'grain' of the report is one ulp-ish unit of the largest expected value"""
    var, mean = got
    _assert_equal(mean, want_mean, 2.0 ** -23, f"{what}: mean")
    _assert_equal(var, want_var, 2.0 ** -23, f"{what}: var")


def _unaligned(t, cuda):
    """the same values from a view one float into a larger buffer: every group / plane base moves by 4 bytes"""
    buf = torch.zeros(t.numel() + 1, device=cuda)
    buf[1:] = t.to(cuda).reshape(-1)
    return buf[1:].view(t.shape)


def _border_is_zero(rec):
    r = rec.records()
    return not (r[:, :, :, 0].any() or r[:, :, :, -1].any() or r[:, :, :, :, 0].any() or r[:, :, :, :, -1].any())


def _ident(s):
    return "x".join(str(int(v)) for v in s)


# ---- 1. probes ------------------------------------------------------------------------------------------------------------------------------
def _probe_tensor(C, H=2, W=4):
    vals = torch.tensor(gx.PROBE_VALUES)
    idx = (torch.arange(C).view(C, 1, 1) + torch.arange(H).view(1, H, 1) * W + torch.arange(W).view(1, 1, W)) % len(vals)
    x = vals[idx].view(1, C, H, W).contiguous()
    gx.assert_saturated(x)
    assert set(torch.unique(x).tolist()) == set(gx.PROBE_VALUES)
    return x


def _identity_conv(E, cuda, C):
    w = torch.zeros(C, C, 3, 3)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    return E.PackedConv(w.to(cuda), None)


@pytest.mark.parametrize("form", ["silu", "gn_apply", "rec_from_f32", "handover_input", "record_output", "record_output_up"])
def test_probe_silu_is_the_identity_on_the_saturated_set(plugin, cuda, form):
    """Every form of SiLU returns t itself on {0, 32, 40, 48, 56, 32 + 2^-5, 63.96875, 4000}: rcp(1.0f) == 1.0f on this hardware (and
    1.0f / 1.0f, trivially).  Every probe value is a 16-bit number, so a split-bf16 identity conv passes it unchanged."""
    E = plugin.engine
    C, H, W = (128, 8, 12) if form.startswith("record_output") else (64, 2, 4)      # (the record convs: the smallest plane their other tests use)
    x = _probe_tensor(C, H, W)
    unit = gx.unit_coef(1, C).to(cuda)
    want = x
    if form == "silu":
        got = E.silu(x.to(cuda))
        _assert_equal(E.silu(_unaligned(x, cuda)), want, 2.0 ** -5, "silu, scalar path")
    elif form == "gn_apply":
        # mean 0, var + eps == 1: a = 1, s = 0
        co = torch.zeros(32), torch.full((32,), float(torch.tensor(1.0) - torch.tensor(1e-6)))
        assert float(co[1][0] + torch.tensor(1e-6)) == 1.0
        got = E.gn_apply(x.to(cuda), co[0].to(cuda), co[1].to(cuda), silu=True)
    elif form == "rec_from_f32":
        rec = E.rec_from_f32(x.to(cuda), unit)
        assert _border_is_zero(rec)
        got = rec.to_f32()
    elif form == "handover_input":
        pc = _identity_conv(E, cuda, C)
        assert pc.fuses_pre_gn()
        got = pc(x.to(cuda), pre_gn=unit)
    else:
        up = form.endswith("_up")
        pc = _identity_conv(E, cuda, C)
        assert pc.takes_rec(up)
        xrec = E.rec_from_f32(x.to(cuda))
        _assert_equal(xrec.to_f32(), x, 2.0 ** -5, "raw record of the probe values")
        if up:      # nearest-2x, then the centre tap: every output pixel is its input pixel
            want = torch.nn.functional.interpolate(x, scale_factor=2.0, mode="nearest")
        for fam in (E.CONV_REC_ONE_BLOCK, E.CONV_REC_TWO_BLOCKS):
            y, yr = pc.call_rec(xrec, upsample2x=up, want_f32=True, want_rec=True, rec_coef=unit, family=fam)
            _assert_equal(y, want, 2.0 ** -5, f"{form} family {fam}: fp32 output")
            assert _border_is_zero(yr)
            got = yr.to_f32()
            _assert_equal(got, want, 2.0 ** -5, f"{form} family {fam}")
    torch.cuda.synchronize()
    _assert_equal(got, want, 2.0 ** -5, form)


@pytest.mark.parametrize("B,C,groups,affine,silu_class", gx.COEFF_PROBES)
def test_probe_gn_coeffs_are_exact(plugin, cuda, B, C, groups, affine, silu_class):
    """var = fl32(4^-k - 1e-6f): with the production eps, 1.0f / sqrtf(var + eps) must be 2^k exactly -- gn_coeffs returns (a, s) of
    gn_exact_ref.exact_coeffs bit for bit, for gamma = +-2^m and +-{1, 1.25, 1.5, 1.75}.  Also without gamma and beta."""
    E = plugin.engine
    co = gx.coeff_probe(B, C, groups, affine, silu_class)
    got = E.gn_coeffs(co.mean.to(cuda), co.var.to(cuda), None if co.gamma is None else co.gamma.to(cuda),
                      None if co.beta is None else co.beta.to(cuda), C, groups)
    _assert_equal(got, co.coef, 2.0 ** -8, f"gn_coeffs B={B} C={C} groups={groups} affine={affine}")


# ---- 2. statistics pass ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", gx.STATS_OFFSETS)
@pytest.mark.parametrize("shape", gx.STATS_SHAPES, ids=_ident)
def test_statistics_pass(plugin, cuda, shape, offset):
    E = plugin.engine
    c = gx.stats_case(shape, offset)
    _assert_stats(E.gn_stats(c.x.to(cuda), 32), c.var, c.mean, f"gn_stats {shape} +{offset}")
    _assert_stats(E.gn_stats(_unaligned(c.x, cuda), 32), c.var, c.mean, f"gn_stats {shape} +{offset} from an unaligned view")


# ---- 3. row bands ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", gx.STATS_OFFSETS)
def test_row_band_sums(plugin, cuda, offset):
    E = plugin.engine
    c = gx.stats_case(gx.BAND_SHAPE, offset)
    x = c.x.to(cuda)
    B, C, H, W = gx.BAND_SHAPE
    sums = {}
    for lo, hi in gx.BANDS:
        sums[(lo, hi)] = E.gn_sums(x, lo, hi, 32)
        want = gx.expected_sums(c.x, 32, lo, hi)
        got = sums[(lo, hi)].cpu()
        assert got.dtype == torch.float64 and torch.equal(got, want), f"gn_sums rows [{lo}, {hi}): {lr.mismatch_report(got, want, 1.0)}"
    whole = E.gn_stats(x, 32)
    _assert_stats(whole, c.var, c.mean, "gn_stats on the band tensor")
    count = (C // 32) * H * W
    for what, s in (("one band", sums[(0, 12)]), ("two bands", sums[(0, 5)] + sums[(5, 12)])):
        got = E.gn_from_sums(s, count)
        _assert_stats(got, c.var, c.mean, f"gn_from_sums of {what}")
        assert torch.equal(got[0], whole[0]) and torch.equal(got[1], whole[1])


# ---- 4. pooled statistics -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixels", gx.POOL_CASES, ids=_ident)
def test_pooled_statistics(plugin, cuda, pixels):
    E = plugin.engine
    c = gx.pool_case(pixels)
    _assert_stats(E.gn_pool(c.means.to(cuda), c.vars.to(cuda), list(c.pixels)), c.var, c.mean, f"gn_pool {pixels}")


# ---- 5. epilogue statistics, hand-over kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("case", gx.HANDOVER_STATS, ids=_ident)
def test_handover_epilogue_statistics(plugin, cuda, case, mode):
    """The activation {0, 32, 64} and the integer weights have lo = 0: both modes must return the same bits."""
    E = plugin.engine
    c = gx.handover_stats_case(case)
    pc = E.PackedConv(c.w.to(cuda), c.bias.to(cuda))
    assert pc.leaves_stats(32)
    x, coef = c.x.to(cuda), c.co.coef.to(cuda)
    r = None if c.res is None else c.res.to(cuda)
    with _mode(E, mode):
        y0 = pc(x, residual=r, pre_gn=coef)
        y1, stats = pc.call_stats(x, coef, residual=r, groups=32)
        torch.cuda.synchronize()
    what = f"hand-over {case} {mode}"
    _assert_equal(y1, c.y, c.g, f"{what}: y")
    _assert_equal(y0, c.y, c.g, f"{what}: y of the call without statistics")
    _assert_stats(stats, c.var, c.mean, f"{what}: epilogue statistics")
    _assert_stats(E.gn_stats(y1, 32), c.var, c.mean, f"{what}: the statistics pass on the same y")


# ---- 6. epilogue statistics, record kernels -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("case", gx.REC_STATS, ids=_ident)
def test_record_epilogue_statistics(plugin, cuda, case, mode):
    E = plugin.engine
    B, cin, cout, H, W, res, up, family = case
    c = gx.rec_stats_case(case)
    pc = E.PackedConv(c.w.to(cuda), c.bias.to(cuda))
    assert pc.leaves_stats(32, upsample2x=up, rec=True)
    xrec = E.rec_from_f32(c.x.to(cuda))
    _assert_equal(xrec.to_f32(), c.x, 1.0, "record image of x")
    r = None if c.res is None else c.res.to(cuda)
    fam = E.CONV_REC_ONE_BLOCK if family == 1 else 0
    with _mode(E, mode):
        y0, _ = pc.call_rec(xrec, residual=r, upsample2x=up, want_f32=True, family=fam)
        y1, stats = pc.call_rec_stats(xrec, residual=r, upsample2x=up, family=fam, groups=32)
        torch.cuda.synchronize()
    what = f"record {case} {mode}"
    _assert_equal(y1, c.y, c.g, f"{what}: y")
    _assert_equal(y0, c.y, c.g, f"{what}: y of the call without statistics")
    _assert_stats(stats, c.var, c.mean, f"{what}: epilogue statistics")
    _assert_stats(E.gn_stats(y1, 32), c.var, c.mean, f"{what}: the statistics pass on the same y")


# ---- 7. fixed-statistics apply --------------------------------------------------------------------------------------------------------------
def _gn_apply(E, cuda, x, co, silu):
    return E.gn_apply(x, co.mean.to(cuda), co.var.to(cuda), None if co.gamma is None else co.gamma.to(cuda), None if co.beta is None else co.beta.to(cuda),
                      groups=co.groups, silu=silu)


@pytest.mark.parametrize("cls", gx.APPLY_CLASSES)
@pytest.mark.parametrize("shape", gx.APPLY_SHAPES, ids=_ident)
def test_apply_fixed_statistics(plugin, cuda, shape, cls):
    E = plugin.engine
    c = gx.apply_case(shape, cls)
    silu = cls == "silu"
    _assert_equal(_gn_apply(E, cuda, c.x.to(cuda), c.co, silu), c.want, c.g, f"gn_apply {shape} {cls}")
    x1 = _unaligned(c.x, cuda)
    out = torch.zeros(c.x.numel() + 1, device=cuda)[1:].view(shape)
    got = E.gn_apply(x1, c.co.mean.to(cuda), c.co.var.to(cuda), None if c.co.gamma is None else c.co.gamma.to(cuda),
                     None if c.co.beta is None else c.co.beta.to(cuda), groups=32, silu=silu, out=out)
    _assert_equal(got, c.want, c.g, f"gn_apply {shape} {cls} from and to unaligned views")


@pytest.mark.parametrize("shape", gx.APPLY_SHAPES[:3], ids=_ident)
def test_apply_agrees_with_gn_coeffs_on_any_statistics(plugin, cuda, shape):
    """No assumption about rounding: with random, non-exact mean, var, gamma, beta, gn_apply(zeros) is the s row of gn_coeffs, and
    gn_apply(ones) with mean = 0 and beta = 0 is the a row -- the two kernels form their constants the same way."""
    E = plugin.engine
    B, C, H, W = shape
    gen = torch.Generator().manual_seed(C + H)
    mean, var = torch.randn(B * 32, generator=gen).to(cuda), (torch.rand(B * 32, generator=gen) * 3 + 0.01).to(cuda)
    gamma, beta = torch.randn(C, generator=gen).to(cuda), torch.randn(C, generator=gen).to(cuda)
    coef = E.gn_coeffs(mean, var, gamma, beta, C, 32).cpu()
    got = E.gn_apply(torch.zeros(shape, device=cuda), mean, var, gamma, beta).cpu()
    _assert_equal(got, coef[:, 1].reshape(B, C, 1, 1).expand(shape).contiguous(), 2.0 ** -23, "gn_apply(zeros) against the s row")
    zero_m, zero_b = torch.zeros_like(mean), torch.zeros_like(beta)
    coef0 = E.gn_coeffs(zero_m, var, gamma, zero_b, C, 32).cpu()
    assert torch.equal(coef0[:, 0], coef[:, 0]) and not coef0[:, 1].any()
    got = E.gn_apply(torch.ones(shape, device=cuda), zero_m, var, gamma, zero_b).cpu()
    _assert_equal(got, coef[:, 0].reshape(B, C, 1, 1).expand(shape).contiguous(), 2.0 ** -23, "gn_apply(ones) against the a row")


def test_apply_unsaturated_silu_within_4_ulp(plugin, cuda):
    """The one tolerance of the module.  Lattice x, exact coefficients, so t = a x + s is exact and |t| <= 16; against SiLU in fp64 of that t.
    Bound: 4 ulp of the fp32 reference value -- expf <= 1 ulp (HIP's documented bound), damped by e / (1 + e) on its way into 1 + e; the
    add <= 0.5; the division <= 1 (2.5 in all, documented bounds added linearly); the rounding of the reference 0.5; rounded up to 4.
    Measured on MI355X: 1.82 ulp."""
    E = plugin.engine
    u = gx.unsaturated_case()
    got = E.gn_apply(u.x.to(cuda), u.mean.to(cuda), u.var.to(cuda), u.gamma.to(cuda), u.beta.to(cuda), silu=True).cpu()
    lin = E.gn_apply(u.x.to(cuda), u.mean.to(cuda), u.var.to(cuda), u.gamma.to(cuda), u.beta.to(cuda), silu=False).cpu()
    _assert_equal(lin, u.t, 2.0 ** -20, "t = a x + s")
    ref32 = u.want.float()
    ulp = torch.nextafter(ref32.abs(), torch.full_like(ref32, float("inf"))).double() - ref32.abs().double()
    err = ((got.double() - u.want).abs() / ulp)
    print(f"unsaturated SiLU: max error {err.max().item():.3f} ulp of the fp32 reference over |t| <= {u.t.abs().max().item():.2f}")
    assert err.max().item() <= 4.0


# ---- 8. fused GroupNorm + SiLU input of the hand-over conv ----------------------------------------------------------------------------------
def test_fused_input_cases_reach_every_cout_block_variant(plugin, cuda):
    E = plugin.engine
    fused = []
    for case in gx.FUSED_CASES:
        B, cin, cout, H, W, res = case
        pc = E.PackedConv(torch.zeros(cout, cin, 3, 3, device=cuda), None)
        if pc.fuses_pre_gn():
            fused.append(case)
    assert any(c[2] <= 64 for c in fused), "no case on the 64-cout block kernel"
    assert any(c[2] > 64 and c[2] % 128 == 0 for c in fused) and any(c[2] % 128 != 0 and c[2] > 64 for c in fused), "no case on the 128-cout block kernel"
    assert len(fused) == len(gx.FUSED_CASES), "a row of the table lost its fused kernel: the parametrised test would skip it"
    with E.precision(E.PRECISION_F32):
        assert not E.PackedConv(torch.zeros(128, 128, 3, 3, device=cuda), None).fuses_pre_gn()      # no fused kernel in the exact mode: nothing to test there


@pytest.mark.parametrize("cls,mode", [("lattice", "bf16x3"), ("lattice", "bf16"), ("integer", "bf16x3"), ("integer", "bf16")])
@pytest.mark.parametrize("case", gx.FUSED_CASES, ids=_ident)
def test_fused_gn_silu_input(plugin, cuda, case, cls, mode):
    """pc(x, pre_gn=coef) with x = raw_for(32 |lattice x|): per-channel a and s differ between neighbours and a is negative on half of them,
    so a wrong channel, a lost sign or a pad pixel that is not zero changes bits.  Also equal to the unfused pair gn_apply + conv: on this
    set the two forms of SiLU agree exactly."""
    E = plugin.engine
    c = gx.fused_case(case, cls)
    pc = E.PackedConv(c.w.to(cuda), c.bias.to(cuda))
    x, coef = c.x.to(cuda), c.co.coef.to(cuda)
    r = None if c.res is None else c.res.to(cuda)
    with _mode(E, mode):
        assert pc.fuses_pre_gn()
        y = pc(x, residual=r, pre_gn=coef)
        act = _gn_apply(E, cuda, x, c.co, True)
        y2 = pc(act, residual=r)
        torch.cuda.synchronize()
    what = f"fused input {case} {cls} {mode}"
    _assert_equal(act, c.act, c.g, f"{what}: gn_apply(x, silu=True)")
    _assert_equal(y, c.want[TERMS_OF_MODE[mode]], c.g, what)
    _assert_equal(y2, c.want[TERMS_OF_MODE[mode]], c.g, f"{what}: gn_apply, then the plain conv")


# ---- 9. activated record images -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gx.REC_FROM_SHAPES, ids=_ident)
def test_activated_record_from_f32(plugin, cuda, shape):
    """rec_from_f32(raw_for(32 |lattice x|), coef): the record image reads back as the activation itself, inside a ring of zeros."""
    E = plugin.engine
    c = gx.rec_from_case(shape)
    rec = E.rec_from_f32(c.x.to(cuda), c.co.coef.to(cuda))
    _assert_equal(rec.to_f32(), lr.expected_split(c.want), 2.0 ** -5, f"rec_from_f32(x, coef) {shape}")
    assert _border_is_zero(rec), "the border ring is not zero"


@pytest.mark.parametrize("family", ["one_block", "two_blocks"])
@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("case,up", gx.REC_ACT_CASES, ids=lambda v: _ident(v[:5]) if isinstance(v, tuple) else ("up" if v else "direct"))
def test_activated_record_output(plugin, cuda, case, up, mode, family):
    """Record conv with rec_coef: the record output is split(silu(a y + s)) = split(t) with t exact and saturated (gn_exact_ref.rec_act_case);
    the fp32 output of the same launch is still the conv's exact value; the border ring is zero."""
    E = plugin.engine
    c = gx.rec_act_case(case, up)
    terms = TERMS_OF_MODE[mode]
    pc = E.PackedConv(c.w.to(cuda), c.bias.to(cuda))
    assert pc.takes_rec(up)
    xrec = E.rec_from_f32(c.x.to(cuda))
    r = None if c.res is None else c.res.to(cuda)
    fam = E.CONV_REC_ONE_BLOCK if family == "one_block" else E.CONV_REC_TWO_BLOCKS
    coef = c.coef.to(cuda)
    with _mode(E, mode):
        y, yr = pc.call_rec(xrec, residual=r, upsample2x=up, want_f32=True, want_rec=True, rec_coef=coef, family=fam)
        _, yr2 = pc.call_rec(xrec, residual=r, upsample2x=up, want_f32=False, want_rec=True, rec_coef=coef, family=fam)
        torch.cuda.synchronize()
    what = f"activated record {case} up={up} {mode} {family}"
    _assert_equal(y, c.y[terms], c.g, f"{what}: fp32 output of the same launch")
    _assert_equal(yr.to_f32(), c.rec[terms], c.gt, f"{what}: record output")
    _assert_equal(yr2.to_f32(), c.rec[terms], c.gt, f"{what}: record output alone")
    assert _border_is_zero(yr) and _border_is_zero(yr2), f"{what}: the border ring is not zero"


# ---- 10. the routes agree -------------------------------------------------------------------------------------------------------------------
def test_every_statistics_route_gives_the_same_bits(plugin, cuda):
    """One integer y (a record conv's output): gn_stats, gn_from_sums of two bands, the record epilogue's pair and the hand-over epilogue's
    pair -- that kernel computes 32 y from an activated input (gn_exact_ref.routes_case), whose (var, mean) are (1024 var, 32 mean) exactly --
    are bit-equal and equal the expected value."""
    E = plugin.engine
    B, cin, cout, H, W = gx.ROUTES_CASE[:5]
    rc = gx.routes_case()
    c = rc.rec
    pc = E.PackedConv(c.w.to(cuda), c.bias.to(cuda))
    y, rec_pair = pc.call_rec_stats(E.rec_from_f32(c.x.to(cuda)), residual=c.res.to(cuda), family=E.CONV_REC_ONE_BLOCK, groups=32)
    _assert_equal(y, c.y, 1.0, "y")
    pairs = {"record epilogue": rec_pair, "gn_stats": E.gn_stats(y, 32)}
    h = H // 2 + 1
    pairs["gn_from_sums of two bands"] = E.gn_from_sums(E.gn_sums(y, 0, h, 32) + E.gn_sums(y, h, H, 32), (cout // 32) * H * W)
    pc32 = E.PackedConv(c.w.to(cuda), rc.bias_hand.to(cuda))
    assert pc32.leaves_stats(32)
    yh, hand_pair = pc32.call_stats(rc.x_hand.to(cuda), rc.co.coef.to(cuda), residual=rc.res_hand.to(cuda), groups=32)
    _assert_equal(yh, rc.y_hand, 32.0, "hand-over y = 32 x the record conv's y")
    _assert_stats(hand_pair, rc.var_hand, rc.mean_hand, "hand-over epilogue, of 32 y")
    pairs["hand-over epilogue (of 32 y, scaled back)"] = (hand_pair[0] / 1024.0, hand_pair[1] / 32.0)
    for what, pair in pairs.items():
        _assert_stats(pair, c.var, c.mean, what)
    first = pairs["gn_stats"]
    for what, pair in pairs.items():
        assert torch.equal(pair[0], first[0]) and torch.equal(pair[1], first[1]), f"{what} differs from gn_stats"
