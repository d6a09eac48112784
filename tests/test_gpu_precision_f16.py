"""MDTILE_PRECISION_F16 on the GPU: the fp16 record producers, every fp16 consumer against its exact contract, the tiled VAE end to end, range
safety and stability.

Contract of the mode (include/mdtile.h): a 3x3 conv whose operand the library itself produces as silu(a x + s) is fp16_rn(act) x fp16_rn(w) with
fp32 accumulation; a conv on the raw residual stream keeps the three-term bf16 kernels; the attention is mode 2's; the rest is fp32.
  * producers: to_f32() of an fp16 record is within half an fp16 ulp of the fp64 activation plus the fp32 activation's own error -- taken as the
    distance of the BF16X3 record (hi + lo) of the same input from the same fp64 value, plus a few fp32 ulps (_check_fp16_record says why);
  * consumers: an fp64 reference on the operands the kernel really sees (the record read back through to_f32(), fp16_rn(w)); the tolerance is
    fp32 accumulation order, TOL_EXACT of the bf16 tests.  The same call in the default mode must be >= 10x further from that reference;
  * end to end: the error against the fp32 oracle must be <= 1/2 of mode 2's on the same case in the same process (tools/precision_model.py
    predicts >= 4.2x; a factor 2 is left for tiling and frozen statistics).  The torch-float16 oracle's error is printed, not gated.
Every test leaves the default mode behind."""
import pytest
import torch
import torch.nn.functional as F

from hostsim import ldm_decoder as ld
from oracle import gpu_reference as gr
from oracle import vae_oracle as vo

pytestmark = pytest.mark.gpu

TOL_EXACT = 2e-5


@pytest.fixture(autouse=True)
def _default_mode_after(plugin):
    E = plugin.engine
    assert E.get_precision() == E.PRECISION_BF16X3
    yield
    mode = E.get_precision()
    E.set_precision(E.PRECISION_BF16X3)
    assert mode == E.PRECISION_BF16X3, "a test leaked its precision mode"


def _h(t: torch.Tensor) -> torch.Tensor:
    """fp16_rn of the value clamped to +-65504 (v_med3_f32 + v_cvt_pk_f16_f32), subnormals kept, widened to fp64."""
    return t.detach().float().clamp(-65504.0, 65504.0).to(torch.float16).to(torch.float64)


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _ulp16(v: torch.Tensor) -> torch.Tensor:
    """spacing of fp16 at |v| (fp64 tensor): 2^(e - 10) for 2^e <= |v| < 2^(e + 1), 2^-24 below 2^-14"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -14))          # |v| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(v), e - 1 - 10)


def _coef(B, C, seed, big=False):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(B, 1, C, generator=g) * 1.5 + 0.25
    s = torch.randn(B, 1, C, generator=g) * 0.5
    if big:
        a[:, :, ::7] *= 3.0e4          # activations far beyond fp16's range in every seventh channel
    return torch.cat([a, s], dim=1).contiguous()


def _check_fp16_record(name, got16, split3, x, coef):
    """got16: to_f32() of the fp16 record; split3: to_f32() of the BF16X3 record (hi + lo) of the same values; x, coef: what was activated.
    Bound per element: half an fp16 ulp AT THE EXPECTED VALUE, plus the fp32 activation's own error = the BF16X3 record's distance from the fp64
    value, plus an fp32-rounding-sized term: hi + lo is the fp32 activation cut to 16 bits, so its distance from fp64 can be smaller than the
    fp32 activation's own (the cut may cancel it), and the fp16 form rounds the UNCUT value.  That term is (4 + min(|t|, 20)) fp32 ulps of the
    value, t = a x + s: fma, the scaling by log2(e), v_exp_f32 and v_rcp_f32 round once each (<= 1 ulp each), and the rounding of the exponent's
    argument is |t| 2^-24 relative in e^-t (beyond |t| = 20, e^-|t| < 2e-9 carries nothing)."""
    t64 = x.double().cpu() * coef[:, 0].double().cpu()[:, :, None, None] + coef[:, 1].double().cpu()[:, :, None, None]
    ref64 = t64 * torch.sigmoid(t64)
    got16, split3 = got16.double().cpu(), split3.double().cpu()
    assert torch.isfinite(got16).all(), f"{name}: Inf / NaN in an fp16 record"
    assert got16.abs().max().item() <= 65504.0
    want = ref64.clamp(-65504.0, 65504.0)
    own = (split3 - ref64).abs() + 2.0 ** -23 * (4.0 + t64.abs().clamp_max(20.0)) * ref64.abs()
    over = ref64.abs() > 65504.0
    own = torch.where(over, torch.zeros_like(own), own)                  # beyond the range the value IS the clamp
    tol = 0.5 * _ulp16(want) + own
    d = (got16 - want).abs()
    worst = (d / tol).max().item()
    # (worst ratio seen on an MI355X over every producer case of this file: 0.9996 -- round-to-nearest reaches the half ulp)
    print(f"{name}: fp16 record vs fp64 activation: worst |d| / (ulp/2 + own error) = {worst:.4f}; {int(over.sum())} values beyond +-65504")
    assert worst <= 1.0, f"{name}: fp16 record off by {worst:.4f} x its tolerance"
    if over.any():
        assert (got16[over].abs() == 65504.0).all(), f"{name}: a value beyond the range did not read back as +-65504"
    return ref64


# ---------------------------------------------------------------------------------------------------------------- producers
@pytest.mark.parametrize("B,C,H,W,big", [(1, 128, 17, 45, False), (2, 256, 24, 40, True), (1, 32, 5, 3, True)])
def test_rec_from_f32_writes_the_fp16_form(plugin, cuda, B, C, H, W, big):
    E = plugin.engine
    torch.manual_seed(C + H)
    x = torch.randn(B, C, H, W) * (4.0 if big else 1.0)
    coef = _coef(B, C, 3 + C, big)
    xd, cd = x.to(cuda), coef.to(cuda)
    split = E.rec_from_f32(xd, cd)
    assert split.fmt == E.REC_BF16X2
    with E.precision(E.PRECISION_F16):
        rec = E.rec_from_f32(xd, cd)
        raw = E.rec_from_f32(xd)
        assert rec.fmt == E.REC_F16 and raw.fmt == E.REC_BF16X2       # a raw record is a bf16 split in every mode
        got = rec.to_f32()
        assert torch.equal(raw.records(), E.rec_from_f32(xd).records())
        torch.cuda.synchronize()
    assert torch.equal(raw.to_f32(), E.rec_from_f32(xd).to_f32())
    ref = _check_fp16_record(f"rec_from_f32 {(B, C, H, W)}", got, split.to_f32(), x, coef)
    if big:
        assert (ref.abs() > 65504.0).any()
    # the border of the hi half is zero (the conv's padding); the lo half is not part of the form
    r = rec.records()[:, 0]
    assert not r[:, :, 0].any() and not r[:, :, -1].any() and not r[:, :, :, 0].any() and not r[:, :, :, -1].any()


def test_a_record_is_rejected_in_the_wrong_mode(plugin, cuda):
    E = plugin.engine
    torch.manual_seed(1)
    conv = torch.nn.Conv2d(128, 128, 3, 1, 1)
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    x, coef = torch.randn(1, 128, 16, 32, device=cuda), _coef(1, 128, 2).to(cuda)
    with E.precision(E.PRECISION_F16):
        rec = E.rec_from_f32(x, coef)
    for mode in (E.PRECISION_BF16X3, E.PRECISION_BF16):
        with E.precision(mode):
            with pytest.raises(E.MdtileError, match="record format mismatch"):
                pc.call_rec(rec, want_f32=True)
    assert torch.isfinite(rec.to_f32()).all()          # reading it is always possible: the tag travels with the image


# ---------------------------------------------------------------------------------------------------------------- consumers
def _check_exact(name, f16, three, ref):
    e1, e3 = _rel(f16, ref), _rel(three, ref)
    print(f"{name}: fp16 kernel vs fp16-operand fp64 reference {e1:.2e}, the default mode {e3:.2e}")
    assert torch.isfinite(f16).all()
    assert e1 < TOL_EXACT, f"{name}: fp16 kernel off its contract: rel err {e1}"
    assert e3 >= 10 * max(e1, 1e-7), f"{name}: the default mode is as close to the fp16-operand reference ({e3}) as mode 5 ({e1})"


REC_CASES = [  # B, cin, cout, H, W (output), residual     (tests/test_gpu_precision_bf16.py's, without the upsample cases)
    (1, 128, 128, 16, 32, False),     # exactly one block
    (1, 128, 128, 17, 45, True),      # ragged rows and columns
    (2, 256, 128, 40, 36, True),      # batch 2, 16 K-steps
    (1, 512, 512, 24, 40, False),     # 4 cout blocks
]


def _conv_setup(cuda, E, B, cin, cout, H, W, res, seed, k=3):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, k, 1, k // 2)
    x = torch.randn(B, cin, H, W)
    r = torch.randn(B, cout, H, W) if res else None
    coef = _coef(B, cin, seed + 1)
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    return conv, x.to(cuda), None if r is None else r.to(cuda), coef.to(cuda), pc


def _ref(operand, conv, r):
    ref = F.conv2d(operand.double().cpu(), _h(conv.weight), conv.bias.detach().double(), padding=1)
    return ref if r is None else ref + r.double().cpu()


@pytest.mark.parametrize("family", ["one_block", "two_blocks"])
@pytest.mark.parametrize("B,cin,cout,H,W,res", REC_CASES)
def test_record_conv_fp16(plugin, cuda, B, cin, cout, H, W, res, family):
    """k_conv3x3_rec_f16 / _f16s (one block per CU) and k_conv3x3_rec2_f16 / _f16s (two blocks per CU), fp32 and record output."""
    E = plugin.engine
    conv, x, r, coef, pc = _conv_setup(cuda, E, B, cin, cout, H, W, res, cin + 7 * cout + H)
    ycoef = _coef(B, cout, 5 * cout + W).to(cuda)
    fam = E.CONV_REC_ONE_BLOCK if family == "one_block" else E.CONV_REC_TWO_BLOCKS
    with E.precision(E.PRECISION_F16):
        xrec = E.rec_from_f32(x, coef)
        operand = xrec.to_f32()
        y, _ = pc.call_rec(xrec, residual=r, want_f32=True, family=fam)                                            # _f16s, fp32 only
        y2, yrec = pc.call_rec(xrec, residual=r, want_f32=True, want_rec=True, rec_coef=ycoef, family=fam)         # _f16: fp16 record out
        _, yraw = pc.call_rec(xrec, residual=r, want_f32=False, want_rec=True, family=fam)                         # _f16s: raw split record out
        torch.cuda.synchronize()
    x3 = E.rec_from_f32(x, coef)
    three, yrec3 = pc.call_rec(x3, residual=r, want_f32=True, want_rec=True, rec_coef=ycoef, family=fam)
    _check_exact(f"record conv {family} {(B, cin, cout, H, W, res)}", y, three, _ref(operand, conv, r))
    assert torch.equal(y, y2), "the fp32 output depends on the record output's form"
    assert yrec.fmt == E.REC_F16 and yraw.fmt == E.REC_BF16X2
    assert _rel(yraw.to_f32(), y) < 2.0 ** -15
    # the record output: fp16_rn of the activated fp32 output.  Own error: the split record the SAME activation code writes from the same y.
    with E.precision(E.PRECISION_BF16X3):
        split_of_y = E.rec_from_f32(y, ycoef).to_f32()
    _check_fp16_record(f"record output {family} {(B, cin, cout, H, W)}", yrec.to_f32(), split_of_y, y, ycoef)
    assert yrec3.fmt == E.REC_BF16X2


@pytest.mark.parametrize("B,cin,cout,H,W,res", [(1, 256, 256, 37, 61, True), (2, 128, 128, 33, 40, False)])
def test_record_conv_statistics_epilogue_fp16(plugin, cuda, B, cin, cout, H, W, res):
    """k_conv3x3_rec_f16_st: the fp16 MFMAs with the GroupNorm statistics of the output in the epilogue."""
    E = plugin.engine
    conv, x, r, coef, pc = _conv_setup(cuda, E, B, cin, cout, H, W, res, 5 * cin + H)
    assert pc.leaves_stats(32, False, rec=True)
    with E.precision(E.PRECISION_F16):
        xrec = E.rec_from_f32(x, coef)
        operand = xrec.to_f32()
        y, (var, mean) = pc.call_rec_stats(xrec, residual=r, family=E.CONV_REC_ONE_BLOCK)
        torch.cuda.synchronize()
    three, _ = pc.call_rec_stats(E.rec_from_f32(x, coef), residual=r, family=E.CONV_REC_ONE_BLOCK)
    _check_exact(f"record conv + statistics {(B, cin, cout, H, W)}", y, three, _ref(operand, conv, r))
    v_ref, m_ref = vo.get_var_mean(y.double(), 32)
    assert _rel(mean, m_ref) < 1e-5 and _rel(var, v_ref) < 1e-5


def test_record_conv_out_fp16(plugin, cuda):
    """conv_out (3 couts) behind norm_out: k_conv3x3_rec_f16s<1, 1, 2>."""
    E = plugin.engine
    conv, x, _, coef, pc = _conv_setup(cuda, E, 1, 128, 3, 40, 70, False, 11)
    with E.precision(E.PRECISION_F16):
        xrec = E.rec_from_f32(x, coef)
        operand = xrec.to_f32()
        y = pc.call_rec(xrec, want_f32=True)[0]
        torch.cuda.synchronize()
    three = pc.call_rec(E.rec_from_f32(x, coef), want_f32=True)[0]
    _check_exact("record conv_out", y, three, _ref(operand, conv, None))


@pytest.mark.parametrize("B,cin,cout,H,W,res,stats", [(1, 512, 512, 33, 47, True, False), (2, 256, 128, 20, 70, False, False), (1, 128, 64, 18, 40, False, False),
                                                      (1, 256, 256, 24, 40, True, True)])
def test_fp32_handover_conv_with_pre_gn_fp16(plugin, cuda, B, cin, cout, H, W, res, stats):
    """k_conv3x3_f16<4, true>, <2, true> and the statistics form: fp32 input, activated and rounded to fp16 while staging.  The operand the kernel
    sees is the record producer's (the same fp32 activation code, the same conversion), read back through to_f32()."""
    E = plugin.engine
    conv, x, r, coef, pc = _conv_setup(cuda, E, B, cin, cout, H, W, res, cin + W)
    assert pc.fuses_pre_gn()
    with E.precision(E.PRECISION_F16):
        operand = E.rec_from_f32(x, coef).to_f32() if cin % 32 == 0 else None
        if stats:
            y, (var, mean) = pc.call_stats(x, coef, residual=r)
        else:
            y = pc(x, residual=r, pre_gn=coef)
        torch.cuda.synchronize()
    three = pc.call_stats(x, coef, residual=r)[0] if stats else pc(x, residual=r, pre_gn=coef)
    _check_exact(f"fp32 hand-over conv + pre_gn {(B, cin, cout, H, W, res, stats)}", y, three, _ref(operand, conv, r))
    if stats:
        v_ref, m_ref = vo.get_var_mean(y.double(), 32)
        assert _rel(mean, m_ref) < 1e-5 and _rel(var, v_ref) < 1e-5


def test_unproven_operands_keep_the_three_term_kernels_bit_for_bit(plugin, cuda):
    """Mode 5 with a raw record, a bf16-split activated record, no pre_gn, a 1x1 conv outside the attention or the stride-2 conv: the BF16X3 result."""
    E = plugin.engine
    conv, x, r, coef, pc = _conv_setup(cuda, E, 2, 256, 128, 40, 36, True, 77)
    raw, act3 = E.rec_from_f32(x), E.rec_from_f32(x, coef)
    c1 = torch.nn.Conv2d(256, 128, 1).to(cuda)
    p1 = E.PackedConv(c1.weight.detach(), c1.bias.detach())
    cd = torch.nn.Conv2d(256, 256, 3, 2, 0).to(cuda)
    pd = E.PackedConv(cd.weight.detach(), cd.bias.detach())

    def run():
        return [pc.call_rec(raw, residual=r, want_f32=True)[0], pc.call_rec(act3, residual=r, want_f32=True)[0], pc(x, residual=r), p1(x, residual=r),
                pd.down2(x), pc.call_rec(raw, want_f32=False, want_rec=True)[1].to_f32()]

    base = run()
    with E.precision(E.PRECISION_F16):
        got = run()
        torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(got, base)):
        assert torch.equal(a, b), f"call {i} differs from BF16X3 in mode 5"


@pytest.mark.parametrize("H,W", [(64, 64), (10, 12)], ids=["stream_kernel", "small_kernel"])
def test_attn_proj_flag_only_matters_in_mode_5(plugin, cuda, H, W):
    """MDTILE_CONV_ATTN_PROJ on a 1x1 conv: no effect in BF16X3, F32 and BF16; in mode 5 the flagged conv is mode 2's (one-term bf16, the attention's
    arithmetic) and the unflagged one BF16X3's (three terms: nin_shortcut reads the raw stream)."""
    E = plugin.engine
    torch.manual_seed(H)
    c = torch.nn.Conv2d(512, 512, 1).to(cuda)
    plain = E.PackedConv(c.weight.detach(), c.bias.detach())
    proj = E.PackedConv(c.weight.detach(), c.bias.detach(), attn_proj=True)
    x, r = torch.randn(1, 512, H, W, device=cuda), torch.randn(1, 512, H, W, device=cuda)
    out = {}
    for mode in (E.PRECISION_BF16X3, E.PRECISION_F32, E.PRECISION_BF16, E.PRECISION_F16):
        with E.precision(mode):
            out[mode] = (plain(x, residual=r), proj(x, residual=r))
            torch.cuda.synchronize()
    for mode in (E.PRECISION_BF16X3, E.PRECISION_F32, E.PRECISION_BF16):
        assert torch.equal(*out[mode]), f"the flag changed a 1x1 conv in mode {mode}"
    assert not torch.equal(out[E.PRECISION_BF16X3][0], out[E.PRECISION_BF16][0])
    assert torch.equal(out[E.PRECISION_F16][0], out[E.PRECISION_BF16X3][0]) and torch.equal(out[E.PRECISION_F16][1], out[E.PRECISION_BF16][1])


@pytest.mark.parametrize("how", ["one_block", "two_blocks", "window_one_block", "window_two_blocks"])
def test_upsample_conv_in_mode_5(plugin, cuda, how):
    """k_upconv_rec_o16 / k_upconv_rec2_o16: three-term MFMAs on the raw record (fp32 output bit-equal to BF16X3), activated record output in fp16."""
    E = plugin.engine
    torch.manual_seed(12)
    B, cin, cout, Hin, Win = 2, 256, 128, 30, 44
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1)
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    xr = E.rec_from_f32(torch.randn(B, cin, Hin, Win).to(cuda))
    ycoef = _coef(B, cout, 9).to(cuda)
    kw = dict(upsample2x=True, want_f32=True, want_rec=True, rec_coef=ycoef, family=E.CONV_REC_ONE_BLOCK if "one" in how else E.CONV_REC_TWO_BLOCKS)
    if "window" in how:
        kw["window"] = (3, 5, 20, 33)
    y3, yrec3 = pc.call_rec(xr, **kw)
    with E.precision(E.PRECISION_F16):
        y, yrec = pc.call_rec(xr, **kw)
        yraw = pc.call_rec(xr, **{**kw, "rec_coef": None})[1]
        torch.cuda.synchronize()
    assert torch.equal(y, y3), "the upsample conv's fp32 output is not the BF16X3 one"
    assert yrec.fmt == E.REC_F16 and yrec3.fmt == E.REC_BF16X2 and yraw.fmt == E.REC_BF16X2
    _check_fp16_record(f"upsample conv {how}", yrec.to_f32(), yrec3.to_f32(), y, ycoef)
    r = yrec.records()[:, 0]
    assert not r[:, :, 0].any() and not r[:, :, -1].any() and not r[:, :, :, 0].any() and not r[:, :, :, -1].any()


def test_fp16_subnormal_weights_are_multiplied_not_flushed(plugin, cuda):
    """Does v_mfma_f32_32x32x16_f16 keep subnormal A / B operands?  One conv whose weights all lie below 2^-14 (fp16's smallest normal), no bias:
    flushed operands would give exactly zero.  Found on an MI355X: kept (max |y| = 8.306e-4 = max |reference|, 4.85e-7 of the range apart, record and
    hand-over kernel alike) -- the header says so and the references here use the unflushed fp16_rn(w)."""
    E = plugin.engine
    torch.manual_seed(4)
    conv = torch.nn.Conv2d(128, 128, 3, 1, 1)
    with torch.no_grad():
        conv.weight.copy_(torch.randn_like(conv.weight) * 2.0 ** -17)
        conv.bias.zero_()
    assert conv.weight.abs().max().item() < 2.0 ** -14
    x, coef = torch.randn(1, 128, 24, 40, device=cuda), _coef(1, 128, 6).to(cuda)
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    with E.precision(E.PRECISION_F16):
        xrec = E.rec_from_f32(x, coef)
        operand = xrec.to_f32()
        y = pc.call_rec(xrec, want_f32=True)[0]
        yh = pc(x, pre_gn=coef)
        torch.cuda.synchronize()
    kept = _ref(operand, conv, None)
    e_kept, e_h = _rel(y, kept), _rel(yh, kept)
    print(f"fp16 subnormal weights: record kernel vs the unflushed reference {e_kept:.2e} (hand-over kernel {e_h:.2e}); max |y| {y.abs().max().item():.3e}, "
          f"max |reference| {kept.abs().max().item():.3e} (flushed operands would give 0)")
    assert y.abs().max().item() > 0.0, "subnormal fp16 operands were flushed to zero"
    assert e_kept < TOL_EXACT and e_h < TOL_EXACT


# ---------------------------------------------------------------------------------------------------------------- end to end
def _end_to_end(plugin, cuda, net_fn, x, tile, fast, is_decoder, color_fix, name, half_oracle=True):
    E = plugin.engine
    net = net_fn().to(cuda)
    ref = gr.tiled_forward_gpu(net, x, tile, fast, is_decoder=is_decoder, color_fix=color_fix).float().cpu()
    assert torch.isfinite(ref).all(), f"{name}: the fp32 oracle is not finite"
    e16 = float("nan")
    if half_oracle:
        ref16 = gr.tiled_forward_gpu(net_fn().to(cuda).half(), x.half(), tile, fast, is_decoder=is_decoder, color_fix=color_fix).float().cpu()
        e16 = _rel(ref16, ref) if torch.isfinite(ref16).all() else float("inf")
    net.original_forward = net.forward
    hook = plugin.tilevae.VAEHook(net, tile, is_decoder=is_decoder, fast_decoder=fast, fast_encoder=fast, color_fix=color_fix)
    with E.precision(E.PRECISION_BF16):
        out2 = hook(x.to(cuda)).float().cpu()
    with E.precision(E.PRECISION_F16):
        out5 = hook(x.to(cuda)).float().cpu()
    out3 = hook(x.to(cuda)).float().cpu()
    assert out5.shape == ref.shape
    e2, e5, e3 = _rel(out2, ref), _rel(out5, ref), _rel(out3, ref)
    print(f"{name}: vs fp32 oracle -- F16 mode {e5:.2e} (rel L2 {_rel_l2(out5, ref):.2e}), BF16 mode {e2:.2e} (rel L2 {_rel_l2(out2, ref):.2e}), "
          f"ratio {e2 / max(e5, 1e-30):.2f}, torch float16 oracle {e16:.2e}, BF16X3 {e3:.2e}")
    assert torch.isfinite(out5).all(), f"{name}: NaN / Inf in mode 5"
    assert e5 <= 0.5 * e2, f"{name}: mode 5 ({e5}) is not within half of mode 2's error ({e2})"
    assert e5 > e3, f"{name}: mode 5 is not the arithmetic that ran (as close to fp32 as BF16X3)"


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "slow"])
@pytest.mark.parametrize("stress", [False, 8], ids=["default", "stress"])
def test_decode_end_to_end(plugin, cuda, fast, stress):
    """Full-width SD decoder, 96x96 latent, decoder tile 64 (the geometry of tests/test_gpu_precision_bf16.py).
    Measured on an MI355X (error against the fp32 oracle, F16 / BF16): fast 1.77e-3 / 1.57e-2, slow 1.81e-3 / 1.65e-2, fast stress 1.56e-3 / 1.03e-2,
    slow stress 2.06e-3 / 9.7e-3 (the whole table: DESIGN.md section 3.8)."""
    torch.manual_seed(21)
    z = torch.randn(1, 4, 96, 96)
    with torch.no_grad():
        _end_to_end(plugin, cuda, lambda: ld.make_decoder(7, stress=stress), z, 64, fast, True, False, f"decode fast={fast} stress={stress}")


@pytest.mark.parametrize("fast,color_fix", [(True, False), (True, True), (False, False)], ids=["fast", "fast_colorfix", "slow"])
@pytest.mark.parametrize("stress", [False, 8], ids=["default", "stress"])
def test_encode_end_to_end(plugin, cuda, fast, color_fix, stress):
    """Full-width encoder, 168 x 136 image, encoder tile 64."""
    torch.manual_seed(5)
    x = torch.randn(1, 3, 168, 136)
    with torch.no_grad():
        _end_to_end(plugin, cuda, lambda: ld.make_encoder(7, stress=stress), x, 64, fast, False, color_fix,
                    f"encode fast={fast} color_fix={color_fix} stress={stress}")


def _scaled(make):
    def fn():
        net = make(7)
        with torch.no_grad():
            net.conv_in.weight.mul_(3.0e4)
            net.conv_in.bias.mul_(3.0e4)
        return net
    return fn


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "slow"])
@pytest.mark.parametrize("which", ["decoder", "encoder"])
def test_range_safety_with_the_stream_beyond_fp16(plugin, cuda, which, fast):
    """conv_in scaled by 3e4: the residual stream passes 65504 (checked below on the eager net).  The fp32 oracle stays finite; mode 5 keeps fp16 off
    the stream, so it must stay finite and within half of mode 2's error.  (The torch-float16 oracle overflows here by construction: not run.)"""
    torch.manual_seed(21 if which == "decoder" else 5)
    x = torch.randn(1, 4, 96, 96) if which == "decoder" else torch.randn(1, 3, 168, 136)
    make = _scaled(ld.make_decoder if which == "decoder" else ld.make_encoder)
    with torch.no_grad():
        assert make().conv_in(x[:, :, :32, :32]).abs().max().item() > 65504.0
        # fast: frozen statistics, record chain; slow: pooled statistics -- the conversion pass and the hand-over conv are the fp16 producers there
        _end_to_end(plugin, cuda, make, x, 64, fast, which == "decoder", False, f"range safety {which} fast={fast}", half_oracle=False)


# ---------------------------------------------------------------------------------------------------------------- stability
def _decoder_hook(plugin, cuda):
    dec = ld.make_decoder(7).to(cuda)
    dec.original_forward = dec.forward
    hook = plugin.tilevae.VAEHook(dec, 64, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
    torch.manual_seed(21)
    return hook, torch.randn(1, 4, 96, 96, device=cuda)


def test_mode_5_decode_is_bit_stable_and_device_slots_agree(plugin, cuda):
    E = plugin.engine
    hook, z = _decoder_hook(plugin, cuda)
    with torch.no_grad(), E.precision(E.PRECISION_F16):
        a = hook(z).clone()
        b = hook(z).clone()
        hook.devices = [0, 0]
        c = hook(z).clone()
        hook.devices = None
        torch.cuda.synchronize()
    assert torch.equal(a, b), "two mode-5 decodes differ"
    assert torch.equal(a, c), "a mode-5 decode through devices = [0, 0] differs from one device"


def test_mode_5_decode_is_bit_stable_next_to_mfma_kernels(plugin, cuda):
    """A mode-5 tiled decode while a side stream runs hand-over convs (MFMA kernels sharing the CUs): bit-identical to the decode alone."""
    E, dev = plugin.engine, cuda
    torch.manual_seed(3)
    c512 = torch.nn.Conv2d(512, 512, 3, padding=1).to(dev)
    p512 = E.PackedConv(c512.weight.detach(), c512.bias.detach())
    xs = torch.randn(2, 512, 200, 200, device=dev)
    k512 = _coef(2, 512, 1).to(dev)
    hook, z = _decoder_hook(plugin, cuda)
    side = torch.cuda.Stream()
    bad = 0
    with torch.no_grad(), E.precision(E.PRECISION_F16):
        p512(xs, pre_gn=k512)                      # (the fp16 plane is built here, not on the side stream)
        alone = hook(z).clone()
        torch.cuda.synchronize()
        for _ in range(3):
            with torch.cuda.stream(side):
                for _ in range(6):
                    p512(xs, pre_gn=k512)
            y = hook(z)
            side.synchronize()
            torch.cuda.synchronize()
            bad += int(not torch.equal(y, alone))
    print(f"mode-5 decode overlapped with hand-over convs on a side stream: {bad} of 3 runs differ from the decode alone")
    assert bad == 0
