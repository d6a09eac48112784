"""MDTILE_PRECISION_BF16 on the GPU: every one-term kernel against its exact contract, the tiled VAE end to end, and co-residency.

Contract of the mode: each matrix-core product is bf16_rn(a) x bf16_rn(b) (the hi halves the packers and splitters already produce),
accumulated in fp32; everything else (residual, bias, GroupNorm statistics, softmax, conv_in) stays fp32.
  * per kernel: an fp64 reference on bf16_rn-rounded operands (for the upsample convs: the merged sub-pixel weights the packer rounds);
    the tolerance is fp32 accumulation order (<= 2e-5 of the output range).
    Each result must also be much further from that reference in the default BF16X3 mode: the lo terms are really gone.
  * end to end: the error against the fp32 oracle must be no larger than that of the same oracle run with the decoder / encoder and the
    input cast to torch.bfloat16 (upstream's own path at dtype_vae = bfloat16), under an absolute ceiling, with no NaN / Inf.
Every test leaves the default mode behind (mdtile.precision restores it)."""
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


def _bf(t: torch.Tensor) -> torch.Tensor:
    """bf16_rn, as the packers (__bf16 conversion) and split8r / split8c / split8v round, widened to fp64."""
    return t.detach().float().to(torch.bfloat16).to(torch.float64)


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


def _rel_l2(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _both(E, fn):
    """fn() in mode 2 and in the default mode"""
    with E.precision(E.PRECISION_BF16):
        one = fn()
        torch.cuda.synchronize()
    three = fn()
    torch.cuda.synchronize()
    return one, three


def _check_exact(name, one, three, ref):
    e1, e3 = _rel(one, ref), _rel(three, ref)
    print(f"{name}: one-term vs bf16-operand fp64 reference {e1:.2e}, bf16x3 {e3:.2e}")
    assert torch.isfinite(one).all()
    assert e1 < TOL_EXACT, f"{name}: one-term kernel off its contract: rel err {e1}"
    assert e3 > 10 * max(e1, 1e-7), f"{name}: the default mode is as close to the bf16-operand reference ({e3}) as mode 2 ({e1})"


REC_CASES = [  # B, cin, cout, H, W (output), upsample, residual
    (1, 128, 128, 16, 32, False, False),     # exactly one block
    (1, 128, 128, 17, 45, False, True),      # ragged rows and columns
    (2, 256, 128, 40, 36, False, True),      # batch 2, 16 K-steps
    (1, 512, 512, 24, 40, False, False),     # 4 cout blocks
    (1, 128, 128, 32, 48, True, False),      # sub-pixel upsample, NK = 8
    (2, 256, 128, 40, 36, True, True),       # upsample + residual + batch
]


def _up_conv_ref(x, weight, bias):
    """fp64 reference of nearest-2x + 3x3 conv in the kernels' sub-pixel form: output parity (a, b) is a 2x2 conv of the input whose
    weights are the fp32 sums of the 3x3 taps that land on the same input pixel (k_upconv_pack_bf16x3: summed in (dy, dx) order, then
    split) -- the one-term product is bf16_rn(merged weight) x bf16_rn(x), not a sum of rounded taps."""
    w = weight.detach().float()
    taps = {(0, 0): (0, 1), (0, 1): (1, 3), (1, 0): (0, 2), (1, 1): (2, 3)}     # (parity, tap) -> [lo, hi) over the 3x3 index
    xp = F.pad(_bf(x), (1, 1, 1, 1))
    B, _, H, W = x.shape
    out = torch.empty(B, w.shape[0], 2 * H, 2 * W, dtype=torch.float64)
    for a in (0, 1):
        for b in (0, 1):
            wm = torch.empty(w.shape[0], w.shape[1], 2, 2)
            for u in (0, 1):
                for v in (0, 1):
                    s = torch.zeros(w.shape[0], w.shape[1])
                    for dy in range(*taps[(a, u)]):
                        for dx in range(*taps[(b, v)]):
                            s = s + w[:, :, dy, dx]            # fp32, the packer's order
                    wm[:, :, u, v] = s
            out[:, :, a::2, b::2] = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], _bf(wm), bias.detach().double())
    return out


def _rec_setup(cuda, B, cin, cout, H, W, up, res, seed):
    torch.manual_seed(seed)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1)
    hin, win = (H // 2, W // 2) if up else (H, W)
    x = torch.randn(B, cin, hin, win)
    r = torch.randn(B, cout, H, W) if res else None
    ref = _up_conv_ref(x, conv.weight, conv.bias) if up else F.conv2d(_bf(x), _bf(conv.weight), conv.bias.detach().double(), padding=1)
    if res:
        ref = ref + r.double()
    return conv, x, r, ref


@pytest.mark.parametrize("family", ["one_block", "two_blocks"])
@pytest.mark.parametrize("B,cin,cout,H,W,up,res", REC_CASES)
def test_record_conv_one_term(plugin, cuda, B, cin, cout, H, W, up, res, family):
    """k_conv3x3_rec1t / k_upconv_rec1t (one block per CU) and k_conv3x3_rec2_1t / k_upconv_rec2_1t (two blocks per CU)."""
    E = plugin.engine
    conv, x, r, ref = _rec_setup(cuda, B, cin, cout, H, W, up, res, cin + 7 * cout + H)
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    xrec = E.rec_from_f32(x.to(cuda))
    rr = None if r is None else r.to(cuda)
    fam = E.CONV_REC_ONE_BLOCK if family == "one_block" else E.CONV_REC_TWO_BLOCKS
    one, three = _both(E, lambda: pc.call_rec(xrec, residual=rr, upsample2x=up, want_f32=True, family=fam)[0])
    _check_exact(f"record conv {family} {(B, cin, cout, H, W, up, res)}", one, three, ref)
    # the record output of the one-term kernel still carries both planes: hi + lo of the same fp32 values
    with E.precision(E.PRECISION_BF16):
        y, yrec = pc.call_rec(xrec, residual=rr, upsample2x=up, want_f32=True, want_rec=True, family=fam)
    assert _rel(yrec.to_f32(), y) < 2.0 ** -15


@pytest.mark.parametrize("B,cin,cout,H,W,up,res", [(1, 256, 256, 37, 61, False, True), (2, 128, 128, 32, 48, True, False)])
def test_record_conv_statistics_epilogue_one_term(plugin, cuda, B, cin, cout, H, W, up, res):
    """k_conv3x3_rec1t_st / k_upconv_rec1t_st: the one-term MFMAs with the GroupNorm statistics of the output in the epilogue."""
    E = plugin.engine
    conv, x, r, ref = _rec_setup(cuda, B, cin, cout, H, W, up, res, 5 * cin + H)
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    assert pc.leaves_stats(32, up, rec=True)
    xrec = E.rec_from_f32(x.to(cuda))
    rr = None if r is None else r.to(cuda)
    with E.precision(E.PRECISION_BF16):
        y, (var, mean) = pc.call_rec_stats(xrec, residual=rr, upsample2x=up)
        torch.cuda.synchronize()
    three, _ = pc.call_rec_stats(xrec, residual=rr, upsample2x=up)
    _check_exact(f"record conv + statistics {(B, cin, cout, H, W, up)}", y, three, ref)
    v_ref, m_ref = vo.get_var_mean(y.double(), 32)
    assert _rel(mean, m_ref) < 1e-5 and _rel(var, v_ref) < 1e-5


def test_record_conv_out_one_term(plugin, cuda):
    """conv_out (3 couts): k_conv3x3_rec1t<1, 1, 2>."""
    E = plugin.engine
    torch.manual_seed(11)
    conv = torch.nn.Conv2d(128, 3, 3, 1, 1)
    x = torch.randn(1, 128, 40, 70)
    ref = F.conv2d(_bf(x), _bf(conv.weight), conv.bias.detach().double(), padding=1)
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    xrec = E.rec_from_f32(x.to(cuda))
    one, three = _both(E, lambda: pc.call_rec(xrec, want_f32=True)[0])
    _check_exact("record conv_out", one, three, ref)


@pytest.mark.parametrize("blocks", ["one_block", "two_blocks"])
def test_upconv_window_one_term(plugin, cuda, blocks):
    E = plugin.engine
    torch.manual_seed(12)
    B, cin, cout, Hin, Win = 2, 256, 128, 30, 44
    win = (3, 5, 20, 33)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1)
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    x = torch.randn(B, cin, Hin, Win)
    xr = E.rec_from_f32(x.to(cuda))
    y0, x0, h, w = win
    ref = _up_conv_ref(x, conv.weight, conv.bias)[:, :, 2 * y0:2 * (y0 + h), 2 * x0:2 * (x0 + w)]
    fam = E.CONV_REC_ONE_BLOCK if blocks == "one_block" else E.CONV_REC_TWO_BLOCKS
    one, three = _both(E, lambda: pc.call_rec(xr, upsample2x=True, want_f32=True, window=win, family=fam)[0])
    _check_exact(f"upconv window ({blocks})", one, three, ref)


@pytest.mark.parametrize("B,cin,cout,H,W,up", [(1, 512, 512, 33, 47, False), (2, 256, 128, 20, 70, False), (1, 128, 256, 18, 40, True),
                                               (1, 512, 512, 21, 33, True),
                                               (2, 32, 64, 9, 33, False),       # 64-cout blocks (k_conv3x3_bf16x1<2, false>): two K-steps, ragged tiles, batch 2
                                               (2, 32, 64, 9, 33, True)])       # 64-cout blocks of the sub-pixel kernel (k_upconv_bf16x1<2>): 9 x 33 -> 18 x 66
def test_fp32_handover_conv_one_term(plugin, cuda, B, cin, cout, H, W, up):
    """k_conv3x3_bf16x1 / k_upconv_bf16x1: fp32 input, split while staging, hi half only.  (H, W: the INPUT size.)"""
    E = plugin.engine
    torch.manual_seed(cin + W)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1)
    x = torch.randn(B, cin, H, W)
    ref = _up_conv_ref(x, conv.weight, conv.bias) if up else F.conv2d(_bf(x), _bf(conv.weight), conv.bias.detach().double(), padding=1)
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    xd = x.to(cuda)
    one, three = _both(E, lambda: pc(xd, upsample2x=up))
    _check_exact(f"fp32 hand-over conv {(B, cin, cout, H, W, up)}", one, three, ref)


def _coef(B, C, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.rand(B, 1, C, generator=g) * 1.5 + 0.25, torch.randn(B, 1, C, generator=g) * 0.5], dim=1).contiguous()


def _activated_hi(E, x, coef):
    """bf16_rn(silu(a x + s)) exactly as the kernels round it: the hi plane of the activated record image (rec_from_f32 runs the same fp32
    activation code as the fused staging), read out by a one-term record conv with unit weights -- 1.0 x hi and nothing else per output."""
    C = x.shape[1]
    w = torch.zeros(128, C, 3, 3, device=x.device)
    w[torch.arange(C), torch.arange(C), 1, 1] = 1.0
    ident = E.PackedConv(w, torch.zeros(128, device=x.device))
    with E.precision(E.PRECISION_BF16):
        hi = ident.call_rec(E.rec_from_f32(x, coef), want_f32=True)[0][:, :C]
        torch.cuda.synchronize()
    assert torch.equal(hi, hi.to(torch.bfloat16).float())
    return hi


@pytest.mark.parametrize("B,cin,cout,H,W,res,stats", [(2, 32, 128, 9, 33, True, False),      # k_conv3x3_bf16x1<4, true>
                                                      (1, 32, 64, 9, 33, False, False),      # <2, true>: 64-cout blocks
                                                      (1, 32, 128, 9, 33, True, True)])      # <4, true, 1, true>: statistics in the epilogue
def test_fp32_handover_conv_with_pre_gn_one_term(plugin, cuda, B, cin, cout, H, W, res, stats):
    """The fused GroupNorm + SiLU forms of k_conv3x3_bf16x1: fp32 input, activated in fp32 and rounded to bf16 while staging."""
    E = plugin.engine
    torch.manual_seed(cin + cout + W)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1)
    x, coef = torch.randn(B, cin, H, W).to(cuda), _coef(B, cin, cout + 1).to(cuda)
    r = torch.randn(B, cout, H, W).to(cuda) if res else None
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    assert pc.fuses_pre_gn() and (not stats or pc.leaves_stats(32))
    ref = F.conv2d(_activated_hi(E, x, coef).double().cpu(), _bf(conv.weight), conv.bias.detach().double(), padding=1)
    if res:
        ref = ref + r.double().cpu()
    with E.precision(E.PRECISION_BF16):
        if stats:
            one, (var, mean) = pc.call_stats(x, coef, residual=r)
        else:
            one = pc(x, residual=r, pre_gn=coef)
        torch.cuda.synchronize()
    three = pc.call_stats(x, coef, residual=r)[0] if stats else pc(x, residual=r, pre_gn=coef)
    _check_exact(f"fp32 hand-over conv + pre_gn {(B, cin, cout, H, W, res, stats)}", one, three, ref)
    if stats:
        v_ref, m_ref = vo.get_var_mean(one.double(), 32)
        assert _rel(mean, m_ref) < 1e-5 and _rel(var, v_ref) < 1e-5


@pytest.mark.parametrize("B,cin,cout,H,W", [(1, 128, 128, 64, 90), (1, 256, 256, 41, 57), (2, 512, 512, 32, 32),
                                            (2, 32, 64, 19, 67)])      # 64-cout blocks (k_conv3x3_bf16x1<2, false, 2>): 19 x 67 -> 9 x 33, batch 2
def test_stride2_conv_one_term(plugin, cuda, B, cin, cout, H, W):
    E = plugin.engine
    torch.manual_seed(cin + H)
    conv = torch.nn.Conv2d(cin, cout, 3, 2, 0)
    x = torch.randn(B, cin, H, W)
    ref = F.conv2d(F.pad(_bf(x), (0, 1, 0, 1)), _bf(conv.weight), conv.bias.detach().double(), stride=2)
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    xd = x.to(cuda)
    one, three = _both(E, lambda: pc.down2(xd))
    _check_exact(f"stride-2 conv {(B, cin, cout, H, W)}", one, three, ref)


@pytest.mark.parametrize("B,cin,cout,H,W,res", [(1, 512, 512, 64, 64, True), (1, 256, 128, 48, 48, False), (2, 128, 256, 40, 60, True),
                                                (1, 256, 128, 10, 12, False),
                                                (1, 64, 256, 5, 7, True),        # small-image kernel, 256-cout blocks (k_conv1x1_bf16x1<8, 256>), ragged pixel tile
                                                (2, 64, 64, 5, 7, False)])       # ... 64-cout blocks (<2, 256>), batch 2
def test_conv1x1_one_term(plugin, cuda, B, cin, cout, H, W, res):
    """k_conv1x1_stream1t (HW >= 2048) and k_conv1x1_bf16x1 (the small-image kernel)."""
    E = plugin.engine
    torch.manual_seed(cin + cout + H)
    conv = torch.nn.Conv2d(cin, cout, 1)
    x = torch.randn(B, cin, H, W)
    r = torch.randn(B, cout, H, W) if res else None
    ref = F.conv2d(_bf(x), _bf(conv.weight), conv.bias.detach().double())
    if res:
        ref = ref + r.double()
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    xd, rd = x.to(cuda), None if r is None else r.to(cuda)
    one, three = _both(E, lambda: pc(xd, residual=rd))
    _check_exact(f"1x1 conv {(B, cin, cout, H, W, res)}", one, three, ref)


def _attn_ref(q, k, v_tok, scale, round_p):
    """fp64 attention on bf16_rn operands.  round_p: P rounded to bf16 at the global row maximum (what the kernel does when the whole key
    range is one 128-key block)."""
    qb, kb, vb = _bf(q), _bf(k), _bf(v_tok)
    s = torch.einsum("bct,bcu->btu", qb, kb) * scale
    p = torch.exp(s - s.max(dim=2, keepdim=True).values)
    l = p.sum(dim=2, keepdim=True)
    if round_p:
        p = _bf(p)
    return torch.einsum("btu,buc->bct", p / l, vb)


@pytest.mark.parametrize("C", [128, 256, 512])
@pytest.mark.parametrize("T", [77, 128, 1000])
def test_attention_one_term(plugin, cuda, C, T):
    """k_attn_bf16x1: QK^T on K_hi x Q_hi, P.V on V_hi x P_hi, against fp64 on bf16 operands with P rounded at the row maximum (what the
    kernel does when the keys are one 128-key block; with several blocks it rounds at the running maximum of the online softmax).  Must
    sit well closer to that reference than BF16X3 does."""
    E = plugin.engine
    torch.manual_seed(C + T)
    B = 2
    q, k = torch.randn(B, C, T) * 1.5, torch.randn(B, C, T) * 1.5
    v = torch.randn(B, T, C)
    scale = C ** -0.5
    qd, kd, vd = q.to(cuda), k.to(cuda), v.to(cuda)
    one, three = _both(E, lambda: E.vae_attn(qd, kd, vd, scale))
    ref = _attn_ref(q, k, v, scale, round_p=True)
    e1, e3 = _rel(one, ref), _rel(three, ref)
    print(f"attention C={C} T={T}: one-term vs bf16-operand reference {e1:.2e}, bf16x3 {e3:.2e}")
    assert torch.isfinite(one).all()
    # P is rounded from fp32 scores / exp2 in the kernel: a P element within fp32 round-off of a bf16 rounding boundary may round the other
    # way (one bf16 ulp, 2^-8 of that weight) -- a few such elements per tensor; several key blocks add the running-maximum rounding
    tol = 3e-4 if T <= 128 else 2e-3
    assert e1 < tol and e1 < 0.5 * e3, (e1, e3)


# ---------------------------------------------------------------------------------------------------------------- end to end
CEIL = 3e-2


def _end_to_end(plugin, cuda, net_fn, x, tile, fast, is_decoder, color_fix, name):
    E = plugin.engine
    net = net_fn().to(cuda)
    ref = gr.tiled_forward_gpu(net, x, tile, fast, is_decoder=is_decoder, color_fix=color_fix).float().cpu()
    ref16 = gr.tiled_forward_gpu(net_fn().to(cuda).to(torch.bfloat16), x.to(torch.bfloat16), tile, fast, is_decoder=is_decoder,
                                 color_fix=color_fix).float().cpu()
    net.original_forward = net.forward
    hook = plugin.tilevae.VAEHook(net, tile, is_decoder=is_decoder, fast_decoder=fast, fast_encoder=fast, color_fix=color_fix)
    with E.precision(E.PRECISION_BF16):
        out = hook(x.to(cuda)).float().cpu()
    out3 = hook(x.to(cuda)).float().cpu()
    assert out.shape == ref.shape
    e1, e16, e3 = _rel(out, ref), _rel(ref16, ref), _rel(out3, ref)
    print(f"{name}: vs fp32 oracle -- BF16 mode {e1:.2e} (rel L2 {_rel_l2(out, ref):.2e}), bf16 oracle {e16:.2e} (rel L2 {_rel_l2(ref16, ref):.2e}), "
          f"BF16X3 {e3:.2e}")
    assert torch.isfinite(out).all(), f"{name}: NaN / Inf in mode 2"
    assert e1 <= e16, f"{name}: mode 2 ({e1}) is worse than upstream's own bf16 path ({e16})"
    assert e1 < CEIL, f"{name}: rel err {e1}"
    assert e1 > e3, f"{name}: mode 2 is not the arithmetic that ran (as close to fp32 as BF16X3)"


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "slow"])
@pytest.mark.parametrize("stress", [False, 8], ids=["default", "stress"])
def test_decode_end_to_end(plugin, cuda, fast, stress):
    """Full-width SD decoder, 96x96 latent, decoder tile 64 (the geometry of test_gpu_vae_large / test_gpu_vae_stress)."""
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


def test_mode_2_decode_is_bit_stable_next_to_mfma_kernels(plugin, cuda):
    """A mode-2 tiled decode while a side stream runs hand-over convs (MFMA kernels sharing the CUs): bit-identical to the decode alone."""
    E, dev = plugin.engine, cuda
    torch.manual_seed(3)
    c512 = torch.nn.Conv2d(512, 512, 3, padding=1).to(dev)
    p512 = E.PackedConv(c512.weight.detach(), c512.bias.detach())
    xs = torch.randn(2, 512, 200, 200, device=dev)
    g = torch.Generator().manual_seed(1)
    k512 = torch.cat([torch.rand(2, 1, 512, generator=g) * 1.5 + 0.25, torch.randn(2, 1, 512, generator=g) * 0.5], dim=1).contiguous().to(dev)
    dec = ld.make_decoder(7).to(dev)
    dec.original_forward = dec.forward
    hook = plugin.tilevae.VAEHook(dec, 64, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
    torch.manual_seed(21)
    z = torch.randn(1, 4, 96, 96, device=dev)
    side = torch.cuda.Stream()
    bad = 0
    with torch.no_grad(), E.precision(E.PRECISION_BF16):
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
    print(f"mode-2 decode overlapped with hand-over convs on a side stream: {bad} of 3 runs differ from the decode alone")
    assert bad == 0
