"""GPU parity of the Tiled-VAE kernels (GroupNorm statistics / apply+SiLU, MFMA conv, flash attention, crop+store, fast-mode
input) and of the whole tiled decode through the plugin's VAEHook, against the oracle and the upstream-generated goldens.
Tolerances (fp32 everywhere; summation order differs from eager torch): primitives <= 2e-5 relative, end-to-end decode
<= 1e-3 relative to the output's max (the BASELINE.json target), in practice ~1e-5."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hostsim import ldm_decoder as ld
from hostsim import stub_host as sh
from oracle import vae_oracle as vo

pytestmark = pytest.mark.gpu


def _rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return (a - b).abs().max().item() / max(b.abs().max().item(), 1e-30)


@pytest.mark.parametrize("shape", [(2, 64, 9, 13), (1, 128, 33, 47), (1, 512, 20, 28), (3, 32, 5, 7), (1, 256, 64, 64)])
def test_gn_stats_and_apply(plugin, cuda, shape):
    E = plugin.engine
    torch.manual_seed(11)
    t = torch.randn(*shape) * 3 + 0.5
    var_r, mean_r = vo.get_var_mean(t, 32)
    var, mean = E.gn_stats(t.to(cuda), 32)
    assert _rel(mean.cpu(), mean_r) < 1e-5 and _rel(var.cpu(), var_r) < 1e-5
    g, b = torch.randn(shape[1]), torch.randn(shape[1])
    for silu in (False, True):
        ref = vo.custom_group_norm(t, 32, mean_r, var_r, g, b)
        ref = F.silu(ref) if silu else ref
        out = E.gn_apply(t.to(cuda), mean_r.to(cuda), var_r.to(cuda), g.to(cuda), b.to(cuda), 32, 1e-6, silu)
        assert (out.cpu() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    out = E.gn_apply(t.to(cuda), mean_r.to(cuda), var_r.to(cuda), None, None, 32, 1e-6, False)
    assert (out.cpu() - vo.custom_group_norm(t, 32, mean_r, var_r)).abs().max().item() < 2e-5


def test_gn_golden(plugin, cuda, golden_vae):
    E = plugin.engine
    torch.manual_seed(11)
    t = torch.randn(2, 64, 9, 13) * 3 + 0.5
    g, b = torch.randn(64), torch.randn(64)
    var, mean = E.gn_stats(t.to(cuda), 32)
    assert np.allclose(var.cpu().numpy(), golden_vae["gn/var"], rtol=1e-5) and np.allclose(mean.cpu().numpy(), golden_vae["gn/mean"], rtol=1e-5, atol=1e-6)
    out = E.gn_apply(t.to(cuda), mean, var, g.to(cuda), b.to(cuda))
    assert np.allclose(out.cpu().numpy(), golden_vae["gn/out"], rtol=1e-4, atol=2e-5)


def test_gn_pool_silu_add(plugin, cuda):
    E = plugin.engine
    torch.manual_seed(1)
    vars_ = [torch.rand(64) + 0.1 for _ in range(5)]
    means = [torch.randn(64) for _ in range(5)]
    px = [86 * 86, 86 * 64, 64 * 86, 64 * 64, 70 * 70]
    v_r, m_r = vo.pool_stats(vars_, means, px)
    v, m = E.gn_pool(torch.vstack(means).to(cuda), torch.vstack(vars_).to(cuda), px)
    assert _rel(v.cpu(), v_r) < 1e-6 and _rel(m.cpu(), m_r) < 1e-6
    x = torch.randn(3, 7, 11, 13) * 4
    y = torch.randn(3, 7, 11, 13)
    assert (E.silu(x.to(cuda)).cpu() - F.silu(x)).abs().max().item() < 1e-6
    assert torch.equal(E.add(x.to(cuda), y.to(cuda)).cpu(), x + y)


CONV_CASES = [  # B, cin, cout, k, H, W, upsample, residual, token_major
    (1, 4, 128, 3, 20, 30, False, False, False),     # conv_in shape class (cin < slab)
    (2, 128, 128, 3, 17, 45, False, True, False),    # ragged tile edges + fused residual, batch 2
    (1, 64, 256, 1, 19, 33, False, False, False),    # nin_shortcut
    (1, 128, 3, 3, 24, 40, False, False, False),     # conv_out (narrow config, Cout=3)
    (1, 32, 32, 3, 16, 32, False, True, False),      # small-decoder widths
    (1, 96, 64, 3, 9, 70, False, False, False),
    (1, 128, 128, 3, 32, 48, True, False, False),    # fused nearest-2x upsample
    (1, 128, 128, 1, 13, 29, False, False, True),    # v projection, token-major output
    (1, 512, 512, 3, 24, 40, False, True, False),    # SD mid-block width
    (1, 512, 512, 1, 16, 24, False, False, True),
    (1, 256, 256, 3, 70, 100, False, True, False),   # many pixel tiles x 2 cout blocks (block -> XCD mapping)
    (2, 256, 128, 3, 40, 36, True, True, False),     # upsample + residual + batch, cout block of 128 from 256 cin
    (1, 48, 160, 3, 11, 33, False, False, False),    # cin = 3 K-steps, cout padded 160 -> 256
    (1, 512, 512, 3, 74, 100, True, False, False),   # sub-pixel upsample conv: ragged input tiles (37 x 50), 4 cout blocks
    (1, 64, 64, 3, 18, 66, True, True, False),       # sub-pixel upsample conv, 64-cout block variant + residual
    (1, 256, 256, 3, 50, 70, False, False, False),   # 16-row blocks (default for 128-cout blocks)
    (2, 512, 256, 1, 21, 37, False, True, False),    # split-bf16 1x1 (flat pixel run): nin_shortcut shape, batch 2, residual
    (1, 256, 128, 1, 40, 50, False, False, False),   # split-bf16 1x1, one cout block
    (1, 96, 64, 1, 17, 19, False, True, False),      # split-bf16 1x1, 64-cout block variant, 3 phases, ragged last pixel tile
    (1, 512, 512, 1, 31, 33, False, True, False),    # proj_out shape (+ the queue's residual add)
    (1, 32, 160, 1, 23, 29, False, True, False),     # split-bf16 1x1, ONE phase (no prefetch), 256-cout block variant with 160 real couts
    (1, 160, 320, 1, 10, 50, False, False, False),   # split-bf16 1x1, 5 phases (odd: the two-phase trip ends half way), 2 cout blocks of 256
    (1, 64, 128, 1, 48, 52, False, True, False),     # streaming 1x1 (H*W % 4 == 0, >= 2048 px, cout % 128 == 0): 4 K-steps, ragged last 512-px block, residual
    (2, 96, 256, 1, 50, 60, False, False, False),    # streaming 1x1: 6 K-steps (ring wraps twice), two cout blocks, batch 2
    (1, 32, 128, 1, 40, 52, False, True, False),     # streaming 1x1: exactly two K-steps (no steady-state issue)
    (1, 512, 128, 1, 64, 64, False, False, False),   # streaming 1x1: 32 K-steps
    (1, 64, 512, 1, 40, 64, False, True, False),     # streaming 1x1, 256-cout blocks x 2, residual
    (1, 64, 128, 1, 45, 47, False, True, False),     # H*W % 4 != 0: stays on the plain 1x1 kernel
    (1, 3, 128, 3, 37, 131, False, False, False),    # conv_in kernel (k_conv3x3_fewcin): the encoder's 3 -> 128, odd width (unpaired last pixel, odd plane size)
    (2, 4, 512, 3, 19, 260, False, True, False),     # conv_in kernel: the decoder's 4 -> 512 (four cout blocks), three column blocks, batch, residual
    (1, 3, 48, 3, 5, 2, False, False, False),        # conv_in kernel: fewer couts than a block, a 2-px-wide image
    (1, 4, 128, 3, 1, 1, False, False, False),       # conv_in kernel: one pixel
    (1, 3, 128, 3, 64, 129, False, True, False),     # conv_in kernel: odd row pitch (pairs only 8-byte aligned on every other row)
]


@pytest.mark.parametrize("exact", [False, True], ids=["bf16x3", "f32"])
@pytest.mark.parametrize("B,cin,cout,k,H,W,up,res,tok", CONV_CASES)
def test_conv2d_vs_torch(plugin, cuda, B, cin, cout, k, H, W, up, res, tok, exact):
    E = plugin.engine
    torch.manual_seed(cin * 7 + cout + k)
    conv = torch.nn.Conv2d(cin, cout, k, 1, k // 2)
    hin, win = (H // 2, W // 2) if up else (H, W)
    x = torch.randn(B, cin, hin, win)
    with torch.no_grad():
        ref = conv(F.interpolate(x, scale_factor=2.0, mode="nearest") if up else x)
        r = torch.randn_like(ref) if res else None
        if res:
            ref = ref + r
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    rr = None
    if res:
        rr = (r.permute(0, 2, 3, 1).reshape(B, H * W, cout) if tok else r).contiguous().to(cuda)
    out = pc(x.to(cuda), residual=rr, upsample2x=up, token_major=tok, exact=exact).cpu()
    if tok:
        out = out.view(B, H, W, cout).permute(0, 3, 1, 2)
    err = _rel(out, ref)
    # exact-fp32 MFMA kernel: fp32 round-off only.  Default path (3x3, cin % 16 == 0): split-bf16 operands, 16 significand
    # bits per factor, fp32 accumulation -> <= 1e-4 of the output range (the end-to-end budget is 1e-3).
    tol = 2e-5 if exact else 5e-5
    assert err < tol, f"conv rel err {err}; worst at {np.unravel_index((out - ref).abs().argmax().item(), ref.shape)}"


@pytest.mark.parametrize("B,cin,cout,H,W,res", [
    (1, 128, 128, 17, 45, True),     # ragged edges, 128-cout block
    (2, 512, 512, 24, 40, False),    # SD mid-block width, batch 2 (per-sample statistics)
    (1, 64, 32, 20, 33, True),       # 64-cout block variant
    (1, 256, 128, 9, 70, False),
])
def test_conv2d_fused_groupnorm_silu(plugin, cuda, B, cin, cout, H, W, res):
    """mdtile_conv2d_gn: y = conv(silu(groupnorm_fixed_stats(x))) (+ residual) with the norm + SiLU applied while the conv
    stages its input, against the unfused torch chain on given (not self-computed) statistics."""
    E = plugin.engine
    torch.manual_seed(cin + cout + H)
    conv = torch.nn.Conv2d(cin, cout, 3, 1, 1)
    x = torch.randn(B, cin, H, W) * 1.7 + 0.3
    mean = torch.randn(B * 32) * 0.2
    var = torch.rand(B * 32) * 2.0 + 0.3
    gamma, beta = torch.randn(cin) * 0.5 + 1.0, torch.randn(cin) * 0.3
    cpg = cin // 32
    with torch.no_grad():
        m = mean.view(B, 32, 1, 1, 1)
        v = var.view(B, 32, 1, 1, 1)
        xn = ((x.view(B, 32, cpg, H, W) - m) / torch.sqrt(v + 1e-6)).view(B, cin, H, W)
        xn = F.silu(xn * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1))
        ref = conv(xn)
        r = torch.randn_like(ref) if res else None
        if res:
            ref = ref + r
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    assert pc.fuses_pre_gn()
    coef = E.gn_coeffs(mean.to(cuda), var.to(cuda), gamma.to(cuda), beta.to(cuda), cin, 32, 1e-6)
    out = pc(x.to(cuda), residual=None if r is None else r.to(cuda), pre_gn=coef).cpu()
    err = _rel(out, ref)
    assert err < 5e-5, f"fused GN+SiLU conv rel err {err}"
    # and identical (to fp32 round-off of exp / rcp) to the engine's own unfused pair
    xa = E.gn_apply(x.to(cuda), mean.to(cuda), var.to(cuda), gamma.to(cuda), beta.to(cuda), 32, 1e-6, True)
    out2 = pc(xa, residual=None if r is None else r.to(cuda)).cpu()
    assert _rel(out, out2) < 2e-5


def test_tiled_decode_fused_norm_matches_unfused(plugin, cuda):
    dec = ld.make_decoder(3).to(cuda)
    dec.original_forward = dec.forward
    torch.manual_seed(9)
    z = torch.randn(1, 4, 30, 38).to(cuda)
    outs = {}
    old = plugin.tilevae.FUSE_PRE_GN
    try:
        for fuse in (True, False):
            plugin.tilevae.FUSE_PRE_GN = fuse
            for fast in (True, False):
                hook = plugin.tilevae.VAEHook(dec, 12, is_decoder=True, fast_decoder=fast, fast_encoder=False, color_fix=False)
                outs[(fuse, fast)] = hook(z).cpu()
    finally:
        plugin.tilevae.FUSE_PRE_GN = old
    for fast in (True, False):
        assert _rel(outs[(True, fast)], outs[(False, fast)]) < 5e-5


@pytest.mark.parametrize("exact", [False, True], ids=["bf16x3", "f32"])
@pytest.mark.parametrize("B,C,T", [(1, 512, 3000), (2, 256, 700), (1, 128, 64), (1, 128, 100), (2, 128, 200), (1, 256, 77), (1, 512, 150), (1, 512, 1000),
                                   (1, 512, 128), (2, 256, 513), (1, 128, 2050)])
def test_attention_vs_oracle(plugin, cuda, B, C, T, exact):
    E = plugin.engine
    torch.manual_seed(C + T)
    q, k, v = torch.randn(B, C, T), torch.randn(B, C, T) * 1.5, torch.randn(B, C, T)
    scale = float(int(C) ** (-0.5))
    w_ = torch.softmax(torch.bmm(q.permute(0, 2, 1), k) * scale, dim=2)          # attn.py:57-60
    ref = torch.bmm(v, w_.permute(0, 2, 1))                                        # attn.py:63-66
    out = E.vae_attn(q.to(cuda), k.to(cuda), v.permute(0, 2, 1).contiguous().to(cuda), scale, exact=exact).cpu()
    err = _rel(out, ref)
    # exact: fp32 MFMA.  Default: split-bf16 operands (16 significand bits per factor), fp32 accumulation + softmax.
    assert err < (2e-5 if exact else 5e-5), f"attention rel err {err}"


@pytest.mark.parametrize("exact", [False, True], ids=["bf16x3", "f32"])
@pytest.mark.parametrize("C,T,spike", [(128, 300, 4.0), (128, 300, 1.0), (512, 700, 2.5), (512, 700, 0.6), (256, 1500, 3.0)])
def test_attention_online_softmax_rescale_branch(plugin, cuda, exact, C, T, spike):
    """Force the running-max update late in the key sequence (a spike in the last key block) -- bounded random data alone
    never exercises a wrong rescale.  Both kernels take a key block's exponentials against the running maximum INCLUDING that block
    (m_new = max(m_run, m_blk)) and rescale acc_o and l_run by alpha = exp(m_run - m_new) in the same block; the split-bf16 kernel skips
    the multiply of acc_o for a wave whose queries all have alpha == 1.  A spike in a late block gives alpha << 1 there (0 for the
    large spikes: everything accumulated before is dropped), and the blocks behind T // 2 run with alpha == 1 again."""
    E = plugin.engine
    torch.manual_seed(0)
    B = 1
    q, k, v = torch.randn(B, C, T), torch.randn(B, C, T), torch.randn(B, C, T)
    k[:, :, T - 10] = q[:, :, 5] * spike      # query 5 matches a key of the last block very strongly
    k[:, :, T // 2] = q[:, :, 170] * spike * 0.8
    k[:, :, 3] = q[:, :, 170] * 3.0
    scale = float(C ** -0.5)
    w_ = torch.softmax(torch.bmm(q.permute(0, 2, 1), k) * scale, dim=2)
    ref = torch.bmm(v, w_.permute(0, 2, 1))
    out = E.vae_attn(q.to(cuda), k.to(cuda), v.permute(0, 2, 1).contiguous().to(cuda), scale, exact=exact).cpu()
    assert _rel(out, ref) < (2e-5 if exact else 5e-5)


def test_attn_block_golden(plugin, cuda, golden_vae):
    """q/k/v/proj_out 1x1 convs + attention core == upstream attn_forward on the golden AttnBlock (C=64 is below the
    kernel's 128-channel granule, so this one checks the convs and uses a 128-channel twin for the core)."""
    torch.manual_seed(12)
    ab = ld.AttnBlock(128).eval()
    hx = torch.randn(1, 128, 7, 9)
    with torch.no_grad():
        ref = vo.attn_body(ab, hx)
    pack = plugin.tilevae.AttnPack(ab.to(cuda))
    out = pack(hx.to(cuda), torch.zeros_like(hx).to(cuda)).cpu()
    assert _rel(out, ref) < 5e-5


def test_crop_store_and_fast_input(plugin, cuda):
    E = plugin.engine
    ins, outs = vo.split_tiles(40, 56, 16)
    result = torch.zeros(1, 3, 320, 448, device=cuda)
    ref = torch.zeros(1, 3, 320, 448)
    torch.manual_seed(0)
    for ib, ob in zip(ins, outs):
        tile = torch.randn(1, 3, (ib[3] - ib[2]) * 8, (ib[1] - ib[0]) * 8)
        E.crop_store(tile.to(cuda), ib, ob, result)
        ref[:, :, ob[2]:ob[3], ob[0]:ob[1]] = vo.crop_valid_region(tile, ib, ob)
    assert torch.equal(result.cpu(), ref)
    for (H, W, ts) in [(40, 56, 16), (128, 128, 64), (30, 70, 24), (97, 61, 32)]:
        torch.manual_seed(H)
        z = torch.randn(2, 4, H, W) * 1.7 + 0.3
        got = E.vae_fast_input(z.to(cuda), ts).cpu()
        ref = vo.fast_mode_input(z, ts)
        assert got.shape == ref.shape
        assert (got - ref).abs().max().item() < 1e-5


def test_tiled_decode_vs_goldens_and_oracle(plugin, cuda, cases, golden_vae):
    s = cases["vae_stride"]
    for c in cases["vae"]:
        dec = ld.make_decoder(c["dec_seed"], small=True).to(cuda)
        dec.original_forward = dec.forward
        torch.manual_seed(c["seed"])
        z = torch.randn(1, 4, c["H"], c["W"])
        hook = plugin.tilevae.VAEHook(dec, c["ts"], is_decoder=True, fast_decoder=c["fast"], fast_encoder=False, color_fix=False)
        out = hook(z.to(cuda)).cpu()
        gold = torch.from_numpy(golden_vae[c["name"] + "/sub"])
        err = (out[:, :, ::s, ::s] - gold).abs().max().item() / gold.abs().max().item()
        assert err < 2e-4, f"{c['name']}: rel err {err}"
        mom = golden_vae[c["name"] + "/moments"]
        assert abs(out.double().sum().item() - mom[0]) < 1e-3 * max(1.0, abs(mom[0]), (mom[1]) ** 0.5)
        assert abs((out.double() ** 2).sum().item() - mom[1]) < 2e-3 * mom[1]


@pytest.mark.parametrize("fast", [True, False])
def test_tiled_decode_full_width_decoder(plugin, cuda, fast):
    """The real SD/SDXL decoder widths (ch=128: 512/512/256/128 channels, attention at C=512) on a small latent."""
    dec_cpu = ld.make_decoder(3)
    torch.manual_seed(5)
    z = torch.randn(1, 4, 34, 42)
    ref = vo.tiled_forward(dec_cpu, z, 12, fast)
    dec = ld.make_decoder(3).to(cuda)
    dec.original_forward = dec.forward
    hook = plugin.tilevae.VAEHook(dec, 12, is_decoder=True, fast_decoder=fast, fast_encoder=False, color_fix=False)
    out = hook(z.to(cuda)).cpu()
    err = _rel(out, ref)
    assert err < 2e-4, f"full-width tiled decode (fast={fast}): rel err {err}"


def _random_vae_case(seed):
    import random
    r = random.Random(1000 + seed)
    dec = seed % 3 != 2                       # two decodes for one encode
    if dec:
        H, W, ts = r.randint(30, 120), r.randint(30, 120), r.choice([8, 12, 16, 24, 32, 48])
    else:
        H, W, ts = r.randint(200, 700), r.randint(200, 700), r.choice([64, 96, 128, 200, 256])
    return dec, H, W, ts, bool(r.getrandbits(1)), r.randint(1, 2), (not dec) and bool(r.getrandbits(1))


@pytest.mark.parametrize("seed", [1, 2, 4, 5, 6, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17])      # (0, 3, 10: the CPU oracle needs 7-30 s each)
def test_tiled_vae_random_geometries_vs_cpu_oracle(plugin, cuda, seed):
    """15 seeded random (size, tile, mode, batch) cases on the reduced-width networks against the CPU oracle (upstream's split_tiles,
    estimator, task queue, crop: scripts/tilevae.py:375-388, 464-505, 577-737): odd sizes, one-tile-wide grids, tiles larger than one
    axis, ragged last tiles, stacked and single tiles, live windows on every geometry."""
    dec, H, W, ts, fast, N, color_fix = _random_vae_case(seed)
    net_cpu = ld.make_decoder(seed, small=True) if dec else ld.make_encoder(seed, small=True)
    torch.manual_seed(seed)
    x = torch.randn(N, 4 if dec else 3, H, W)
    ref = vo.tiled_forward(net_cpu, x, ts, fast, is_decoder=dec, color_fix=color_fix)
    net = (ld.make_decoder(seed, small=True) if dec else ld.make_encoder(seed, small=True)).to(cuda)
    net.original_forward = net.forward
    hook = plugin.tilevae.VAEHook(net, ts, is_decoder=dec, fast_decoder=fast, fast_encoder=fast, color_fix=color_fix)
    out = hook(x.to(cuda)).cpu()
    assert out.shape == ref.shape
    err = _rel(out, ref)
    print(f"{'decode' if dec else 'encode'} {N} x {H}x{W} tile {ts} fast={fast} color_fix={color_fix}: rel err {err:.2e}")
    assert err < 2e-4, f"{(dec, H, W, ts, fast, N, color_fix)}: rel err {err}"


def test_untiled_small_input_takes_original_forward(plugin, cuda):
    dec = ld.make_decoder(0, small=True).to(cuda)
    dec.original_forward = dec.forward
    hook = plugin.tilevae.VAEHook(dec, 64, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
    z = torch.randn(1, 4, 48, 48, device=cuda)
    calls = []
    inner = dec.original_forward

    def spy(x):
        calls.append(tuple(x.shape))
        return inner(x)

    dec.original_forward = spy
    out = hook(z)                                           # max(H,W) <= 2*11 + 64  (tilevae.py:381-384)
    assert calls == [(1, 4, 48, 48)], "tiny inputs must be handed to the untouched original forward"
    # the host's own (MIOpen) convs are not run-to-run bit-stable on this stack: compare with a tolerance
    assert torch.allclose(out, inner(z), rtol=1e-4, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------
# encoder direction: stride-2 Downsample conv, encoder queue, pad 32, color_fix semi-fast mode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,cin,cout,H,W", [(1, 128, 128, 40, 66), (2, 32, 32, 17, 21), (1, 256, 256, 64, 64), (1, 512, 512, 33, 95)])
def test_downsample_conv_default_precision_vs_torch(plugin, cuda, B, cin, cout, H, W):
    """ldm Downsample: F.pad(x, (0,1,0,1)) then conv3x3 stride 2 (odd and even sizes), default precision = the split-bf16 stride-2 kernel
    (5e-5: one conv of split-bf16 operands).  (Until round 4 this test shared its name with the precision-parametrised one further down
    and was silently replaced by it: tests/test_no_shadowed_tests.py now rejects duplicate test names.)"""
    E = plugin.engine
    torch.manual_seed(cin + H)
    conv = torch.nn.Conv2d(cin, cout, 3, 2, 0)
    x = torch.randn(B, cin, H, W)
    with torch.no_grad():
        ref = conv(F.pad(x, (0, 1, 0, 1)))
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    out = pc.down2(x.to(cuda)).cpu()
    assert out.shape == ref.shape
    assert _rel(out, ref) < 5e-5


def test_tiled_encode_vs_goldens_and_oracle(plugin, cuda):
    import json, os
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "cases_enc.json")) as f:
        enc_cases = json.load(f)["enc"]
    gold = np.load(os.path.join(here, "vae_enc.npz"))
    for c in enc_cases:
        enc = ld.make_encoder(c["enc_seed"], small=True).to(cuda)
        enc.original_forward = enc.forward
        torch.manual_seed(c["seed"])
        x = torch.randn(1, 3, c["H"], c["W"])
        hook = plugin.tilevae.VAEHook(enc, c["ts"], is_decoder=False, fast_decoder=False, fast_encoder=c["fast"], color_fix=c["color_fix"])
        out = hook(x.to(cuda)).cpu()
        g = torch.from_numpy(gold[c["name"] + "/out"])
        assert out.shape == g.shape, f"{c['name']}: shape {tuple(out.shape)} vs upstream {tuple(g.shape)}"
        err = _rel(out, g)
        assert err < 2e-4, f"{c['name']}: rel err vs the upstream golden {err}"


@pytest.mark.parametrize("fast,color_fix", [(True, False), (False, False), (True, True)])
def test_tiled_encode_full_width_encoder(plugin, cuda, fast, color_fix):
    """The real SD/SDXL encoder widths (ch=128 ... 512, attention at C=512) on a small image, against the oracle."""
    enc_cpu = ld.make_encoder(2)
    torch.manual_seed(6)
    x = torch.randn(1, 3, 168, 136)
    ref = vo.tiled_forward(enc_cpu, x, 64, fast, is_decoder=False, color_fix=color_fix)
    enc = ld.make_encoder(2).to(cuda)
    enc.original_forward = enc.forward
    hook = plugin.tilevae.VAEHook(enc, 64, is_decoder=False, fast_decoder=False, fast_encoder=fast, color_fix=color_fix)
    out = hook(x.to(cuda)).cpu()
    assert out.shape == ref.shape
    err = _rel(out, ref)
    assert err < 2e-4, f"full-width tiled encode (fast={fast}, color_fix={color_fix}): rel err {err}"


@pytest.mark.parametrize("fast", [True, False])
def test_tiled_decode_batch_of_two(plugin, cuda, fast):
    """N = 2 latents in one call (upstream's buffers are [N, ...] throughout; statistics are per sample)."""
    dec_cpu = ld.make_decoder(5, small=True)
    torch.manual_seed(8)
    z = torch.randn(2, 4, 36, 44)
    ref = vo.tiled_forward(dec_cpu, z, 16, fast)
    dec = ld.make_decoder(5, small=True).to(cuda)
    dec.original_forward = dec.forward
    hook = plugin.tilevae.VAEHook(dec, 16, is_decoder=True, fast_decoder=fast, fast_encoder=False, color_fix=False)
    out = hook(z.to(cuda)).cpu()
    assert out.shape == ref.shape
    assert _rel(out, ref) < 2e-4


def test_tiled_decode_half_precision_vae(plugin, cuda):
    """A webui without --no-half-vae hands over an fp16 decoder: weights are taken as they are (fp16 values), the engine
    computes in fp32 / split-bf16 and the result comes back in the net's dtype (upstream :656)."""
    dec_cpu = ld.make_decoder(6, small=True).half().float()          # the fp16-rounded weights, fp32 arithmetic
    torch.manual_seed(9)
    z = torch.randn(1, 4, 36, 44)
    ref = vo.tiled_forward(dec_cpu, z.half().float(), 16, True)
    dec = ld.make_decoder(6, small=True).half().to(cuda)
    dec.original_forward = dec.forward
    hook = plugin.tilevae.VAEHook(dec, 16, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
    out = hook(z.half().to(cuda))
    assert out.dtype == torch.float16
    assert _rel(out.float().cpu(), ref) < 2e-3                          # + one fp16 rounding of the output


@pytest.mark.parametrize("live,L,n_stacked,n_single", [(False, 64, 3, 9), (True, 80, 1 + 4, 16)], ids=["whole_tiles", "live_windows"])
def test_stacked_sweep_falls_back_to_one_tile_per_sweep_on_oom(plugin, cuda, monkeypatch, live, L, n_stacked, n_single):
    """Fast mode stacks tiles of one shape along the batch axis (TILE_BATCH); a stacked sweep that runs out of memory is repeated tile by
    tile and the result is the same image (upstream sizes the tile for ONE tile's activations, scripts/tilevae.py:79-99).
    whole tiles, 64^2 latent at tile 16: 9 tiles = 4 of 38x38, 2 + 2 of 32x38 / 38x32, 1 of 32x32.
    live windows, 80^2: 16 tiles stacked by (shape, window sizes) = 4 inner tiles (one failed stack of 3), 4 x 2 edge tiles (four failed
    stacks of 2), 4 x 1 corner tiles; every tile then runs singly, once (round 4: one pass per chunk, no cut in front of the first
    narrowed upsample conv any more)."""
    tv = plugin.tilevae
    dec = ld.make_decoder(4).to(cuda)
    dec.original_forward = dec.forward
    torch.manual_seed(17)
    z = torch.randn(1, 4, L, L, device=cuda)
    hook = tv.VAEHook(dec, 16, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
    monkeypatch.setattr(tv, "TILE_BATCH", 3)
    monkeypatch.setattr(tv, "LIVE_WINDOW", live)
    ref = hook(z).clone()
    calls = {"stacked": 0, "single": 0}
    orig = tv.VAEHook._advance

    def flaky(self, route, st, **kw):          # (the sweep's input st.x: a stack of tiles when its batch is > N = 1)
        if kw.get("frozen") is None:           # (the estimator pass moves through the same seam, norm by norm: not a tile sweep)
            return orig(self, route, st, **kw)
        if st.x.shape[0] > 1:
            calls["stacked"] += 1
            raise torch.cuda.OutOfMemoryError("simulated")
        calls["single"] += 1
        return orig(self, route, st, **kw)

    monkeypatch.setattr(tv.VAEHook, "_advance", flaky)
    out = hook(z)
    assert calls["stacked"] == n_stacked and calls["single"] == n_single  # one failed stacked sweep per group with > 1 tile, then every tile singly
    assert torch.equal(out, ref)
    # the batch is also bounded by what is free: a tile that "needs" more than the card has gets batch 1
    assert hook._tile_batch_that_fits(1, (10 ** 5, 10 ** 5), cuda) == 1 and hook._tile_batch_that_fits(1, (16, 16), cuda) == 3


@pytest.mark.parametrize("B,cin,cout,H,W", [(1, 128, 128, 67, 130), (2, 64, 64, 40, 37), (1, 32, 48, 16, 66), (1, 256, 256, 90, 64), (1, 128, 128, 2, 2),
                                            (1, 48, 160, 33, 35)])
@pytest.mark.parametrize("exact", [False, True], ids=["bf16x3", "f32"])
def test_downsample_conv_vs_torch(plugin, cuda, B, cin, cout, H, W, exact):
    """ldm Downsample (encoder task, upstream scripts/tilevae.py:155-171): conv3x3 stride 2 over pad(x, right 1, bottom 1) -- the
    split-bf16 stride-2 kernel (default) and the exact-fp32 MFMA kernel (MDTILE_PRECISION_F32) against torch fp32."""
    E = plugin.engine
    torch.manual_seed(cin + cout + H)
    conv = torch.nn.Conv2d(cin, cout, 3, 2, 0)
    x = torch.randn(B, cin, H, W)
    with torch.no_grad():
        ref = conv(F.pad(x, (0, 1, 0, 1)))
    pc = E.PackedConv(conv.weight.detach().to(cuda), conv.bias.detach().to(cuda))
    try:
        if exact:
            E.set_precision(E.PRECISION_F32)
        out = pc.down2(x.to(cuda)).cpu()
    finally:
        E.set_precision(E.PRECISION_BF16X3)
    assert out.shape == ref.shape
    err = _rel(out, ref)
    assert err < (2e-5 if exact else 5e-5), f"downsample conv rel err {err}"


@pytest.mark.parametrize("B,C,T", [(1, 512, 3000), (2, 256, 700), (1, 128, 2050), (1, 512, 77)])
def test_attention_channel_major_v_equals_token_major(plugin, cuda, B, C, T):
    """MDTILE_ATTN_V_CHANNEL_MAJOR: v handed over as [B, C, T] (what the split-bf16 1x1 kernels write) must give the SAME records, hence
    bit-identical attention output, as the token-major form -- T % 4 == 0 (float4 rows) and ragged T."""
    E = plugin.engine
    torch.manual_seed(T + C)
    q, k = torch.randn(B, C, T, device=cuda), torch.randn(B, C, T, device=cuda) * 1.3
    v = torch.randn(B, C, T, device=cuda)
    scale = float(C ** -0.5)
    a = E.vae_attn(q, k, v.permute(0, 2, 1).contiguous(), scale)
    b = E.vae_attn(q, k, v, scale, v_channel_major=True)
    assert torch.equal(a, b)


def test_attention_forced_to_exact_fp32_by_env_alone(cuda):
    """env MDTILE_ATTN_MODE=f32 on its own (conv path untouched) -- documented in include/mdtile.h.  Round 3 regressed it: the host chose
    the v layout from mdtile_get_precision(), which still said BF16X3, and the exact kernel rejected the channel-major v.  The choice is
    now the library's own dispatch predicate (mdtile_vae_attn_takes_channel_major).  The switch is read when the library loads, so
    the decode runs in a child process."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = (
        "import sys, torch\n"
        f"sys.path.insert(0, {root!r})\n"
        "from hostsim import stub_host as sh, ldm_decoder as ld\n"
        "from oracle import vae_oracle as vo\n"
        "sh.install('cuda:0'); sh.set_device('cuda:0'); pl = sh.load_plugin(); E = pl.engine\n"
        "assert E.get_precision() == E.PRECISION_BF16X3 and not E.v_channel_major_ok(128) and not E.v_channel_major_ok(512)\n"
        "dec = ld.make_decoder(2, small=True); torch.manual_seed(4); z = torch.randn(1, 4, 40, 36)\n"
        "ref = vo.tiled_forward(dec, z, 16, True)\n"
        "g = ld.make_decoder(2, small=True).to('cuda:0'); g.original_forward = g.forward\n"
        "out = pl.tilevae.VAEHook(g, 16, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)(z.to('cuda:0')).cpu()\n"
        "err = (out - ref).abs().max().item() / ref.abs().max().item()\n"
        "assert err < 2e-4, err\n"
        "print('attn-f32-env ok', err)\n")
    env = dict(os.environ, MDTILE_ATTN_MODE="f32")
    r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "attn-f32-env ok" in r.stdout, r.stdout[-3000:]


@pytest.mark.parametrize("C,T", [(512, 1444), (512, 7396), (128, 3000)])
def test_attention_of_a_stacked_batch_is_bit_identical_to_the_single_images(plugin, cuda, C, T):
    """A tile's attention must not depend on the tiles it is stacked with (scripts/tilevae.py stacks tiles along the batch axis; the
    live-window and the whole-tile sweeps stack differently and their images are compared bit for bit): the key-range split, which
    fixes the order a query's partial sums are combined in, is chosen per image (csrc/vae_attn_bf16x3.hip: attn_nsplit)."""
    E = plugin.engine
    g = torch.Generator(device="cpu").manual_seed(C + T)
    q = torch.randn(3, C, T, generator=g).to(cuda)
    k = torch.randn(3, C, T, generator=g).to(cuda)
    v = torch.randn(3, C, T, generator=g).to(cuda)
    scale = float(C ** -0.5)
    whole = E.vae_attn(q, k, v, scale, v_channel_major=True)
    for b in range(3):
        one = E.vae_attn(q[b:b + 1].contiguous(), k[b:b + 1].contiguous(), v[b:b + 1].contiguous(), scale, v_channel_major=True)
        assert torch.equal(whole[b:b + 1], one), f"image {b} of the stack differs from its own launch"
    two = E.vae_attn(q[:2].contiguous(), k[:2].contiguous(), v[:2].contiguous(), scale, v_channel_major=True)
    assert torch.equal(whole[:2], two)
