"""DemoFusion on the GPU (csrc/demofusion.hip, tile_methods/demofusion.py): the five kernels and mdtile.moments one by
one against the fp64 restatements of tests/demofusion_ref.py, in fp32, fp16 and bf16, on square, portrait and landscape canvases, and the
delegate's model evaluation end to end against the oracle (pinned to upstream by tests/test_oracle_vs_reference.py).

The kernels promise fp32 operations on the latent's values and ONE rounding to its dtype T, so every tolerance is
    0.5 ulp_T(reference) + k * 2^-24 * (sum of the absolute terms of the element),   without the first term for T = fp32,
with k the number of fp32 roundings the element can collect (demofusion_ref.tolerance); tests/test_demofusion_host.py shows that the promised
arithmetic holds these bounds and that sums kept in T miss them.  Inputs are drawn in fp32 on the CPU and cast to T; the kernel and the
reference see the same T values."""
import math
import random
from types import SimpleNamespace

import pytest
import torch

import demofusion_ref as dr
from hostsim import stub_host as sh
from oracle import demofusion_oracle as do

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
F32 = torch.float32


def _dt(dtype):
    return str(dtype).replace("torch.", "")


# ---------------------------------------------------------------------------------------------------------------------
# the delegate's model evaluation on the engine against the oracle (pinned to upstream)
# ---------------------------------------------------------------------------------------------------------------------
def _demo_tile_fn(x):
    return 0.9 * x + 0.1 * x.flip(-1) + 0.05 * x.flip(-2)


DEMO_CASES = [  # W0, H0, S, window, overlap, jitter, mixture
    (24, 24, 2, 16, 8, True, False),
    (24, 24, 3, 16, 8, True, True),
    (24, 24, 2, 16, 8, False, False),
    (20, 20, 2, 16, 4, True, True),
    (32, 32, 4, 32, 16, True, False),
]


@pytest.mark.parametrize("W0,H0,S,window,overlap,jitter,mixture", DEMO_CASES)
def test_demofusion_sample_one_step_vs_oracle(plugin, cuda, W0, H0, S, window, overlap, jitter, mixture):
    import random
    from oracle import demofusion_oracle as do
    W, H = W0 * S, H0 * S
    p = sh.make_processing(W * 8, H * 8)
    p.random_jitter, p.mixture, p.current_scale_num, p.gaussian_filter = jitter, mixture, S, True
    p.cosine_scale_2, p.cosine_scale_3 = 1.0, 1.0
    p.sd_model = SimpleNamespace(apply_model=lambda x, t, cond: _demo_tile_fn(x))
    smp = sh.kdiff_sampler()
    smp.model_wrap_cfg = SimpleNamespace(step=0, inner_model=SimpleNamespace(forward=None), image_cfg_scale=None, forward=None)
    cls = plugin.demofusion.DemoFusion
    cls.is_edit_model = False
    d = cls(p, smp)
    d.window_size, d.sig = window, 0.3
    d.w, d.h = W, H
    random.seed(1234)
    d.get_views(overlap, 3, 2)
    random.seed(1234)
    origins, J, _, _ = do.views(W, H, window, overlap, jitter)
    assert d.jitter_range == J and [(b.x, b.y) for bb in d.batched_bboxes for b in bb] == origins
    d.sampler_forward = lambda x, sigma, cond: _demo_tile_fn(x)
    d.cosine_factor = 0.5 * (1 + torch.cos(torch.pi * torch.tensor((3 + 1) / (10 + 1))))
    torch.manual_seed(3)
    x = torch.randn(2, 4, H + 2 * J, W + 2 * J)
    cond = {"c_crossattn": [torch.zeros(2, 77, 8, device=cuda)], "c_concat": [torch.zeros(2, 5, 1, 1, device=cuda)]}
    got = d.sample_one_step(x.to(cuda), torch.ones(2, device=cuda), cond).cpu()
    want = do.sample_one_step(x, origins, window, J, 3, 2, S, mixture, True, 0.3, d.cosine_factor, 1.0, 1.0, _demo_tile_fn)
    # the local path and the scatter / mix are the same fp32 operations in the same order; the Gaussian filter's tap order and the
    # std reduction differ from torch's (conv2d / std are not order-specified): fp32 round-off only
    assert torch.allclose(got, want, rtol=2e-5, atol=2e-5), f"max diff {(got - want).abs().max().item()}"


def test_demofusion_local_and_scatter_paths_bit_exact(plugin, cuda):
    """window blend and lattice scatter / mix in isolation: identical to the eager op sequence (fp32, list order)."""
    import random
    from oracle import demofusion_oracle as do
    E = plugin.engine
    W = H = 48
    random.seed(7)
    origins, J, ov, stride = do.views(W, H, 16, 8, True)
    import math
    cols = math.ceil((W - ov) / (16 - ov))
    nom = [min(int(c * ((W - 16) / (cols - 1))), W - 16) for c in range(cols)]
    N, C, Hp, Wp = 2, 4, H + 2 * J, W + 2 * J
    torch.manual_seed(2)
    tiles = torch.randn(len(origins) * N, C, 16, 16)
    buf, cnt = torch.zeros(N, C, Hp, Wp), torch.zeros(N, C, Hp, Wp)
    for i, (x, y) in enumerate(origins):
        buf[:, :, y:y + 16, x:x + 16] += tiles[i * N:(i + 1) * N]
        cnt[:, :, y:y + 16, x:x + 16] += 1
    want = buf / torch.where(cnt == 0, torch.tensor(1), cnt)
    ws = E.WindowSet(origins, nom, nom, J, 16, cuda)
    got = E.window_blend(tiles.to(cuda), ws, N, C, Hp, Wp).cpu()
    assert torch.equal(got, want)
    # lattice gather / scatter + mix
    S = 3
    x = torch.randn(N, C, Hp, Wp)
    xg = torch.randn(N, C, Hp, Wp)
    end = Wp - J
    cells = [(bx, by) for by in range(S) for bx in range(S)]
    h0 = len(range(J, end, S))
    g = E.dilated_gather(x.to(cuda), xg.to(cuda), 4, cells, S, J, h0, h0).cpu()
    ref = torch.cat([(x if i < 4 else xg)[:, :, by + J:end:S, bx + J:end:S] for i, (bx, by) in enumerate(cells)], dim=0)
    assert torch.equal(g, ref)
    for mixture in (False, True):
        outs = torch.randn((2 if mixture else 1) * S * S * N, C, h0, h0)
        xglob = torch.zeros(N, C, Hp, Wp)
        for i, (bx, by) in enumerate(cells + cells if mixture else cells):
            xglob[:, :, by + J:end:S, bx + J:end:S] += outs[i * N:(i + 1) * N]
        c2 = torch.tensor(0.37) ** 1.0
        want = want * 0 + (buf / torch.where(cnt == 0, torch.tensor(1), cnt)) * (1 - c2) + ((xglob / 2 if mixture else xglob) / 1) * c2
        got = E.demofusion_combine(E.window_blend(tiles.to(cuda), ws, N, C, Hp, Wp), outs.to(cuda), S, J, mixture, float(c2)).cpu()
        assert torch.equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------
# window blend: rows != cols, nomx != nomy
# ---------------------------------------------------------------------------------------------------------------------
def _nominal(n, win, ov):
    k = math.ceil((n - ov) / (win - ov)) or 1
    step = (n - win) / (k - 1) if k > 1 else 0
    return [min(int(i * step), n - win) for i in range(k)]


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("W,H,jitter", [(48, 32, True), (32, 48, True), (48, 48, True), (40, 24, False)])
def test_demofusion_window_blend_vs_fp64(plugin, cuda, W, H, jitter, dtype):
    E = plugin.engine
    win = 16
    random.seed(7)
    origins, J, ov, _ = do.views(W, H, win, 8, jitter)
    assert J == (4 if jitter else 0)
    N, C, Hp, Wp = 2, 4, H + 2 * J, W + 2 * J
    cnt = dr.window_counts(origins, win, Hp, Wp)
    # the padding ring a jittered window does not reach has count 0 (-> divided by 1); without jitter there is no ring
    assert int(cnt.max()) >= 4 and (int(cnt.min()) == 0) == jitter
    tiles = torch.randn(len(origins) * N, C, win, win, generator=torch.Generator().manual_seed(W * 100 + H)).to(dtype)
    ws = E.WindowSet(origins, _nominal(W, win, ov), _nominal(H, win, ov), J, win, cuda)
    assert (ws.rows != ws.cols) == (W != H)
    got = E.window_blend(tiles.to(cuda), ws, N, C, Hp, Wp).cpu()
    assert got.dtype == dtype
    ref, mag = dr.window_blend(tiles, origins, N, Hp, Wp)
    r = dr.ratio(got, ref, dr.tolerance(ref, mag, 4, dtype))
    print(f"window blend {W}x{H} J={J} {_dt(dtype)}: max count {int(cnt.max())}, {int((cnt == 0).sum()) * N * C} elements of count 0, "
          f"largest error / bound {r:.5f}")
    assert r <= 1.0
    assert torch.equal(got[:, :, cnt == 0], torch.zeros_like(got[:, :, cnt == 0]))
    if dtype == F32:
        assert torch.equal(got, dr.window_blend(tiles, origins, N, Hp, Wp, dtype=F32)[0])       # the eager fp32 sequence, bit for bit


# ---------------------------------------------------------------------------------------------------------------------
# dilated gather and scatter / mix on the lattice: Hp != Wp, and the largest lattice
# ---------------------------------------------------------------------------------------------------------------------
LATTICES = [(Hp, Wp, S, J, mix) for (Hp, Wp, S, J) in [(64, 48, 2, 4), (48, 64, 2, 4), (84, 60, 3, 6), (60, 84, 3, 6)] for mix in (False, True)]
LATTICES.append((40, 40, 8, 4, True))       # W0 = H0 = 4 at S = 8 with mixture: 128 cells (the kernel's MAX_CELLS), cell coordinates up to 7


def _lattice_id(c):
    return f"{c[0]}x{c[1]}-S{c[2]}-J{c[3]}-{'mix' if c[4] else 'plain'}"


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("case", LATTICES, ids=_lattice_id)
def test_demofusion_dilated_gather_equals_slicing(plugin, cuda, case, dtype):
    E = plugin.engine
    Hp, Wp, S, J, mixture = case
    h0, w0 = dr.lattice_shape(Hp, Wp, S, J)
    N, C = 2, 4
    g = torch.Generator().manual_seed(Hp * 1000 + Wp + S)
    x, xf = torch.randn(N, C, Hp, Wp, generator=g).to(dtype), torch.randn(N, C, Hp, Wp, generator=g).to(dtype)
    cells = dr.lattice_cells(S, mixture)
    assert S != 8 or len(cells) == 128
    for nfirst in ({S * S, S * S - 1, 0} if mixture else {0}):          # the split of a batch between x_in and the filtered latent
        got = E.dilated_gather(x.to(cuda), xf.to(cuda), nfirst, cells, S, J, h0, w0).cpu()
        assert torch.equal(got, dr.dilated_gather(x, xf, nfirst, cells, S, J)[0]), f"num_from_x {nfirst}"


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("case", LATTICES, ids=_lattice_id)
def test_demofusion_combine_vs_fp64(plugin, cuda, case, dtype):
    E = plugin.engine
    Hp, Wp, S, J, mixture = case
    h0, w0 = dr.lattice_shape(Hp, Wp, S, J)
    N, C = 2, 4
    g = torch.Generator().manual_seed(Hp + Wp + S)
    x_local = torch.randn(N, C, Hp, Wp, generator=g).to(dtype)
    gl = torch.randn(len(dr.lattice_cells(S, mixture)) * N, C, h0, w0, generator=g).to(dtype)
    c2 = float(torch.tensor(0.37))
    got = E.demofusion_combine(x_local.to(cuda), gl.to(cuda), S, J, mixture, c2).cpu()
    assert got.dtype == dtype
    ref, mag = dr.combine(x_local, gl, S, J, mixture, c2)
    r = dr.ratio(got, ref, dr.tolerance(ref, mag, 8, dtype))
    print(f"combine {_lattice_id(case)} {_dt(dtype)}: largest error / bound {r:.5f}")
    assert r <= 1.0
    if dtype == F32:
        assert torch.equal(got, dr.combine(x_local, gl, S, J, mixture, c2, dtype=F32)[0])          # the eager fp32 sequence, bit for bit
    end = Wp - J
    if Hp > Wp:
        # the quirk: the lattice ends at Wp - J on BOTH axes, so the rows from there on (still inside the latent) get no global term
        assert end < Hp - J
        local_only = (x_local.float()[:, :, end:] * (1 - torch.tensor(c2))).to(dtype)
        assert torch.equal(got[:, :, end:], local_only)
        assert not torch.equal(got[:, :, J:end, J:end], (x_local.float()[:, :, J:end, J:end] * (1 - torch.tensor(c2))).to(dtype))
    elif Hp < Wp:
        # landscape: the lattice runs through the bottom jitter padding to the last row
        assert J > 0 and J + (h0 - 1) * S + S - 1 == Hp - 1
        assert bool((mag[:, :, Hp - J:, J:end] > x_local.double().abs()[:, :, Hp - J:, J:end] * (1 - c2)).all())


# ---------------------------------------------------------------------------------------------------------------------
# Gaussian filter, re-standardisation, moments
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("shape,K,sigma", [((2, 4, 48, 32), 3, 0.8), ((2, 4, 48, 32), 7, 1.5), ((2, 4, 48, 32), 15, 3.0),
                                           ((1, 1, 5, 9), 15, 3.0),            # K > H and K > W: every tap row / column is clipped somewhere
                                           ((1, 3, 11, 13), 7, 1.5)])          # several planes, odd width
def test_demofusion_blur_vs_fp64(plugin, cuda, shape, K, sigma, dtype):
    E = plugin.engine
    k = plugin.demofusion.DemoFusion.gaussian_kernel(None, K, sigma, 1)[0, 0].to(device=cuda, dtype=F32).contiguous()
    assert tuple(k.shape) == (K, K)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(K)).to(dtype)
    got = E.depthwise_blur(x.to(cuda), k).cpu()
    assert got.dtype == dtype
    ref, mag = dr.blur(x, k.cpu())
    r = dr.ratio(got, ref, dr.tolerance(ref, mag, K * K, dtype))
    print(f"blur {shape} K={K} {_dt(dtype)}: largest error / bound {r:.5f}")
    assert r <= 1.0


@pytest.mark.parametrize("dtype,mean,std,shape", [(torch.float32, 50.0, 0.5, (2, 4, 24, 40)), (torch.bfloat16, 50.0, 0.5, (2, 4, 24, 40)),
                                                  (torch.float16, 0.0, 1.0, (2, 4, 24, 40)),
                                                  (torch.float32, 0.0, 1.0, (2, 3, 7, 11)), (torch.bfloat16, 0.0, 1.0, (2, 3, 7, 11)),
                                                  (torch.float16, 0.0, 1.0, (2, 3, 7, 11))], ids=str)
def test_demofusion_restandardize_vs_fp64(plugin, cuda, dtype, mean, std, shape):
    E = plugin.engine
    g = torch.Generator().manual_seed(5)
    x = (torch.randn(*shape, generator=g) * std + mean).to(dtype)
    tgt = (torch.randn(*shape, generator=g) * 1.7 * std + mean + 0.3).to(dtype)
    st = torch.stack(dr.moments(x) + dr.moments(tgt)).float()            # (mean, std of x, target mean, target std) as the kernel reads them
    got = E.restandardize(x.to(cuda), st.to(cuda)).cpu()
    assert got.dtype == dtype
    ref, mag = dr.restandardize(x, st)
    r = dr.ratio(got, ref, dr.tolerance(ref, mag, 8, dtype))
    print(f"restandardize {shape} mean {mean} std {std} {_dt(dtype)}: largest error / bound {r:.5f}")
    assert r <= 1.0


@pytest.mark.parametrize("dtype,mean,std,shape", [(torch.float32, 0.0, 1.0, (2, 4, 48, 32)), (torch.float32, 50.0, 0.5, (2, 4, 48, 32)),
                                                  (torch.float16, 0.0, 1.0, (2, 4, 48, 32)), (torch.bfloat16, 50.0, 0.5, (2, 4, 48, 32)),
                                                  (torch.float32, 0.0, 1.0, (1, 3, 7, 11))], ids=str)
def test_demofusion_moments_vs_fp64(plugin, cuda, dtype, mean, std, shape):
    """mean = 100 * std is where the E[x^2] - mean^2 form loses digits: the bound carries the (1 + mean^2 / var) amplification."""
    E = plugin.engine
    x = (torch.randn(*shape, generator=torch.Generator().manual_seed(9)) * std + mean).to(dtype)
    got = E.moments(x.to(cuda)).cpu()
    assert got.dtype == torch.float64 and tuple(got.shape) == (2,)
    m, s = x.double().mean(), x.double().std()
    n = x.numel()
    tol_mean = n * 2.0 ** -52 * float(x.double().abs().mean())
    tol_std = n * 2.0 ** -52 * (1.0 + float(m) ** 2 / float(s) ** 2)
    e_mean, e_std = abs(float(got[0] - m)), abs(float(got[1] - s)) / float(s)
    print(f"moments {shape} mean {mean} std {std} {_dt(dtype)}: mean error {e_mean:.3e} (bound {tol_mean:.3e}), relative std error {e_std:.3e} "
          f"(bound {tol_std:.3e})")
    assert e_mean <= tol_mean and e_std <= tol_std


def test_demofusion_gather_rects_bf16_equals_slicing(plugin, cuda):
    """The local windows of a jitter-padded portrait canvas, as the delegate gathers them, and the batch copies of both samplers."""
    E = plugin.engine
    x = torch.randn(2, 4, 64, 48, generator=torch.Generator().manual_seed(3)).to(torch.bfloat16)
    rects = [(0, 4), (13, 1), (32, 7), (5, 29), (17, 48), (31, 45)]
    rows = torch.cat([x[:, :, y:y + 16, xx:xx + 16] for (xx, y) in rects], dim=0)
    assert torch.equal(E.gather_rects(x.to(cuda), rects, 16, 16).cpu(), rows)
    assert torch.equal(E.gather_rects(x.to(cuda), rects, 16, 16, repeat=3, tile_major=True).cpu(), rows.repeat_interleave(3, dim=0))
    assert torch.equal(E.gather_rects(x.to(cuda), rects, 16, 16, repeat=2, tile_major=False).cpu(), rows.repeat(2, 1, 1, 1))


# ---------------------------------------------------------------------------------------------------------------------
# the delegate end to end on non-square canvases, in every dtype
# ---------------------------------------------------------------------------------------------------------------------
NONSQUARE = [  # W0, H0, S, window, overlap, jitter, mixture: the rows pinned to upstream in tests/test_oracle_vs_reference.py
    (20, 28, 2, 16, 8, True, False),
    (28, 20, 2, 16, 8, True, True),
    (16, 24, 3, 16, 12, True, True),
    (24, 16, 3, 16, 12, True, False),
    (28, 20, 2, 16, 8, False, True),
]


def _delegate(plugin, W0, H0, S, window, overlap, jitter, mixture):
    W, H = W0 * S, H0 * S
    p = sh.make_processing(W * 8, H * 8)
    p.random_jitter, p.mixture, p.current_scale_num, p.gaussian_filter = jitter, mixture, S, True
    p.cosine_scale_2, p.cosine_scale_3 = 1.0, 1.0
    p.sd_model = SimpleNamespace(apply_model=lambda x, t, cond: _demo_tile_fn(x))
    smp = sh.kdiff_sampler()
    smp.model_wrap_cfg = SimpleNamespace(step=0, inner_model=SimpleNamespace(forward=None), image_cfg_scale=None, forward=None)
    cls = plugin.demofusion.DemoFusion
    cls.is_edit_model = False
    d = cls(p, smp)
    d.window_size, d.sig = window, 0.3
    d.w, d.h = W, H
    random.seed(1234)
    d.get_views(overlap, 3, 2)
    random.seed(1234)
    origins, J, _, _ = do.views(W, H, window, overlap, jitter)
    assert d.jitter_range == J and [(b.x, b.y) for bb in d.batched_bboxes for b in bb] == origins
    d.sampler_forward = lambda x, sigma, cond: _demo_tile_fn(x)
    d.cosine_factor = 0.5 * (1 + torch.cos(torch.pi * torch.tensor((3 + 1) / (10 + 1))))
    return d, origins, J, W, H


def _cond(cuda):
    return {"c_crossattn": [torch.zeros(2, 77, 8, device=cuda)], "c_concat": [torch.zeros(2, 5, 1, 1, device=cuda)]}


@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
@pytest.mark.parametrize("W0,H0,S,window,overlap,jitter,mixture", NONSQUARE)
def test_demofusion_nonsquare_sample_one_step_vs_oracle(plugin, cuda, W0, H0, S, window, overlap, jitter, mixture, dtype):
    """fp32: the criterion of the square cases.  Half: the stand-in model rounds to T inside torch, so no bound follows from the kernels alone;
    instead the engine (fp32 inside every kernel, one rounding each) must be no further from the fp64 evaluation of the same T inputs than
    upstream's own arithmetic, the eager evaluation in T, which rounds after every operation."""
    d, origins, J, W, H = _delegate(plugin, W0, H0, S, window, overlap, jitter, mixture)
    torch.manual_seed(3)
    x = torch.randn(2, 4, H + 2 * J, W + 2 * J).to(dtype)
    got = d.sample_one_step(x.to(cuda), torch.ones(2, device=cuda), _cond(cuda)).cpu()
    assert got.dtype == dtype and got.shape == x.shape

    def oracle(v):
        return do.sample_one_step(v, origins, window, J, 3, 2, S, mixture, True, 0.3, d.cosine_factor, 1.0, 1.0, _demo_tile_fn)
    if dtype == F32:
        want = oracle(x)
        assert torch.allclose(got, want, rtol=2e-5, atol=2e-5), f"max diff {(got - want).abs().max().item()}"
        return
    ref64 = oracle(x.double())
    eager = oracle(x.clone())
    assert ref64.dtype == torch.float64 and eager.dtype == dtype
    e_rms, e_max = dr.rms(got.double() - ref64), float((got.double() - ref64).abs().max())
    t_rms, t_max = dr.rms(eager.double() - ref64), float((eager.double() - ref64).abs().max())
    print(f"sample_one_step {W0}x{H0} S={S} jitter={jitter} mixture={mixture} {_dt(dtype)}: engine rms {e_rms:.4e} max {e_max:.4e}, "
          f"eager in T rms {t_rms:.4e} max {t_max:.4e}  (ratios {e_rms / t_rms:.3f}, {e_max / t_max:.3f})")
    assert e_rms <= 1.0 * t_rms
    assert e_max <= 1.25 * t_max


def test_demofusion_landscape_lattice_that_cannot_tile_raises(plugin, cuda):
    """J = 4 is no multiple of S = 3: the lattice rows run into the bottom padding with different lengths.  Upstream fails in torch.cat;
    the delegate raises before any lattice kernel reads past a view, and the device stays usable."""
    W0, H0, S, window, overlap, jitter, mixture = 28, 20, 3, 16, 8, True, False
    d, origins, J, W, H = _delegate(plugin, W0, H0, S, window, overlap, jitter, mixture)
    assert J == 4 and dr.lattice_shape(H + 2 * J, W + 2 * J, S, J) is None
    torch.manual_seed(3)
    x = torch.randn(2, 4, H + 2 * J, W + 2 * J)
    with pytest.raises(RuntimeError):
        do.sample_one_step(x, origins, window, J, 3, 2, S, mixture, True, 0.3, d.cosine_factor, 1.0, 1.0, _demo_tile_fn)
    with pytest.raises(ValueError):
        d.sample_one_step(x.to(cuda), torch.ones(2, device=cuda), _cond(cuda))
    torch.cuda.synchronize()
    k = plugin.demofusion.DemoFusion.gaussian_kernel(None, 3, 0.8, 1)[0, 0].to(device=cuda, dtype=F32).contiguous()
    got = plugin.engine.depthwise_blur(x.to(cuda), k).cpu()
    ref, mag = dr.blur(x, k.cpu())
    assert dr.ratio(got, ref, dr.tolerance(ref, mag, 9, F32)) <= 1.0
