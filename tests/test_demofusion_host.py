"""tests/demofusion_ref.py on the CPU, so that tests/test_gpu_demofusion.py rests on something:
  * in fp32 the references ARE the eager op sequence of oracle/demofusion_oracle.py (pinned to upstream): bit for bit for the window blend,
    the dilated gather and the scatter / mix, within 1e-6 for the Gaussian filter (conv2d's tap order is not specified);
  * the arithmetic the kernels promise -- fp32 operations on T inputs, ONE rounding to T -- stays inside the tolerances of the GPU tests;
  * the arithmetic they must not have -- every operation rounded to T, as eager torch does -- does not: the GPU tests would notice it.
"""
import random

import pytest
import torch

import demofusion_ref as dr
from oracle import demofusion_oracle as do

HALF = [torch.float16, torch.bfloat16]
CANVASES = [(48, 32), (32, 48), (48, 48)]          # W, H of the latent; window 16, overlap 8, random.seed(7): J = 4


def _tile_fn(x):
    return 0.9 * x + 0.1 * x.flip(-1) + 0.05 * x.flip(-2)


@pytest.mark.parametrize("dtype,values", [
    (torch.float16, [0.0, 2.0 ** -24, 3e-5, 2.0 ** -14, 0.1, 0.999, 1.0, 1.5, 2.0, 1000.0, 32768.0]),
    (torch.bfloat16, [0.0, 2.0 ** -133, 2.0 ** -126, 0.1, 0.999, 1.0, 1.5, 2.0, 50.0, 3e38]),
    (torch.float32, [0.0, 2.0 ** -149, 2.0 ** -126, 0.1, 0.999, 1.0, 1.5, 2.0, 50.0, 3e38])])
def test_demofusion_ref_ulp_is_the_spacing_of_the_format(dtype, values):
    v = torch.tensor(values, dtype=torch.float64).to(dtype)                    # representable values of T (positive: next pattern = next value)
    ints = torch.int16 if dtype != torch.float32 else torch.int32
    nxt = (v.view(ints) + 1).view(dtype)
    assert torch.equal(dr.ulp(v.double(), dtype), nxt.double() - v.double())
    assert torch.equal(dr.ulp(-v.double(), dtype), dr.ulp(v.double(), dtype))
    # inside a binade the spacing is that of the binade's lower end
    assert float(dr.ulp(torch.tensor(1.999), dtype)) == float(dr.ulp(torch.tensor(1.0), dtype))


@pytest.mark.parametrize("W0,H0,S,window,overlap,jitter,mixture", [
    (20, 28, 2, 16, 8, True, False), (28, 20, 2, 16, 8, True, True), (16, 24, 3, 16, 12, True, True), (24, 16, 3, 16, 12, True, False),
    (28, 20, 2, 16, 8, False, True), (24, 24, 3, 16, 8, True, True)])
def test_demofusion_ref_fp32_is_the_oracle_sequence(W0, H0, S, window, overlap, jitter, mixture):
    """One model evaluation composed from the references in fp32 equals the oracle's, bit for bit (the filtered latent is taken from the
    oracle's own conv2d, which the references only match to round-off)."""
    W, H = W0 * S, H0 * S
    cf = 0.5 * (1 + torch.cos(torch.pi * torch.tensor((3 + 1) / (10 + 1))))
    random.seed(1234)
    origins, J, _, _ = do.views(W, H, window, overlap, jitter)
    torch.manual_seed(3)
    N = 2
    x = torch.randn(N, 4, H + 2 * J, W + 2 * J)
    Hp, Wp = x.shape[2:]
    want = do.sample_one_step(x.clone(), origins, window, J, 3, 2, S, mixture, True, 0.3, cf, 1.0, 1.0, _tile_fn)

    f32 = torch.float32
    tiles = torch.cat([_tile_fn(torch.cat([x[:, :, oy:oy + window, ox:ox + window] for (ox, oy) in b], dim=0)) for b in do.batches(origins, 3)], dim=0)
    x_local, _ = dr.window_blend(tiles, origins, N, Hp, Wp, dtype=f32)
    K, sigma = 2 * S - 1, 0.3 * (0.99 * cf ** 1.0 + 1e-2)
    xg = do.gaussian_filter(x, K, sigma)
    mine, _ = dr.blur(x, do.gaussian_kernel(K, sigma, 1)[0, 0], dtype=f32)
    assert (mine - xg).abs().max().item() <= 1e-6
    xg, _ = dr.restandardize(xg, (xg.mean(), xg.std(), x.mean(), x.std()), dtype=f32)
    cells = dr.lattice_cells(S, mixture)
    assert dr.lattice_shape(Hp, Wp, S, J) is not None
    gouts = []
    for b in do.batches(cells, 2):                      # the model sees the cells in batches; tile_fn acts per row, so batching is immaterial
        first = len(gouts)
        n_from_x = max(0, min(len(b), S * S - first)) if mixture else 0
        gouts += [_tile_fn(t) for t in dr.dilated_gather(x, xg, n_from_x, b, S, J)[0].split(N)]
    got, _ = dr.combine(x_local, torch.cat(gouts, dim=0), S, J, mixture, float(cf ** 1.0), dtype=f32)
    assert torch.equal(got, want)


def _blend_case(W, H, dtype, seed=7, jitter=True):
    random.seed(seed)
    origins, J, _, _ = do.views(W, H, 16, 8, jitter)
    N, C, Hp, Wp = 2, 4, H + 2 * J, W + 2 * J
    g = torch.Generator().manual_seed(W * 100 + H)
    tiles = torch.randn(len(origins) * N, C, 16, 16, generator=g).to(dtype)
    return origins, J, N, Hp, Wp, tiles


@pytest.mark.parametrize("dtype", HALF, ids=str)
@pytest.mark.parametrize("W,H", CANVASES)
def test_demofusion_blend_bound_holds_for_fp32_sums_and_catches_sums_in_T(W, H, dtype):
    origins, J, N, Hp, Wp, tiles = _blend_case(W, H, dtype)
    cnt = dr.window_counts(origins, 16, Hp, Wp)
    assert J == 4 and int(cnt.min()) == 0 and int(cnt.max()) >= 4
    ref, mag = dr.window_blend(tiles, origins, N, Hp, Wp)
    tol = dr.tolerance(ref, mag, 4, dtype)
    promised = dr.window_blend(tiles, origins, N, Hp, Wp, dtype=torch.float32)[0].to(dtype)
    eager = dr.window_blend(tiles, origins, N, Hp, Wp, dtype=dtype)[0]
    r_ok, r_bad = dr.ratio(promised, ref, tol), dr.ratio(eager, ref, tol)
    over = float(((eager.double() - ref).abs() > tol).double().mean())
    print(f"blend {W}x{H} {dtype}: fp32 sums {r_ok:.5f} of the bound, sums in T {r_bad:.2f} ({100 * over:.1f} % of the elements over it)")
    assert r_ok <= 1.0
    assert r_bad > 1.0 and over > 0.01
    # fp32: the same sequence is the reference of the bit-exact GPU assertion, and it holds the fp32 bound too
    t32 = tiles.float()
    ref32, mag32 = dr.window_blend(t32, origins, N, Hp, Wp)
    assert dr.ratio(dr.window_blend(t32, origins, N, Hp, Wp, dtype=torch.float32)[0], ref32, dr.tolerance(ref32, mag32, 4, torch.float32)) <= 1.0


@pytest.mark.parametrize("dtype", HALF, ids=str)
@pytest.mark.parametrize("Hp,Wp,S,J,mixture", [(64, 48, 2, 4, True), (48, 64, 2, 4, False), (84, 60, 3, 6, True), (40, 40, 8, 4, True)])
def test_demofusion_combine_bound_holds_for_fp32_and_catches_T(Hp, Wp, S, J, mixture, dtype):
    h0, w0 = dr.lattice_shape(Hp, Wp, S, J)
    N, C = 2, 4
    g = torch.Generator().manual_seed(Hp + Wp + S)
    x_local = torch.randn(N, C, Hp, Wp, generator=g).to(dtype)
    gl = torch.randn(len(dr.lattice_cells(S, mixture)) * N, C, h0, w0, generator=g).to(dtype)
    c2 = float(torch.tensor(0.37))
    ref, mag = dr.combine(x_local, gl, S, J, mixture, c2)
    tol = dr.tolerance(ref, mag, 8, dtype)
    r_ok = dr.ratio(dr.combine(x_local, gl, S, J, mixture, c2, dtype=torch.float32)[0].to(dtype), ref, tol)
    r_bad = dr.ratio(dr.combine(x_local, gl, S, J, mixture, c2, dtype=dtype)[0], ref, tol)
    print(f"combine {Hp}x{Wp} S={S} {dtype}: fp32 {r_ok:.5f} of the bound, in T {r_bad:.2f}")
    assert r_ok <= 1.0 < r_bad


@pytest.mark.parametrize("dtype", HALF, ids=str)
@pytest.mark.parametrize("shape,K,sigma", [((2, 4, 48, 32), 3, 0.8), ((2, 4, 48, 32), 7, 1.5), ((2, 4, 48, 32), 15, 3.0), ((1, 1, 5, 9), 15, 3.0)])
def test_demofusion_blur_bound_holds_for_fp32_and_catches_T(shape, K, sigma, dtype):
    torch.manual_seed(K)
    x = torch.randn(*shape).to(dtype)
    k = do.gaussian_kernel(K, sigma, 1)[0, 0].float()
    ref, mag = dr.blur(x, k)
    tol = dr.tolerance(ref, mag, K * K, dtype)
    r_ok = dr.ratio(dr.blur(x, k, dtype=torch.float32)[0].to(dtype), ref, tol)
    r_bad = dr.ratio(dr.blur(x, k, dtype=dtype)[0], ref, tol)
    print(f"blur {shape} K={K} {dtype}: fp32 {r_ok:.5f} of the bound, in T {r_bad:.2f}")
    assert r_ok <= 1.0 < r_bad


@pytest.mark.parametrize("dtype,mean,std", [(torch.float16, 0.0, 1.0), (torch.bfloat16, 50.0, 0.5), (torch.float32, 50.0, 0.5)], ids=str)
def test_demofusion_restandardize_bound_holds_for_fp32_and_catches_T(dtype, mean, std):
    torch.manual_seed(5)
    x = (torch.randn(2, 4, 24, 40) * std + mean).to(dtype)
    tgt = (torch.randn(2, 4, 24, 40) * 1.7 * std + mean + 0.3).to(dtype)
    st = torch.stack(dr.moments(x) + dr.moments(tgt)).float()
    ref, mag = dr.restandardize(x, st)
    tol = dr.tolerance(ref, mag, 8, dtype)
    r_ok = dr.ratio(dr.restandardize(x, st, dtype=torch.float32)[0].to(dtype), ref, tol)
    print(f"restandardize {dtype}: fp32 {r_ok:.5f} of the bound")
    assert r_ok <= 1.0
    if dtype != torch.float32:
        r_bad = dr.ratio(dr.restandardize(x, st.to(dtype), dtype=dtype)[0], ref, tol)
        print(f"restandardize {dtype}: in T {r_bad:.2f}")
        assert r_bad > 1.0


def test_demofusion_ref_moments_are_torch_mean_and_std():
    torch.manual_seed(1)
    x = torch.randn(3, 5, 7, 11) * 0.5 + 50.0
    mean, std = dr.moments(x)
    assert abs(float(mean) - float(x.double().mean())) <= 1e-13 * 50 and abs(float(std) - float(x.double().std())) <= 1e-13
