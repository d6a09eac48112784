"""Restatements of the DemoFusion operations (csrc/demofusion.hip, mdtile.moments) as the obvious slicing loops, independent of the engine:

    window_blend     count-averaged sum of the jittered windows                       (upstream demofusion.py:244-257)
    dilated_gather   cat of the strided views of the S x S lattice cells               (:268-283)
    combine          scatter of the global outputs + x_local * (1 - c2) + x_global * c2 (:284-322)
    blur             depthwise K x K filter, zero padding                              (:173-178)
    restandardize    (x - mean_g) / std_g * std + mean                                 (:264)
    moments          (mean, unbiased std) of the whole tensor

Every reference works in `dtype` (float64 unless a test asks for the eager fp32 sequence) and returns TWO tensors: the result, and the sum of
the absolute values of the terms that make up each element -- the quantity the round-off of an fp32 evaluation scales with.
tolerance() turns the pair into the bound the kernels are held to: fp32 operations, ONE rounding to the latent's dtype T.

Both axes of the lattice end at  Wp - J  (upstream takes the end of the rows from the width, :262); slicing clips the rows at Hp.
"""
import math

import torch

U = 2.0 ** -24          # unit round-off of fp32

FORMATS = {             # dtype: (explicit significand bits, emin)
    torch.float16: (10, -14),
    torch.bfloat16: (7, -126),
    torch.float32: (23, -126),
}


def ulp(v, dtype):
    """Spacing of `dtype` at |v| (fp64 tensor), with the subnormal floor: 2^(max(floor(log2 |v|), emin) - bits)."""
    bits, emin = FORMATS[dtype]
    v = torch.as_tensor(v, dtype=torch.float64)
    _, e = torch.frexp(v.abs())                         # |v| = m * 2^e, m in [0.5, 1): floor(log2 |v|) = e - 1; frexp(0) has e = 0
    e = torch.where(v == 0, torch.full_like(e, emin), e - 1)
    return torch.ldexp(torch.ones_like(v), torch.clamp(e, min=emin) - bits)


def tolerance(ref, abs_terms, factor, dtype):
    """0.5 ulp_T(ref) + factor * u * abs_terms; the rounding term is dropped for T = fp32 (nothing is rounded after the fp32 operations)."""
    t = factor * U * abs_terms
    return t if dtype == torch.float32 else t + 0.5 * ulp(ref, dtype)


def ratio(got, ref, tol):
    """Largest |got - ref| / tol (0 / 0 counts as 0: an element that must be exact and is)."""
    err = (got.double() - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / tol)
    return float(r.max())


# ---- local path --------------------------------------------------------------------------------------------------------------------------------
def window_counts(origins, win, Hp, Wp):
    cnt = torch.zeros(Hp, Wp, dtype=torch.int64)
    for (x, y) in origins:
        cnt[y:y + win, x:x + win] += 1
    return cnt


def window_blend(tiles, origins, N, Hp, Wp, dtype=torch.float64):
    """tiles [len(origins) * N, C, win, win], tile-major.  -> (sum / max(count, 1), sum of |tile| / max(count, 1))"""
    tiles = tiles.to(dtype)
    C, win = tiles.shape[1], tiles.shape[2]
    buf = torch.zeros(N, C, Hp, Wp, dtype=dtype)
    mag = torch.zeros(N, C, Hp, Wp, dtype=dtype)
    cnt = torch.zeros(N, C, Hp, Wp, dtype=dtype)
    for i, (x, y) in enumerate(origins):
        buf[:, :, y:y + win, x:x + win] += tiles[i * N:(i + 1) * N]
        mag[:, :, y:y + win, x:x + win] += tiles[i * N:(i + 1) * N].abs()
        cnt[:, :, y:y + win, x:x + win] += 1
    cnt = torch.where(cnt == 0, torch.ones_like(cnt), cnt)
    return buf / cnt, mag / cnt


# ---- global path -------------------------------------------------------------------------------------------------------------------------------
def lattice_cells(S, mixture):
    cells = [(bx, by) for by in range(S) for bx in range(S)]
    return cells + cells if mixture else cells


def lattice_shape(Hp, Wp, S, J):
    """(h0, w0) of the dilated views, or None where the S x S lattice does not tile the canvas (views of different sizes)."""
    end = Wp - J
    hs = {len(range(by + J, min(end, Hp), S)) for by in range(S)}
    ws = {len(range(bx + J, end, S)) for bx in range(S)}
    return (hs.pop(), ws.pop()) if len(hs) == 1 and len(ws) == 1 else None


def dilated_gather(x, x_filtered, num_from_x, cells, S, J):
    """-> (cat of the views, their absolute values): the first num_from_x cells view x, the others x_filtered."""
    end = x.shape[3] - J
    out = torch.cat([(x if i < num_from_x else x_filtered)[:, :, by + J:end:S, bx + J:end:S] for i, (bx, by) in enumerate(cells)], dim=0)
    return out, out.abs()


def combine(x_local, g, S, J, mixture, c2, dtype=torch.float64):
    """g [cells * N, C, h0, w0] in cell-list order; c2 a Python float.  -> (x_local * (1 - c2) + x_global * c2,
    |x_local| * (1 - c2) + sum of |global terms| * c2)"""
    x_local, g = x_local.to(dtype), g.to(dtype)
    N, _, Hp, Wp = x_local.shape
    end = Wp - J
    c2 = torch.tensor(c2, dtype=dtype)
    xg = torch.zeros_like(x_local)
    mag = torch.zeros_like(x_local)
    for i, (bx, by) in enumerate(lattice_cells(S, mixture)):
        xg[:, :, by + J:end:S, bx + J:end:S] += g[i * N:(i + 1) * N]
        mag[:, :, by + J:end:S, bx + J:end:S] += g[i * N:(i + 1) * N].abs()
    if mixture:
        xg, mag = xg / 2, mag / 2
    return x_local * (1 - c2) + xg * c2, x_local.abs() * (1 - c2) + mag * c2


# ---- Gaussian filter and re-standardisation ---------------------------------------------------------------------------------------------------
def blur(x, kernel2d, dtype=torch.float64):
    """Every plane of x [N, C, H, W] filtered with kernel2d [K, K], zeros outside.  -> (sum of x * k, sum of |x * k|)"""
    x, k = x.to(dtype), kernel2d.to(dtype)
    K = k.shape[0]
    r = K // 2
    H, W = x.shape[2:]
    p = torch.zeros(x.shape[0], x.shape[1], H + 2 * r, W + 2 * r, dtype=dtype)
    p[:, :, r:r + H, r:r + W] = x
    out, mag = torch.zeros_like(x), torch.zeros_like(x)
    for ky in range(K):
        for kx in range(K):
            term = p[:, :, ky:ky + H, kx:kx + W] * k[ky, kx]
            out += term
            mag += term.abs()
    return out, mag


def restandardize(x, stats4, dtype=torch.float64):
    """stats4 = (mean of x, std of x, target mean, target std).  -> ((x - m_g) / s_g * s + m, |x - m_g| / s_g * s + |m|)"""
    x = x.to(dtype)
    m_g, s_g, m, s = [v.to(dtype) for v in stats4]
    return (x - m_g) / s_g * s + m, (x - m_g).abs() / s_g * s + m.abs()


def moments(x):
    """-> (mean, unbiased std) of the whole tensor in fp64, two-pass."""
    v = x.double().reshape(-1)
    mean = v.sum() / v.numel()
    return mean, torch.sqrt(((v - mean) ** 2).sum() / (v.numel() - 1))


def moments_tolerance(x):
    """(bound on |mean error|, bound on the RELATIVE std error) of fp64 sums in the E[x^2] - mean^2 form: every sum carries at most n * 2^-52 of
    its absolute terms, and the subtraction amplifies the relative error of the variance by (mean^2 + var) / var."""
    mean, std = moments(x)
    n = x.numel()
    return n * 2.0 ** -52 * float(x.double().abs().mean()), n * 2.0 ** -52 * (1.0 + float(mean) ** 2 / float(std) ** 2)


def rms(v):
    return math.sqrt(float((v.double() ** 2).mean()))
