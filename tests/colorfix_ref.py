"""Restatements of the colour fix (include/mdtile.h) in numpy, written from the definition and independent of the engine:

    wavelet_literal   the literal definition in float64: five dilated 3x3 blurs after replicate padding, high / low split, round once
    wavelet_int       the integer form the engine is held to, bit for bit
    wavelet_pad_once  the WRONG variant that pads once by 31 and then convolves; here only to show that the cases tell it apart
    adain_pixels      AdaIN per pixel in float64
    SHAPES, cases()   the case list both test files share
"""
import math

import numpy as np

LEVELS = 5
SHIFT = 4 * LEVELS          # ten 1-D levels of weight 4

SHAPES = [(1, 1, 1), (1, 7, 3), (5, 1, 1), (2, 3, 3),
          (17, 33, 3), (31, 32, 1),                       # below the halo of 31 in both axes
          (64, 64, 3),
          (65, 130, 3), (97, 200, 3), (130, 67, 1)]
KINDS = ["random", "two_level_white", "two_level_inverse", "ramps"]


def _shaped(a, shape):
    return a.reshape(shape[:2]) if shape[2] == 1 and len(a.shape) == 3 else a


def make_pair(shape, kind):
    """(content, style) uint8 arrays of `shape` = (H, W, C); C == 1 gives [H, W]."""
    H, W, C = shape
    rng = np.random.default_rng(1000 * H + 10 * W + C + 7 * KINDS.index(kind))
    if kind == "random":
        content = rng.integers(0, 256, size=shape, dtype=np.uint8)
        style = rng.integers(0, 256, size=shape, dtype=np.uint8)
    elif kind == "two_level_white":          # d = style - content is 0 or +255
        content = (rng.integers(0, 2, size=shape) * 255).astype(np.uint8)
        style = np.full(shape, 255, np.uint8)
    elif kind == "two_level_inverse":        # d = +-255 everywhere, +255 in the whole top left quarter: v = 255 * 2^20 at its corner
        content = (rng.integers(0, 2, size=shape) * 255).astype(np.uint8)
        content[:H // 2, :W // 2] = 0
        style = (255 - content).astype(np.uint8)
    elif kind == "ramps":
        y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(C), indexing="ij")
        content = ((3 * x + 5 * y + 40 * c) % 256).astype(np.uint8)
        style = ((255 - 2 * x + 7 * y + 90 * c) % 256).astype(np.uint8)
    else:
        raise ValueError(kind)
    return _shaped(np.ascontiguousarray(content), shape), _shaped(np.ascontiguousarray(style), shape)


def cases(extra_shapes=()):
    return [(tuple(s), k) for s in list(SHAPES) + list(extra_shapes) for k in KINDS]


def case_id(case):
    (h, w, c), kind = case
    return f"{h}x{w}x{c}-{kind}"


def _hwc(a):
    return a[:, :, None] if a.ndim == 2 else a


# ---- the literal definition ------------------------------------------------------------------------------------------------------------------
def _blur(x, r):
    """[[1,2,1],[2,4,2],[1,2,1]] / 16 with dilation r after replicate padding by r; x float64 [H, W, C]."""
    H, W = x.shape[:2]
    p = np.pad(x, ((r, r), (r, r), (0, 0)), mode="edge")
    out = np.zeros_like(x)
    for dy, wy in ((-1, 1.0), (0, 2.0), (1, 1.0)):
        for dx, wx in ((-1, 1.0), (0, 2.0), (1, 1.0)):
            out += (wy * wx / 16.0) * p[r + dy * r:r + dy * r + H, r + dx * r:r + dx * r + W]
    return out


def _decompose(x):
    high = np.zeros_like(x)
    for i in range(LEVELS):
        low = _blur(x, 2 ** i)
        high += x - low
        x = low
    return high, x


def wavelet_literal(content, style):
    c, s = _hwc(content).astype(np.float64), _hwc(style).astype(np.float64)
    high, _ = _decompose(c)
    _, low = _decompose(s)
    out = np.clip(np.floor(high + low + 0.5), 0, 255).astype(np.uint8)
    return out.reshape(content.shape)


# ---- the integer form ------------------------------------------------------------------------------------------------------------------------
def _level(v, r, axis):
    n = v.shape[axis]
    i = np.arange(n)
    return np.take(v, np.clip(i - r, 0, n - 1), axis=axis) + 2 * v + np.take(v, np.clip(i + r, 0, n - 1), axis=axis)


def low5_int(d):
    """Ten 1-D levels on int64 [H, W, C]: the low band of d times 2^20."""
    v = d
    for axis in (1, 0):
        for k in range(LEVELS):
            v = _level(v, 2 ** k, axis)
    return v


def wavelet_int(content, style):
    c = _hwc(content).astype(np.int64)
    v = low5_int(_hwc(style).astype(np.int64) - c)
    assert np.abs(v).max() <= 255 << SHIFT
    out = np.clip((c * (1 << SHIFT) + v + (1 << (SHIFT - 1))) >> SHIFT, 0, 255).astype(np.uint8)
    return out.reshape(content.shape)


def wavelet_pad_once(content, style):
    """Replicate padding ONCE by 31, then the ten levels without any clamp, cropped: not the definition."""
    c = _hwc(content).astype(np.int64)
    pad = 2 ** LEVELS - 1
    v = np.pad(_hwc(style).astype(np.int64) - c, ((pad, pad), (pad, pad), (0, 0)), mode="edge")
    for axis in (1, 0):
        for k in range(LEVELS):
            r = 2 ** k
            v = np.roll(v, r, axis=axis) + 2 * v + np.roll(v, -r, axis=axis)      # wraps only inside the padding that is cropped
    H, W = c.shape[:2]
    v = v[pad:pad + H, pad:pad + W]
    out = np.clip((c * (1 << SHIFT) + v + (1 << (SHIFT - 1))) >> SHIFT, 0, 255).astype(np.uint8)
    return out.reshape(content.shape)


# ---- AdaIN -----------------------------------------------------------------------------------------------------------------------------------
def channel_stats(ch):
    """(mean, std) of one channel as the header defines them: integer sums, one division each, std = sqrt(var + 0.65025)."""
    flat = ch.reshape(-1).astype(np.int64)
    n = int(flat.size)
    s1 = int(flat.sum())
    s2 = int((flat * flat).sum())
    mean = s1 / n
    var = (n * s2 - s1 * s1) / (n * (n - 1)) if n > 1 else 0.0
    return mean, math.sqrt(var + 0.65025)


def adain_pixels(content, style):
    """Every pixel of the content through (x - mean_c) / std_c * std_s + mean_s in float64, rounded half up, clamped.  The style may have another
    size."""
    c, s = _hwc(content), _hwc(style)
    out = np.empty(c.shape, np.uint8)
    for ch in range(c.shape[2]):
        mean_c, std_c = channel_stats(c[:, :, ch])
        mean_s, std_s = channel_stats(s[:, :, ch])
        x = c[:, :, ch].astype(np.float64)
        out[:, :, ch] = np.clip(np.floor((x - mean_c) / std_c * std_s + mean_s + 0.5), 0, 255).astype(np.uint8)
    return out.reshape(content.shape)


def hist(img):
    a = _hwc(img)
    return np.stack([np.bincount(a[:, :, ch].reshape(-1), minlength=256) for ch in range(a.shape[2])]).astype(np.int64)
