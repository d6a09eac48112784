"""Numpy restatement of mdtile_resample_table / mdtile_resample_u8 (include/mdtile.h): Pillow's 8-bit Image.resize for Lanczos
and Nearest on "RGB" / "L" images, written with Python floats and math.sin (np.sin may differ from libm in the last bit).  The GPU tests compare
against it bit for bit; tests/test_resample_host.py holds it against Pillow itself and against the tables the library computes."""
import functools
import math

import numpy as np

NEAREST, LANCZOS = 0, 1         # MDTILE_RESAMPLE_*
PRECISION = 22


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def ksize(in_size, out_size, filt):
    if filt == NEAREST:
        return 1
    return int(math.ceil(3.0 * max(in_size / out_size, 1.0))) * 2 + 1


@functools.lru_cache(maxsize=None)
def tables(in_size, out_size, filt):
    """(coef [out, ksize] int32, zero past the taps; bounds [out, 2] int32 = (first source index, taps))."""
    k = ksize(in_size, out_size, filt)
    coef = np.zeros((out_size, k), np.int32)
    bounds = np.zeros((out_size, 2), np.int32)
    if filt == NEAREST:
        a = in_size / out_size
        xo = 0.5 * a
        for xx in range(out_size):          # the accumulated sum, as the affine transform walks it
            coef[xx, 0] = 1 << PRECISION
            bounds[xx] = (min(int(xo), in_size - 1), 1)
            xo += a
        return coef, bounds
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = 3.0 * fs
    ss = 1.0 / fs
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - xmin
        w = [lanczos((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            coef[xx, x] = int(-0.5 + v * (1 << PRECISION)) if v < 0 else int(0.5 + v * (1 << PRECISION))
        bounds[xx] = (xmin, n)
    return coef, bounds


def _pass(img, coef, bounds, axis):
    src = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((coef.shape[0],) + src.shape[1:], np.uint8)
    for xx in range(coef.shape[0]):
        x0, n = bounds[xx]
        acc = np.tensordot(coef[xx, :n].astype(np.int64), src[x0:x0 + n], axes=(0, 0)) + (1 << (PRECISION - 1))
        assert np.abs(acc).max() < 2 ** 31          # the definition sums in int32
        out[xx] = np.clip(acc >> PRECISION, 0, 255)
    return np.moveaxis(out, 0, axis)


def resize(img, out_h, out_w, filt):
    """img uint8 [H, W] or [H, W, 3] -> [out_h, out_w(, 3)]: horizontal pass first into bytes, then the vertical pass; Lanczos skips an axis
    that keeps its size, Nearest takes both always."""
    H, W = img.shape[:2]
    if filt == NEAREST or out_w != W:
        img = _pass(img, *tables(W, out_w, filt), axis=1)
    if filt == NEAREST or out_h != H:
        img = _pass(img, *tables(H, out_h, filt), axis=0)
    return np.ascontiguousarray(img)


# (H, W) -> (outH, outW), every pair checked against Pillow for both filters unless marked
PAIRS = [
    ((67, 131), (134, 262)), ((67, 131), (201, 393)),       # x2 and x3
    ((64, 96), (88, 120)),                                  # non-integer; Nearest's closed form gets 2055 pixels wrong here
    ((200, 300), (100, 150)),                               # / 2
    ((97, 53), (40, 200)),                                  # down on one axis, up on the other
    ((8, 8), (64, 64)),                                     # x8: the borders clip every window
    ((1, 40), (3, 80)), ((40, 1), (80, 5)),                 # an axis of size 1
    ((255, 257), (63, 65)),                                 # ksize 27
    ((33, 47), (33, 94)),                                   # one axis skipped
    ((128, 128), (136, 136)),                               # small non-integer upscale
    ((3, 3), (1, 1)),                                       # output of size 1
    ((500, 20), (37, 160)),                                 # ksize 83
]
NEAREST_ONLY = [((768, 512), (1384, 920))]                  # the closed form gets 7820 pixels wrong


def cases(extra=()):
    """[(src, dst, filt, rgb)] over PAIRS (+ extra pairs) x both filters x {RGB, L}, and NEAREST_ONLY for Nearest."""
    out = []
    for filt in (LANCZOS, NEAREST):
        for src, dst in PAIRS + list(extra) + (NEAREST_ONLY if filt == NEAREST else []):
            for rgb in (True, False):
                out.append((src, dst, filt, rgb))
    return out


def case_id(c):
    (h, w), (oh, ow), filt, rgb = c
    return f"{h}x{w}-{oh}x{ow}-{'lanczos' if filt == LANCZOS else 'nearest'}-{'rgb' if rgb else 'l'}"


def hard_edged(src):
    return (src[0] * src[1]) % 2 == 1


@functools.lru_cache(maxsize=None)
def make_image(src, rgb):
    """Random bytes, or where H * W is odd a hard 0 / 255 image (its Lanczos overshoot is what the clamp cuts)."""
    h, w = src
    rng = np.random.default_rng(h * 1009 + w * 7 + (3 if rgb else 1))
    shape = (h, w, 3) if rgb else (h, w)
    if hard_edged(src):
        img = np.where(rng.random(shape) < 0.5, 0, 255).astype(np.uint8)
    else:
        img = rng.integers(0, 256, size=shape).astype(np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def expected(src, dst, filt, rgb):
    want = resize(make_image(src, rgb), dst[0], dst[1], filt)
    want.setflags(write=False)
    return want
