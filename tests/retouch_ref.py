"""numpy restatement of mdtile_retouch_mask / mdtile_renoise_resize (include/mdtile.h) and the test image generator of the
renoise-mask tests.  A helper module, not a conftest: tests import it by name.

The restatement follows the definition, not the kernels: integer window sums through an explicit triangle-wave index map (no np.pad, so the
border rule is stated here and nowhere else), then the fp32 operation sequence one numpy op at a time, then upstream's quantisation as
trunc -> int32 -> & 255 (what numpy's astype(uint8) does on x86 for the values that occur)."""
import numpy as np


def reflect101(idx, n):
    """BORDER_REFLECT_101 for any integer index: the triangle wave of period 2 (n - 1); n == 1 -> 0."""
    idx = np.asarray(idx, dtype=np.int64)
    if n == 1:
        return np.zeros_like(idx)
    p = 2 * (n - 1)
    r = np.mod(idx, p)              # numpy's mod is non-negative for a positive modulus
    return np.where(r < n, r, p - r)


def grey(img):
    """[H, W] bytes as they are; [H, W, 3] RGB -> PIL's convert("L"): (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    img = np.asarray(img)
    assert img.dtype == np.uint8
    if img.ndim == 2:
        return img.astype(np.int64)
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16


def _window_sums_1d(a, k, axis):
    """Sums over index - k//2 .. index - k//2 + k - 1 along `axis`, reflected, exact in int64."""
    n = a.shape[axis]
    src = reflect101(np.arange(-(k // 2), n - (k // 2) + k - 1), n)          # every index any window touches: n + k - 1 of them
    ext = np.take(a, src, axis=axis)
    c = np.cumsum(ext, axis=axis, dtype=np.int64)
    zero = np.zeros_like(np.take(c, [0], axis=axis))
    c = np.concatenate([zero, c], axis=axis)
    hi = np.take(c, np.arange(k, n + k), axis=axis)
    lo = np.take(c, np.arange(0, n), axis=axis)
    return hi - lo


def window_sums(L, k):
    """(S1, S2) = sums of L and L^2 over the k x k window of every pixel, int64."""
    L = L.astype(np.int64)
    s1 = _window_sums_1d(_window_sums_1d(L, k, 1), k, 0)
    s2 = _window_sums_1d(_window_sums_1d(L * L, k, 1), k, 0)
    return s1, s2


def retouch_mask(img, k):
    """The mask mdtile_retouch_mask is defined to produce: [H, W] float32."""
    f = np.float32
    L = grey(img)
    s1, s2 = window_sums(L, k)
    n = float(k) * float(k)
    x = L.astype(np.float32) / f(255.0)
    mean = (s1.astype(np.float64) / (255.0 * n)).astype(np.float32)
    msq = (s2.astype(np.float64) / (65025.0 * n)).astype(np.float32)
    var = msq - mean * mean
    a = var / (var + f(0.01))
    b = mean - a * mean
    gf = ((a * x + b) - x) * f(255.0)
    assert gf.dtype == np.float32
    q = np.trunc(gf).astype(np.int32) & 255
    return q.astype(np.float32) / f(255.0)


def _taps(n_in, n_out):
    f = np.float32
    scale = f(n_in) / f(n_out)
    dst = np.arange(n_out, dtype=np.float32)
    src = np.maximum(scale * (dst + f(0.5)) - f(0.5), f(0))
    i0 = src.astype(np.int32)
    i1 = np.minimum(i0 + 1, n_in - 1)
    l1 = src - i0.astype(np.float32)
    l0 = f(1) - l1
    assert src.dtype == l1.dtype == l0.dtype == np.float32
    return i0, i1, l0, l1


def bilinear(mask, size):
    """torch's bilinear resize with align_corners=False, op by op in fp32 (the order of mdtile_renoise_resize)."""
    mask = np.asarray(mask, dtype=np.float32)
    h, w = size
    y0, y1, ly0, ly1 = _taps(mask.shape[0], h)
    x0, x1, lx0, lx1 = _taps(mask.shape[1], w)
    ly0, ly1 = ly0[:, None], ly1[:, None]
    top = lx0 * mask[y0][:, x0] + lx1 * mask[y0][:, x1]
    bot = lx0 * mask[y1][:, x0] + lx1 * mask[y1][:, x1]
    out = ly0 * top + ly1 * bot
    assert out.dtype == np.float32
    return out


def renoise_resize(mask, size, strength):
    f = np.float32
    return np.clip((f(1) - bilinear(mask, size)) * f(strength), f(0), f(1))


def make_image(H, W, seed=0, rgb=True):
    """uint8 [H, W, 3] (or [H, W]): smooth gradients, fine texture, exactly flat patches and patches saturated at 0 and at 255 -- every
    regime of the filter (var ~ 0, var >> eps, gf on both sides of 0) and plenty of pixels near a quantisation threshold."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ch = []
    for c in range(3 if rgb else 1):
        g = 127.5 + 90.0 * np.sin(xx / (17.0 + 5 * c) + 0.3 * c) * np.cos(yy / (23.0 - 3 * c)) + 0.12 * (xx - yy)
        tex = rng.integers(-40, 41, size=(H, W)) * (((xx // 16 + yy // 16) % 3) == 0)     # fine texture on a third of the 16-px cells
        ch.append(g + tex)
    img = np.stack(ch, axis=-1)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    h4, w4 = max(1, H // 4), max(1, W // 4)
    img[:h4, :w4] = 93                               # exactly flat
    img[:h4, W - w4:] = 0                            # saturated low
    img[H - h4:, :w4] = 255                          # saturated high
    img[H - h4:, W - w4:] = (200, 40, 120) if rgb else 131   # flat, distinct channels
    return img if rgb else img[..., 0]
