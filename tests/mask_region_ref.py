"""Numpy restatement of free-form mask regions (include/mdtile.h: mdtile_mask_cover_u8, mdtile_mask_region,
mdtile_blend_mask_regions, mdtile_region_noise_masked).  Everything is the SEQUENTIAL loop: fp32 arrays, one rounded operation per step, no fused
operations, tiles and regions in list order -- upstream's loops with one change: a region's `+=` runs over the pixels of its rectangle that its
boolean cover selects, not over the whole rectangle.  It imports nothing of the product.

A region's tensors are dense [.., h, w] over its rectangle; cover None means the whole rectangle.  A pixel a region does not cover is never
indexed, so whatever its output or weight holds there cannot reach a result.  Half dtypes follow the project's rule: callers round the inputs to
the dtype, evaluate this on those values and round the result once."""
from typing import NamedTuple, Optional, Sequence, Tuple

import numpy as np

F1 = np.float32(1.0)


class Region(NamedTuple):
    x: int
    y: int
    w: int
    h: int
    mode: str                       # "bg" | "fg"
    out: Optional[np.ndarray]       # [N, C, h, w] fp32: the model's output for the region
    weight: Optional[np.ndarray]    # [h, w] fp32: fg = the feather; bg + mod = the Gaussian PREMULTIPLIED by the reciprocal map; bg + md = None
    cover: Optional[np.ndarray]     # [h, w] bool / uint8, or None = the whole rectangle


def covered(R) -> np.ndarray:
    return np.ones((R.h, R.w), bool) if R.cover is None else np.asarray(R.cover).reshape(R.h, R.w) != 0


# ---- mask -> coverage, box ------------------------------------------------------------------------------------------------------------
def cover_u8(mask: np.ndarray, W: int, H: int) -> Tuple[np.ndarray, list]:
    """mask uint8 [Hm, Wm], Hm >= H, Wm >= W -> (cover uint8 [H, W], [xmin, ymin, xmax + 1, ymax + 1, count]).  Python integers throughout."""
    Hm, Wm = mask.shape
    assert Hm >= H and Wm >= W
    cover = np.zeros((H, W), np.uint8)
    for y in range(H):
        r0, r1 = y * Hm // H, (y + 1) * Hm // H
        for x in range(W):
            c0, c1 = x * Wm // W, (x + 1) * Wm // W
            box = mask[r0:r1, c0:c1]
            s, n = int(box.astype(np.int64).sum()), box.size
            assert n > 0
            cover[y, x] = 1 if 2 * s >= 255 * n else 0
    return cover, box_of(cover)


def box_of(cover: np.ndarray) -> list:
    ys, xs = np.nonzero(cover)
    if len(ys) == 0:
        return [0, 0, 0, 0, 0]
    return [int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1, int(len(ys))]


# ---- coverage -> the region's dense cover and feather ---------------------------------------------------------------------------------
def radius(w: int, h: int, ratio: float) -> int:
    return int(min(w // 2, h // 2) * ratio)


def chessboard(rcover: np.ndarray) -> np.ndarray:
    """k [h, w] int: for a covered cell the chessboard distance max(|di|, |dj|) to the nearest cell that is not covered, cells outside the
    rectangle counting as not covered (k >= 1); 0 for a cell that is not covered.  By definition: the minimum over every such cell."""
    h, w = rcover.shape
    pad = np.zeros((h + 2, w + 2), bool)
    pad[1:-1, 1:-1] = rcover != 0
    holes = np.argwhere(~pad)                      # in padded coordinates: the frame stands for the whole outside (the nearest outside cell is on it)
    k = np.zeros((h, w), np.int64)
    for i in range(h):
        for j in range(w):
            if pad[i + 1, j + 1]:
                k[i, j] = int(np.max(np.abs(holes - (i + 1, j + 1)), axis=1).min())
    return k


def feather(rcover: np.ndarray, ratio: float) -> np.ndarray:
    """[h, w] fp32: 0.0 where not covered; else with d = k - 1: 1.0 where d >= R, (d / R)^2 in double, rounded to fp32, below."""
    h, w = rcover.shape
    R = radius(w, h, ratio)
    k = chessboard(rcover)
    out = np.zeros((h, w), np.float32)
    for i in range(h):
        for j in range(w):
            if k[i, j] > 0:
                d = int(k[i, j]) - 1
                out[i, j] = 1.0 if d >= R else np.float32((d / R) ** 2)
    return out


def region_tensors(cover: np.ndarray, x: int, y: int, w: int, h: int, ratio: Optional[float]):
    """(rcover uint8 [h, w] of 0 / 1, feather fp32 [h, w] or None when ratio is None)."""
    rcover = (cover[y:y + h, x:x + w] != 0).astype(np.uint8)
    return rcover, None if ratio is None else feather(rcover, ratio)


# ---- the weight sums, as the delegates build them -------------------------------------------------------------------------------------
def weight_sum(grid_w: np.ndarray, method: str, regions: Sequence[Region], gaussians=None) -> np.ndarray:
    """grid_w [H, W] (zeros when no grid is drawn) plus, per BG region in list order, its cover as 0.0 / 1.0 (md) or gaussians[k] * cover (mod)."""
    m = grid_w.astype(np.float32).copy()
    for k, R in enumerate(regions):
        if R.mode != "bg":
            continue
        c = covered(R).astype(np.float32)
        add = c if method == "md" else (gaussians[k].astype(np.float32) * c).astype(np.float32)
        m[R.y:R.y + R.h, R.x:R.x + R.w] += add
    return m


def premultiplied(gaussian: np.ndarray, R, rescale: np.ndarray) -> np.ndarray:
    """A BG region's weight under Mixture of Diffusers as mdtile_blend takes it: (gaussian * cover) * rescale[rect].  0 * inf = NaN under a pixel
    nobody paints -- which the region does not cover, so it is never read."""
    with np.errstate(all="ignore"):
        g = (gaussian.astype(np.float32) * covered(R).astype(np.float32)).astype(np.float32)
        return (g * rescale[R.y:R.y + R.h, R.x:R.x + R.w].astype(np.float32)).astype(np.float32)


# ---- the blend ------------------------------------------------------------------------------------------------------------------------
def blend(W: int, H: int, boxes, method: str, tiles: Optional[np.ndarray], N: int, C: int, regions: Sequence[Region],
          weights: Optional[np.ndarray] = None, tile_weight: Optional[np.ndarray] = None, rescale: Optional[np.ndarray] = None) -> np.ndarray:
    """boxes [(x, y, tw, th)] in list order with tiles [T * N, C, th, tw] fp32, or tiles None: regions only.  weights (md) / rescale (mod): the
    host's maps [H, W].  -> [N, C, H, W] fp32."""
    with np.errstate(all="ignore"):
        buf = np.zeros((N, C, H, W), np.float32)
        if tiles is not None:
            tiles = tiles.astype(np.float32)
            for t, (x, y, tw, th) in enumerate(boxes):
                v = tiles[t * N:(t + 1) * N]
                if method == "md":
                    buf[:, :, y:y + th, x:x + tw] += v
                else:
                    w = (tile_weight.astype(np.float32) * rescale[y:y + th, x:x + tw].astype(np.float32)).astype(np.float32)
                    buf[:, :, y:y + th, x:x + tw] += (v * w).astype(np.float32)
        for R in regions:
            if R.mode != "bg":
                continue
            m = covered(R)
            sl = buf[:, :, R.y:R.y + R.h, R.x:R.x + R.w]      # a view: the assignment below lands in buf
            v = R.out.astype(np.float32)[:, :, m]
            if method == "md":
                sl[:, :, m] = (sl[:, :, m] + v).astype(np.float32)
            else:
                sl[:, :, m] = (sl[:, :, m] + (v * R.weight.astype(np.float32)[m]).astype(np.float32)).astype(np.float32)
        x_out = np.where(weights > 1, buf / weights.astype(np.float32), buf).astype(np.float32) if method == "md" else buf
        fbuf = np.zeros((N, C, H, W), np.float32)
        fmask = np.zeros((H, W), np.float32)
        fcnt = np.zeros((H, W), np.float32)
        for R in regions:
            if R.mode != "fg":
                continue
            m = covered(R)
            ys, xs = slice(R.y, R.y + R.h), slice(R.x, R.x + R.w)
            fb = fbuf[:, :, ys, xs]
            fb[:, :, m] = (fb[:, :, m] + R.out.astype(np.float32)[:, :, m]).astype(np.float32)
            fm, fc = fmask[ys, xs], fcnt[ys, xs]
            fm[m] = (fm[m] + R.weight.astype(np.float32)[m]).astype(np.float32)
            fc[m] = fc[m] + F1
        many = fcnt > 1
        fbuf = np.where(many, fbuf / fcnt, fbuf).astype(np.float32)
        fmask = np.where(many, fmask / fcnt, fmask).astype(np.float32)
        comp = ((x_out * (F1 - fmask)).astype(np.float32) + (fbuf * fmask).astype(np.float32)).astype(np.float32)
        return np.where(fcnt > 0, comp, x_out).astype(np.float32)


# ---- the noise ------------------------------------------------------------------------------------------------------------------------
def region_noise(noise: np.ndarray, regions) -> np.ndarray:
    """regions: [(x, y, w, h, mode, rand [1, C, h, w], cover or None)].  Per layer the sum and the hit count over the COVERING regions in list
    order, averaged where the count > 1; the background layer pasted where its count > 0, the foreground layer on top.  Returns a new array."""
    N, C, H, W = noise.shape
    s = {m: np.zeros((C, H, W), np.float32) for m in ("bg", "fg")}
    n = {m: np.zeros((H, W), np.float32) for m in ("bg", "fg")}
    for (x, y, w, h, mode, rand, cover) in regions:
        m = np.ones((h, w), bool) if cover is None else np.asarray(cover).reshape(h, w) != 0
        sv, nv = s[mode][:, y:y + h, x:x + w], n[mode][y:y + h, x:x + w]
        sv[:, m] = (sv[:, m] + rand[0].astype(np.float32)[:, m]).astype(np.float32)
        nv[m] = nv[m] + F1
    out = noise.astype(np.float32).copy()
    with np.errstate(all="ignore"):
        for mode in ("bg", "fg"):
            layer = np.where(n[mode] > 1, s[mode] / n[mode], s[mode]).astype(np.float32)
            out = np.where(n[mode] > 0, layer[None], out)
    return out.astype(np.float32)
