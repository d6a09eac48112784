"""Numpy restatement of region control on a wrap-around canvas (include/mdtile.h: mdtile_gather_rect_wrap,
mdtile_weight_map_add_rect_wrap, mdtile_region_noise_wrap, mdtile_blend_wrap_regions) and of the host's rectangle rule (tile_utils.region_rect).
Everything is the SEQUENTIAL loop: fp32 arrays, one rounded operation per step, no fused operations, tiles and regions in list order, every index
taken mod the canvas.  It imports tests/wrap_ref.py and tests/shift_ref.py and nothing of the product.

A rectangle (x, y, w, h) covers the canvas pixels ((y + i) mod H, (x + j) mod W); its tensors are dense [.., h, w] whether or not it crosses a seam.
Half dtypes follow the project's rule: callers round the inputs to the dtype, evaluate this on those values and round the result once."""
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

import shift_ref as sr
import wrap_ref as wr

F1 = np.float32(1.0)


class Region(NamedTuple):
    x: int
    y: int
    w: int
    h: int
    mode: str                       # "bg" | "fg"
    out: Optional[np.ndarray]       # [N, C, h, w] fp32: the model's output for the region
    weight: Optional[np.ndarray]    # [h, w] fp32: fg = the feather mask; bg + mod = the RAW Gaussian; bg + md = None


def rect_rule(fx: float, fy: float, fw: float, fh: float, W: int, H: int, wrap_x: bool, wrap_y: bool) -> Tuple[int, int, int, int]:
    """The host rule: an axis that does not wrap clips at the edge (upstream), an axis that wraps takes the origin mod the extent."""
    if wrap_x:
        x, w = int(fx * W) % W, min(W, math.ceil(fw * W))
    else:
        x = max(0, int(fx * W))
        w = min(W - x, math.ceil(fw * W))
    if wrap_y:
        y, h = int(fy * H) % H, min(H, math.ceil(fh * H))
    else:
        y = max(0, int(fy * H))
        h = min(H - y, math.ceil(fh * H))
    return x, y, w, h


def rect_valid(W: int, H: int, x: int, y: int, w: int, h: int, wrap_x: bool, wrap_y: bool) -> bool:
    """What the library accepts; everything else is refused by name."""
    return (0 <= x < W and 0 <= y < H and 0 < w <= W and 0 < h <= H and (wrap_x or x + w <= W) and (wrap_y or y + h <= H))


def index(W: int, H: int, x: int, y: int, w: int, h: int):
    """(rows as a column vector, columns) of the rectangle on the canvas, for `a[..., rows, cols]`."""
    return ((y + np.arange(h)) % H)[:, None], (x + np.arange(w)) % W


def gather_rect(x_in: np.ndarray, x: int, y: int, w: int, h: int) -> np.ndarray:
    H, W = x_in.shape[-2:]
    rr, cc = index(W, H, x, y, w, h)
    return np.ascontiguousarray(x_in[..., rr, cc])


def weight_map_add_rect(weights: np.ndarray, x: int, y: int, w: int, h: int, rect_w: Optional[np.ndarray] = None, scalar: float = 1.0) -> None:
    """In place, fp32.  w <= W and h <= H: no pixel is indexed twice, so the fancy `+=` adds once per element."""
    H, W = weights.shape
    rr, cc = index(W, H, x, y, w, h)
    weights[rr, cc] += np.float32(scalar) if rect_w is None else rect_w.astype(np.float32)


def region_w_map(W: int, H: int, method: str, regions: Sequence[Region]) -> np.ndarray:
    """The background regions' weight sum on the canvas, from zeros, in list order: 1.0 each (md) or the raw Gaussian (mod)."""
    m = np.zeros((H, W), np.float32)
    for R in regions:
        if R.mode == "bg":
            weight_map_add_rect(m, R.x, R.y, R.w, R.h, None if method == "md" else R.weight)
    return m


def region_noise(noise: np.ndarray, regions) -> np.ndarray:
    """regions: [(x, y, w, h, mode, rand [1, C, h, w])].  Per layer the sum and the hit count in list order, averaged where the count > 1;
    the background layer pasted where its count > 0, the foreground layer on top.  Returns a new array."""
    N, C, H, W = noise.shape
    s = {m: np.zeros((C, H, W), np.float32) for m in ("bg", "fg")}
    n = {m: np.zeros((H, W), np.float32) for m in ("bg", "fg")}
    for (x, y, w, h, mode, rand) in regions:
        rr, cc = index(W, H, x, y, w, h)
        s[mode][:, rr, cc] += rand[0].astype(np.float32)
        n[mode][rr, cc] += F1
    out = noise.astype(np.float32).copy()
    with np.errstate(all="ignore"):
        for mode in ("bg", "fg"):
            layer = np.where(n[mode] > 1, s[mode] / n[mode], s[mode]).astype(np.float32)
            out = np.where(n[mode] > 0, layer[None], out)
    return out.astype(np.float32)


def blend(g: wr.Grid, method: str, tiles: Optional[np.ndarray], N: int, C: int, sx: int, sy: int, grid_w: Optional[np.ndarray], region_w: np.ndarray,
          regions: Sequence[Region], tile_weight: Optional[np.ndarray] = None) -> np.ndarray:
    """tiles [T * N, C, th, tw] fp32 in list order, or None (no grid is drawn; grid_w None too).  grid_w: the grid's weight sum in PLAN
    coordinates; region_w: the background regions' on the CANVAS.  -> [N, C, H, W] fp32 on the canvas."""
    H, W = g.H, g.W
    assert (tiles is None) == (grid_w is None)
    with np.errstate(all="ignore"):
        gw = np.zeros((H, W), np.float32) if grid_w is None else np.roll(grid_w.astype(np.float32), (sy, sx), axis=(0, 1))      # plan -> canvas
        wsum = (gw + region_w.astype(np.float32)).astype(np.float32)
        resc = (F1 / wsum).astype(np.float32) if method == "mod" else None
        buf = np.zeros((N, C, H, W), np.float32)
        if tiles is not None:
            tiles = tiles.astype(np.float32)
            for t, (x, y, tw, th) in enumerate(sr.boxes(g, sx, sy)):          # the displaced boxes, list order unchanged
                rr, cc = index(W, H, x, y, tw, th)
                v = tiles[t * N:(t + 1) * N]
                if method == "md":
                    buf[:, :, rr, cc] += v
                else:
                    w = (tile_weight.astype(np.float32) * resc[rr, cc]).astype(np.float32)
                    buf[:, :, rr, cc] += (v * w).astype(np.float32)
        for R in regions:
            if R.mode != "bg":
                continue
            rr, cc = index(W, H, R.x, R.y, R.w, R.h)
            v = R.out.astype(np.float32)
            if method == "md":
                buf[:, :, rr, cc] += v
            else:
                w = (R.weight.astype(np.float32) * resc[rr, cc]).astype(np.float32)
                buf[:, :, rr, cc] += (v * w).astype(np.float32)
        x_out = np.where(wsum > 1, buf / wsum, buf).astype(np.float32) if method == "md" else buf
        fbuf = np.zeros((N, C, H, W), np.float32)
        fmask = np.zeros((H, W), np.float32)
        fcnt = np.zeros((H, W), np.float32)
        for R in regions:
            if R.mode != "fg":
                continue
            rr, cc = index(W, H, R.x, R.y, R.w, R.h)
            fbuf[:, :, rr, cc] += R.out.astype(np.float32)
            fmask[rr, cc] += R.weight.astype(np.float32)
            fcnt[rr, cc] += F1
        many = fcnt > 1
        fbuf = np.where(many, fbuf / fcnt, fbuf).astype(np.float32)
        fmask = np.where(many, fmask / fcnt, fmask).astype(np.float32)
        comp = ((x_out * (F1 - fmask)).astype(np.float32) + (fbuf * fmask).astype(np.float32)).astype(np.float32)
        return np.where(fcnt > 0, comp, x_out).astype(np.float32)


def rolled(regions: Sequence[Region], a: int, b: int, W: int, H: int) -> List[Region]:
    """The regions with their origins moved by (a, b) on the circle; tensors and list order unchanged."""
    return [R._replace(x=(R.x + a) % W, y=(R.y + b) % H) for R in regions]
