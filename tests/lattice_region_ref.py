"""Numpy restatement of region control under the jittered grid (include/mdtile.h: mdtile_blend_lattice_regions).  Everything is
the SEQUENTIAL loop: fp32 arrays, one rounded operation per step, no fused operations, grid tiles in list order and then the regions in list order.
It imports tests/grid_lattice_ref.py (the lattice, its boxes, its weight map, `gaussian`) and takes from tests/wrap_region_ref.py what fits a
canvas that does not wrap (the Region tuple, the background regions' weight map -- `index` mod the canvas is the identity for a rectangle inside
it); nothing of the product.

A region stays where the user put it; only the grid moves.  Region (x, y, w, h) covers the canvas pixels [y, y + h) x [x, x + w).
Half dtypes follow the project's rule: callers round the inputs to the dtype, evaluate this on those values and round the result once."""
from typing import Optional, Sequence

import numpy as np

import grid_lattice_ref as gl
import wrap_region_ref
from grid_lattice_ref import gaussian      # noqa: F401  (for the tests)
from wrap_region_ref import Region, region_w_map      # noqa: F401

F1 = np.float32(1.0)


def rect_valid(W: int, H: int, x: int, y: int, w: int, h: int) -> bool:
    """What the library accepts; everything else is refused by name."""
    return w >= 1 and h >= 1 and x >= 0 and y >= 0 and x + w <= W and y + h <= H


def blend(g: gl.Lattice, method: str, tiles: np.ndarray, N: int, regions: Sequence[Region] = (), region_w: Optional[np.ndarray] = None,
          tile_weight: Optional[np.ndarray] = None) -> np.ndarray:
    """tiles [T * N, C, th, tw] fp32 (tile-major, list order) -> [N, C, H, W] fp32.  region_w: the background regions' weight sum on the canvas
    (None: nothing is added to the grid's sum)."""
    tiles = tiles.astype(np.float32)
    C = tiles.shape[1]
    H, W = g.H, g.W
    for R in regions:
        assert rect_valid(W, H, R.x, R.y, R.w, R.h)
    gw = gl.weight_map(g, tile_weight if method == "mod" else None)
    with np.errstate(all="ignore"):
        wsum = gw if region_w is None else (gw + region_w.astype(np.float32)).astype(np.float32)
        resc = (F1 / wsum).astype(np.float32) if method == "mod" else None
        buf = np.zeros((N, C, H, W), np.float32)
        for r in range(g.rows):
            y0, y1, wy, ty = gl._piece(g.vs[r], g.ys[r], g.th, g.H)
            for c in range(g.cols):
                x0, x1, wx, tx = gl._piece(g.us[c], g.xs[c], g.tw, g.W)
                t = r * g.cols + c
                v = tiles[t * N:(t + 1) * N, :, ty:ty + y1 - y0, tx:tx + x1 - x0]
                if method == "md":
                    buf[:, :, y0:y1, x0:x1] += v
                else:
                    w = (tile_weight[wy:wy + y1 - y0, wx:wx + x1 - x0].astype(np.float32) * resc[y0:y1, x0:x1]).astype(np.float32)
                    buf[:, :, y0:y1, x0:x1] += (v * w).astype(np.float32)
        for R in regions:
            if R.mode != "bg":
                continue
            sl = (slice(R.y, R.y + R.h), slice(R.x, R.x + R.w))
            v = R.out.astype(np.float32)
            if method == "md":
                buf[(slice(None), slice(None)) + sl] += v
            else:
                w = (R.weight.astype(np.float32) * resc[sl]).astype(np.float32)
                buf[(slice(None), slice(None)) + sl] += (v * w).astype(np.float32)
        x_out = np.where(wsum > 1, buf / wsum, buf).astype(np.float32) if method == "md" else buf
        fbuf = np.zeros((N, C, H, W), np.float32)
        fmask = np.zeros((H, W), np.float32)
        fcnt = np.zeros((H, W), np.float32)
        for R in regions:
            if R.mode != "fg":
                continue
            sl = (slice(R.y, R.y + R.h), slice(R.x, R.x + R.w))
            fbuf[(slice(None), slice(None)) + sl] += R.out.astype(np.float32)
            fmask[sl] += R.weight.astype(np.float32)
            fcnt[sl] += F1
        many = fcnt > 1
        fbuf = np.where(many, fbuf / fcnt, fbuf).astype(np.float32)
        fmask = np.where(many, fmask / fcnt, fmask).astype(np.float32)
        comp = ((x_out * (F1 - fmask)).astype(np.float32) + (fbuf * fmask).astype(np.float32)).astype(np.float32)
        return np.where(fcnt > 0, comp, x_out).astype(np.float32)
