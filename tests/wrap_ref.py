"""Numpy restatement of the wrap-x grid (include/mdtile.h: mdtile_plan_create_wrap_x) and of what the engine computes on it:
weight maps, tile gather and the MultiDiffusion / Mixture-of-Diffusers blend as the SEQUENTIAL fp32 `+=` loop over the tile list, with every
column index taken mod W.  Shared by tests/test_wrap_host.py and tests/test_gpu_wrap.py; nothing here touches the library.

Half dtypes follow the project's rule (tests/test_gpu_blend_matrix.py): callers round the inputs to the dtype, evaluate this fp32 restatement on
those values and round the result once."""
import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np


class Grid(NamedTuple):
    W: int
    H: int
    tw: int
    th: int
    ov: int
    cols: int
    rows: int
    xs: Tuple[int, ...]
    ys: Tuple[int, ...]
    boxes: Tuple[Tuple[int, int, int, int], ...]        # (x_c, y_r, tw, th), row-major (y outer); x_c + tw may pass W
    tile_bs: int
    batches: Tuple[Tuple[int, ...], ...]                # tile indices per batch


def clamp(W: int, H: int, tile_w: int, tile_h: int, overlap: int) -> Tuple[int, int, int]:
    """init_grid_bbox's clamp: tiles to the canvas, the overlap to min(REQUESTED tile sizes) - 4."""
    return min(tile_w, W), min(tile_h, H), max(0, min(overlap, min(tile_w, tile_h) - 4))


def plain_origins(extent: int, tile: int, ov: int) -> List[int]:
    """split_bboxes along one axis (the rows of a wrap-x grid are unchanged)."""
    n = max(1, math.ceil((extent - ov) / (tile - ov)))
    step = (extent - tile) / (n - 1) if n > 1 else 0.0
    return [min(int(i * step), extent - tile) for i in range(n)]


def grid(W: int, H: int, tile_w: int, tile_h: int, overlap: int, tile_bs: int) -> Optional[Grid]:
    """None when the effective tile is as wide as the canvas (the library refuses: a tile would meet itself)."""
    tw, th, ov = clamp(W, H, tile_w, tile_h, overlap)
    if tw >= W:
        return None
    cols = math.ceil(W / (tw - ov))
    xs = [int(c * float(W) / cols) for c in range(cols)]
    ys = plain_origins(H, th, ov)
    boxes = tuple((x, y, tw, th) for y in ys for x in xs)
    T = len(boxes)
    nb = math.ceil(T / tile_bs)
    bs = math.ceil(T / nb)
    batches = tuple(tuple(range(i * bs, min((i + 1) * bs, T))) for i in range(nb))
    return Grid(W, H, tw, th, ov, cols, len(ys), tuple(xs), tuple(ys), boxes, bs, batches)


def columns(g: Grid, x: int) -> np.ndarray:
    """The canvas columns of a tile with origin x."""
    return (x + np.arange(g.tw)) % g.W


def gaussian(tile_w: int, tile_h: int) -> np.ndarray:
    """gaussian_weights (tile_utils/utils.py:180-194): float64 profiles, both axes normalised by tile_w^2, cast to fp32."""
    var = 0.01

    def prof(t, mid):
        return np.exp(-(t - mid) * (t - mid) / (tile_w * tile_w) / (2 * var)) / np.sqrt(2 * np.pi * var)

    xp = [prof(x, (tile_w - 1) / 2) for x in range(tile_w)]
    yp = [prof(y, tile_h / 2) for y in range(tile_h)]
    return np.outer(yp, xp).astype(np.float32)


def weight_map(g: Grid, tile_weight: Optional[np.ndarray] = None) -> np.ndarray:
    """`weight[slicer] += init_weight` over the tile list (fp32, from zeros), columns mod W.  tile_weight None: 1.0 (MultiDiffusion)."""
    w = np.zeros((g.H, g.W), np.float32)
    tv = np.float32(1.0) if tile_weight is None else tile_weight.astype(np.float32)
    for (x, y, tw, th) in g.boxes:
        w[y:y + th, columns(g, x)] += tv          # no tile covers a column twice (tw < W): the fancy-indexed += adds once per element
    return w


def gather(g: Grid, x: np.ndarray, batch: int) -> np.ndarray:
    """x [N, C, H, W] -> [len(batch) * N, C, th, tw], tile-major."""
    parts = [np.take(x[:, :, y:y + th, :], bx + np.arange(tw), axis=-1, mode="wrap") for (bx, y, tw, th) in (g.boxes[t] for t in g.batches[batch])]
    return np.concatenate(parts, axis=0)


def blend(g: Grid, method: str, tiles: np.ndarray, N: int, weights: np.ndarray, tile_weight: Optional[np.ndarray] = None,
          rescale: Optional[np.ndarray] = None) -> np.ndarray:
    """tiles [T * N, C, th, tw] fp32 (tile-major, the model outputs of every tile in list order) -> [N, C, H, W] fp32.
    md : buf[slicer] += out_t;                     result = where(weights > 1, buf / weights, buf)
    mod: buf[slicer] += out_t * (tile_weight * rescale[slicer])"""
    tiles = tiles.astype(np.float32)
    buf = np.zeros((N, tiles.shape[1], g.H, g.W), np.float32)
    with np.errstate(all="ignore"):
        for t, (x, y, tw, th) in enumerate(g.boxes):
            cols = columns(g, x)
            v = tiles[t * N:(t + 1) * N]
            if method == "md":
                buf[:, :, y:y + th, cols] += v
            else:
                w = (tile_weight * rescale[y:y + th][:, cols]).astype(np.float32)
                buf[:, :, y:y + th, cols] += (v * w).astype(np.float32)
        if method == "md":
            return np.where(weights > 1, buf / weights, buf).astype(np.float32)
    return buf
