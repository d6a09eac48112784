"""Numpy restatement of the grid with per-axis wrap (include/mdtile.h: mdtile_plan_create_wrap) and of what the engine
computes on it: weight maps, tile gather and the MultiDiffusion / Mixture-of-Diffusers blend as the SEQUENTIAL fp32 `+=` loop over the tile list,
indexed with `rows[:, None], cols`, both taken mod the canvas (a plain tile never passes the edge, so the mod changes nothing on an axis that
does not wrap).  grid() defaults to the x-only panorama (wrap_x, wrap_y) = (1, 0).  Shared by tests/test_wrap_host.py, tests/test_torus_host.py,
tests/test_gpu_wrap.py and tests/test_gpu_torus.py; nothing here touches the library.

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
    boxes: Tuple[Tuple[int, int, int, int], ...]        # (x_c, y_r, tw, th), row-major (y outer); x_c + tw may pass W, y_r + th H
    tile_bs: int
    batches: Tuple[Tuple[int, ...], ...]                # tile indices per batch


def clamp(W: int, H: int, tile_w: int, tile_h: int, overlap: int) -> Tuple[int, int, int]:
    """init_grid_bbox's clamp: tiles to the canvas, the overlap to min(REQUESTED tile sizes) - 4."""
    return min(tile_w, W), min(tile_h, H), max(0, min(overlap, min(tile_w, tile_h) - 4))


def plain_origins(extent: int, tile: int, ov: int) -> List[int]:
    """split_bboxes along one axis (an axis that does not wrap)."""
    n = max(1, math.ceil((extent - ov) / (tile - ov)))
    step = (extent - tile) / (n - 1) if n > 1 else 0.0
    return [min(int(i * step), extent - tile) for i in range(n)]


def circle_origins(extent: int, tile: int, ov: int) -> List[int]:
    """A wrapped axis: n = ceil(extent / (tile - ov)) origins int(i * extent / n); tile i covers (origin + k) mod extent, k in [0, tile)."""
    n = math.ceil(extent / (tile - ov))
    return [int(i * float(extent) / n) for i in range(n)]


def grid(W: int, H: int, tile_w: int, tile_h: int, overlap: int, tile_bs: int, wrap_x: bool = True, wrap_y: bool = False) -> Optional[Grid]:
    """None where the library refuses: neither axis wrapped, or an effective tile as large as the canvas on a wrapped axis (it would meet itself)."""
    tw, th, ov = clamp(W, H, tile_w, tile_h, overlap)
    if not (wrap_x or wrap_y) or (wrap_x and tw >= W) or (wrap_y and th >= H):
        return None
    xs = circle_origins(W, tw, ov) if wrap_x else plain_origins(W, tw, ov)
    ys = circle_origins(H, th, ov) if wrap_y else plain_origins(H, th, ov)
    boxes = tuple((x, y, tw, th) for y in ys for x in xs)          # row-major, y outer
    T = len(boxes)
    nb = math.ceil(T / tile_bs)
    bs = math.ceil(T / nb)
    batches = tuple(tuple(range(i * bs, min((i + 1) * bs, T))) for i in range(nb))
    return Grid(W, H, tw, th, ov, len(xs), len(ys), tuple(xs), tuple(ys), boxes, bs, batches)


# id -> (W, H, requested tile_w, tile_h, overlap, wrap_x, wrap_y, tile_bs): the wrap-y and torus cases of tests/test_gpu_torus.py, planned
# without a GPU in tests/test_torus_host.py.  The overlap is clamped to min(requested tile sizes) - 4.
CASES = {
    # xs 0, 9, 18, 27; ys 0, 5, 11, 16; 2 - 6 tiles per pixel; neither extent a multiple of 4
    "torus_odd": (37, 22, 16, 12, 6, 1, 1, 4),
    # plain columns 0, 10, 20 under cyclic rows 0, 5, 10, 16, 21
    "ring_y": (36, 27, 16, 12, 6, 0, 1, 4),
    # origins 0, 8, 16, 24, 32 on both axes: 3 x 3 tiles on EVERY pixel; at a seam their list order is not their order on the circle
    "order40": (40, 40, 24, 24, 16, 1, 1, 2),
    # every origin a multiple of 4, 4 tiles per pixel: all quads on the vector path (and none when the batches are misaligned)
    "aligned64": (64, 48, 32, 32, 16, 1, 1, 3),
    # 13 x 13 tiles, 144 - 169 of them on one pixel; 43 batches
    "dense50": (50, 50, 48, 48, 44, 1, 1, 4),
    # non-square tiles, 1 - 4 tiles per pixel
    "rect44": (44, 30, 24, 12, 4, 1, 1, 4),
    # the launcher's 2- and 4-planes-per-thread forms (N * C = 8): H * ceil(W / 4) * 8 / 2 = 131072 at 512 x 256, / 4 = 131072 at 1024 x 256
    "planes2_512": (512, 256, 96, 96, 48, 1, 1, 8),
    "planes4_1024": (1024, 256, 128, 128, 8, 1, 1, 8),
}


def case_grid(case: str) -> Grid:
    W, H, tw, th, ov, wx, wy, bs = CASES[case]
    g = grid(W, H, tw, th, ov, bs, bool(wx), bool(wy))
    assert g is not None
    return g


def gaussian(tile_w: int, tile_h: int) -> np.ndarray:
    """gaussian_weights (tile_utils/utils.py:180-194): float64 profiles, both axes normalised by tile_w^2, cast to fp32."""
    var = 0.01

    def prof(t, mid):
        return np.exp(-(t - mid) * (t - mid) / (tile_w * tile_w) / (2 * var)) / np.sqrt(2 * np.pi * var)

    xp = [prof(x, (tile_w - 1) / 2) for x in range(tile_w)]
    yp = [prof(y, tile_h / 2) for y in range(tile_h)]
    return np.outer(yp, xp).astype(np.float32)


def columns(g: Grid, x: int) -> np.ndarray:
    """The canvas columns of a tile with origin x (mod W: a plain tile never passes the edge, so the mod changes nothing there)."""
    return (x + np.arange(g.tw)) % g.W


def rows(g: Grid, y: int) -> np.ndarray:
    """The canvas rows of a tile with origin y, as a column vector for `buf[..., rows, cols]`."""
    return ((y + np.arange(g.th)) % g.H)[:, None]


def weight_map(g: Grid, tile_weight: Optional[np.ndarray] = None) -> np.ndarray:
    """`weight[slicer] += init_weight` over the tile list (fp32, from zeros), both indices mod the canvas.  tile_weight None: 1.0."""
    w = np.zeros((g.H, g.W), np.float32)
    tv = np.float32(1.0) if tile_weight is None else tile_weight.astype(np.float32)
    for (x, y, tw, th) in g.boxes:
        w[rows(g, y), columns(g, x)] += tv        # no tile covers a pixel twice (tile < canvas on a wrapped axis): += adds once per element
    return w


def gather(g: Grid, x: np.ndarray, batch: int) -> np.ndarray:
    """x [N, C, H, W] -> [len(batch) * N, C, th, tw], tile-major."""
    parts = [x[:, :, rows(g, by), columns(g, bx)] for (bx, by, tw, th) in (g.boxes[t] for t in g.batches[batch])]
    return np.ascontiguousarray(np.concatenate(parts, axis=0))      # fancy indexing hands back a transposed view: make the layout plain


def blend(g: Grid, method: str, tiles: np.ndarray, N: int, weights: np.ndarray, tile_weight: Optional[np.ndarray] = None,
          rescale: Optional[np.ndarray] = None) -> np.ndarray:
    """tiles [T * N, C, th, tw] fp32 (tile-major, the model outputs of every tile in list order) -> [N, C, H, W] fp32.
    md : buf[slicer] += out_t;                     result = where(weights > 1, buf / weights, buf)
    mod: buf[slicer] += out_t * (tile_weight * rescale[slicer])"""
    tiles = tiles.astype(np.float32)
    buf = np.zeros((N, tiles.shape[1], g.H, g.W), np.float32)
    with np.errstate(all="ignore"):
        for t, (x, y, tw, th) in enumerate(g.boxes):
            rr, cc = rows(g, y), columns(g, x)
            v = tiles[t * N:(t + 1) * N]
            if method == "md":
                buf[:, :, rr, cc] += v
            else:
                w = (tile_weight * rescale[rr, cc]).astype(np.float32)
                buf[:, :, rr, cc] += (v * w).astype(np.float32)
        if method == "md":
            return np.where(weights > 1, buf / weights, buf).astype(np.float32)
    return buf


def blend_rows_in_circle_order(g: Grid, method: str, tiles: np.ndarray, N: int, weights: np.ndarray, tile_weight: Optional[np.ndarray] = None,
                               rescale: Optional[np.ndarray] = None) -> np.ndarray:
    """What a kernel would give that walked the covering tile ROWS of a canvas row from the start of their cyclic run (first, first + 1, ...
    mod rows) instead of in ascending index; columns inner and ascending, as in the list.  Evaluated per canvas row: the rows that cover it,
    rotated so that the run's first row leads."""
    tiles = tiles.astype(np.float32)
    out = np.zeros((N, tiles.shape[1], g.H, g.W), np.float32)
    with np.errstate(all="ignore"):
        for y in range(g.H):
            cover = [r for r in range(g.rows) if (y - g.ys[r]) % g.H < g.th]
            first = next((r for r in cover if (r - 1) % g.rows not in cover), cover[0])
            walk = sorted(cover, key=lambda r: (r - first) % g.rows)
            acc = np.zeros((N, tiles.shape[1], g.W), np.float32)
            for r in walk:
                ty = (y - g.ys[r]) % g.H
                for c in range(g.cols):
                    t = r * g.cols + c
                    cc = columns(g, g.xs[c])
                    v = tiles[t * N:(t + 1) * N, :, ty, :]
                    if method == "md":
                        acc[:, :, cc] += v
                    else:
                        acc[:, :, cc] += (v * (tile_weight[ty] * rescale[y, cc]).astype(np.float32)).astype(np.float32)
            out[:, :, y, :] = acc
        if method == "md":
            return np.where(weights > 1, out / weights, out).astype(np.float32)
    return out
