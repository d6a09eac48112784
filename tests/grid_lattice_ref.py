"""Numpy restatement of the jittered tile grid on a plain canvas (include/mdtile.h: mdtile_lattice_make, mdtile_lattice_bboxes,
mdtile_lattice_weight_map, mdtile_gather_all_lattice, mdtile_blend_lattice), written from the definition and independent of the engine:

    per axis  stride st = tile - overlap, shift s in [1, st]:  lattice origins u_k = s - st + k st for k = 0, 1, ... up to the first k with
              u_k + tile >= extent;  the box the model runs on is pushed inside, x'_k = min(max(u_k, 0), extent - tile); a tile as large as the
              canvas: one tile at 0, the shift is ignored
    a tile is read at its pushed-in box and contributes where its LATTICE box lies (clipped to the canvas)

The axis is the explicit loop, not the closed forms; weight map and blend are the sequential `+=` loop over the tile list in np.float32.
Shared by tests/test_grid_lattice_host.py and tests/test_gpu_lattice.py; nothing here touches the library.

Half dtypes follow the project's rule (tests/test_gpu_blend_matrix.py): callers round the inputs to the dtype, evaluate this fp32 restatement on
those values and round the result once."""
import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np

import shift_ref
from wrap_ref import clamp, gaussian      # noqa: F401  (gaussian: the Mixture-of-Diffusers tile weight, for the tests)


class Lattice(NamedTuple):
    W: int
    H: int
    tw: int
    th: int
    ov: int
    stride_x: int
    stride_y: int
    sx: int                                             # 0 on an axis that does not move
    sy: int
    us: Tuple[int, ...]                                 # lattice column origins (u_0 <= 0)
    vs: Tuple[int, ...]                                 # lattice row origins
    xs: Tuple[int, ...]                                 # pushed-in column origins
    ys: Tuple[int, ...]
    cols: int
    rows: int
    boxes: Tuple[Tuple[int, int, int, int], ...]        # pushed-in (x'_c, y'_r, tw, th), row-major (y outer)
    tile_bs: int
    batches: Tuple[Tuple[int, ...], ...]                # tile indices per batch


def axis(extent: int, tile: int, stride: int, s: int) -> Tuple[List[int], List[int]]:
    """(lattice origins, pushed-in origins) of one axis, by walking the lattice until a tile reaches the far edge."""
    if tile >= extent:
        return [0], [0]
    assert 1 <= s <= stride
    us = []
    u = s - stride
    while True:
        us.append(u)
        if u + tile >= extent:
            break
        u += stride
    return us, [min(max(u, 0), extent - tile) for u in us]


def lattice(W: int, H: int, tile_w: int, tile_h: int, overlap: int, tile_bs: int, sx: int, sy: int) -> Optional[Lattice]:
    """None where the library refuses: the overlap equals a clamped tile size, or a shift outside [1, stride] on an axis that moves."""
    tw, th, ov = clamp(W, H, tile_w, tile_h, overlap)
    if tw - ov == 0 or th - ov == 0:
        return None
    stx, sty = tw - ov, th - ov
    if (tw < W and not 1 <= sx <= stx) or (th < H and not 1 <= sy <= sty):
        return None
    us, xs = axis(W, tw, stx, sx)
    vs, ys = axis(H, th, sty, sy)
    boxes = tuple((x, y, tw, th) for y in ys for x in xs)
    T = len(boxes)
    nb = math.ceil(T / tile_bs)
    bs = math.ceil(T / nb)
    batches = tuple(tuple(range(i * bs, min((i + 1) * bs, T))) for i in range(nb))
    return Lattice(W, H, tw, th, ov, stx, sty, sx if tw < W else 0, sy if th < H else 0, tuple(us), tuple(vs), tuple(xs), tuple(ys), len(xs), len(ys),
                   boxes, bs, batches)


def rest(W: int, H: int, tile_w: int, tile_h: int, overlap: int) -> Tuple[int, int]:
    """(stride_x, stride_y): the shift of the lattice at rest."""
    tw, th, ov = clamp(W, H, tile_w, tile_h, overlap)
    return tw - ov, th - ov


def shift(seed: int, step: int, axis_: int, stride: int) -> int:
    """--mdtile-grid-jitter's shift along one axis at one sampler step, in [1, stride]: grid_shift's integers moved up by one."""
    return 1 + shift_ref.shift(seed, step, axis_, stride)


# (seed, step, axis, stride) -> shift, computed once from the splitmix64 formula of tests/shift_ref.py with Python integers
PINNED = {
    (0, 0, 0, 128): 48,
    (0, 0, 1, 64): 53,
    (0, 1, 0, 128): 80,
    (1234567, 0, 0, 37): 25,
    (1234567, 0, 1, 22): 12,
    (1234567, 19, 0, 1024): 823,
    (2 ** 63, 3, 0, 2): 2,
    (-1, 5, 1, 1000): 528,
}


def step_shift(W: int, H: int, tile_w: int, tile_h: int, overlap: int, seed: int, step: int) -> Tuple[int, int]:
    """(sx, sy) of a job's step: only the axes whose tile is smaller than the canvas move."""
    tw, th, ov = clamp(W, H, tile_w, tile_h, overlap)
    return (shift(seed, step, 0, tw - ov) if tw < W else 0, shift(seed, step, 1, th - ov) if th < H else 0)


def _piece(u: int, p: int, tile: int, extent: int) -> Tuple[int, int, int, int]:
    """One axis of one tile: the canvas coordinates [lo, hi) its lattice box covers, and where they start inside the lattice box (the tile-weight
    map) and inside the pushed-in box (the tile's values)."""
    lo, hi = max(u, 0), min(u + tile, extent)
    return lo, hi, lo - u, lo - p


def weight_map(g: Lattice, tile_weight: Optional[np.ndarray] = None) -> np.ndarray:
    """`weight[lattice box] += tile weight` over the tile list (fp32, from zeros); the tile weight is indexed in LATTICE coordinates.  None: 1.0."""
    w = np.zeros((g.H, g.W), np.float32)
    for r in range(g.rows):
        y0, y1, wy, _ = _piece(g.vs[r], g.ys[r], g.th, g.H)
        for c in range(g.cols):
            x0, x1, wx, _ = _piece(g.us[c], g.xs[c], g.tw, g.W)
            if tile_weight is None:
                w[y0:y1, x0:x1] += np.float32(1.0)
            else:
                w[y0:y1, x0:x1] += tile_weight[wy:wy + y1 - y0, wx:wx + x1 - x0].astype(np.float32)
    return w


def gather(g: Lattice, x: np.ndarray, batch: int) -> np.ndarray:
    """x [N, C, H, W] -> [len(batch) * N, C, th, tw], tile-major: the pushed-in boxes."""
    parts = [x[:, :, by:by + th, bx:bx + tw] for (bx, by, tw, th) in (g.boxes[t] for t in g.batches[batch])]
    return np.ascontiguousarray(np.concatenate(parts, axis=0))


def blend(g: Lattice, method: str, tiles: np.ndarray, N: int, tile_weight: Optional[np.ndarray] = None) -> np.ndarray:
    """tiles [T * N, C, th, tw] fp32 (tile-major, the model outputs of every tile in list order) -> [N, C, H, W] fp32.
    md : buf[lattice box] += out_t[pushed-in coordinates];             result = where(wsum > 1, buf / wsum, buf)
    mod: buf[lattice box] += out_t[...] * (tile_weight[lattice coordinates] * (1 / wsum)[lattice box])"""
    tiles = tiles.astype(np.float32)
    buf = np.zeros((N, tiles.shape[1], g.H, g.W), np.float32)
    wsum = weight_map(g, tile_weight if method == "mod" else None)
    with np.errstate(all="ignore"):
        rinv = (np.float32(1.0) / wsum).astype(np.float32)
        for r in range(g.rows):
            y0, y1, wy, ty = _piece(g.vs[r], g.ys[r], g.th, g.H)
            for c in range(g.cols):
                x0, x1, wx, tx = _piece(g.us[c], g.xs[c], g.tw, g.W)
                t = r * g.cols + c
                v = tiles[t * N:(t + 1) * N, :, ty:ty + y1 - y0, tx:tx + x1 - x0]
                if method == "md":
                    buf[:, :, y0:y1, x0:x1] += v
                else:
                    w = (tile_weight[wy:wy + y1 - y0, wx:wx + x1 - x0].astype(np.float32) * rinv[y0:y1, x0:x1]).astype(np.float32)
                    buf[:, :, y0:y1, x0:x1] += (v * w).astype(np.float32)
        if method == "md":
            return np.where(wsum > 1, buf / wsum, buf).astype(np.float32)
    return buf
