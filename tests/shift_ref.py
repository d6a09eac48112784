"""Numpy restatement of the shifted wrap-around grid (include/mdtile.h: mdtile_gather_all_shift / mdtile_blend_shift): np.roll
around the gather, the blend and the weight map of tests/wrap_ref.py, the shift function of --mdtile-grid-shift in Python integers, and the
shifted boxes.  Displacing every tile origin of a wrap plan by (sx, sy) on the circle does not change which tile indices cover a pixel, or in
which order; it moves the pixel:

    gather_s(x)    = gather(plan, roll(x, (-sy, -sx)))
    blend_s(tiles) = roll(blend(plan, tiles), (+sy, +sx))          weight map and Mixture-of-Diffusers reciprocal in PLAN coordinates

Shared by tests/test_shift_host.py and tests/test_gpu_shift.py; nothing here touches the library."""
from typing import List, Optional, Tuple

import numpy as np

import wrap_ref as wr

M64 = (1 << 64) - 1


def shift(seed: int, step: int, axis: int, extent: int) -> int:
    """The displacement along one axis (0 = x, 1 = y) at one sampler step: the splitmix64 finaliser of seed + golden * (2 step + axis + 1)."""
    z = (seed + 0x9E3779B97F4A7C15 * (2 * step + axis + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z % extent


# (seed, step, axis, extent) -> shift, computed once from the formula above with Python integers
PINNED = {
    (0, 0, 0, 128): 47,
    (0, 0, 1, 64): 52,
    (0, 1, 0, 128): 79,
    (1234567, 0, 0, 37): 24,
    (1234567, 0, 1, 22): 11,
    (1234567, 1, 0, 37): 21,
    (1234567, 1, 1, 22): 1,
    (1234567, 2, 0, 37): 7,
    (1234567, 2, 1, 22): 20,
    (1234567, 19, 0, 1024): 822,
    (4294967295, 7, 1, 65535): 26914,
    (2 ** 63, 3, 0, 2): 1,
    (-1, 5, 1, 1000): 527,
}


def step_shift(g: wr.Grid, wrap_x: bool, wrap_y: bool, seed: int, step: int) -> Tuple[int, int]:
    """(sx, sy) of a job: only the axes that wrap move."""
    return (shift(seed, step, 0, g.W) if wrap_x else 0, shift(seed, step, 1, g.H) if wrap_y else 0)


def boxes(g: wr.Grid, sx: int, sy: int) -> List[Tuple[int, int, int, int]]:
    """The plan's boxes with origins ((x + sx) mod W, (y + sy) mod H), in list order."""
    return [((x + sx) % g.W, (y + sy) % g.H, tw, th) for (x, y, tw, th) in g.boxes]


def gather(g: wr.Grid, x: np.ndarray, batch: int, sx: int, sy: int) -> np.ndarray:
    return wr.gather(g, np.roll(x, (-sy, -sx), axis=(-2, -1)), batch)


def blend(g: wr.Grid, method: str, tiles: np.ndarray, N: int, sx: int, sy: int, weights: Optional[np.ndarray],
          tile_weight: Optional[np.ndarray] = None, rescale: Optional[np.ndarray] = None) -> np.ndarray:
    """weights / rescale: the plan's UNSHIFTED maps."""
    return np.roll(wr.blend(g, method, tiles, N, weights, tile_weight, rescale), (sy, sx), axis=(-2, -1))


def weight_map(g: wr.Grid, sx: int, sy: int, tile_weight: Optional[np.ndarray] = None) -> np.ndarray:
    """The weight sum of the shifted grid in CANVAS coordinates (what the displaced boxes would add up to): the plan's map, rolled."""
    return np.roll(wr.weight_map(g, tile_weight), (sy, sx), axis=(-2, -1))
