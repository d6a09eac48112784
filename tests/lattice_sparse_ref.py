"""Numpy restatement of inpaint tile skipping under the jittered grid (include/mdtile.h: mdtile_lattice_activity,
mdtile_lattice_subset_make / _bboxes, mdtile_gather_all_lattice_sparse, mdtile_blend_lattice_sparse), built on the restatement of the lattice
(tests/grid_lattice_ref.py: lattice, gather, blend, weight_map) and the live rule, independent of the engine:

    contributing box of tile t = its LATTICE box clipped to the canvas: the only place where its output enters the blend
    active[t]  = some element of mask[:, contributing box] is not equal to zero (NaN is not equal to zero; -0.0 is)
    slot[t]    = number of active t' < t where t is active, else -1
    live[y, x] = every lattice tile whose contributing box holds (y, x) is active
    blend      = the FULL lattice blend with the active tiles' outputs scattered to their places in a full tile array whose other entries are
                 NaN, where live; `fill`'s bits everywhere else.  A NaN of an inactive tile can only reach a pixel that is not live, so a result
                 that is finite where live proves that no inactive entry was selected.

Shared by tests/test_lattice_sparse_host.py and tests/test_gpu_lattice_sparse.py; nothing here touches the library."""
import math
from typing import List, Optional, Sequence, Tuple

import numpy as np

import grid_lattice_ref as lr
import sparse_ref as sr


def boxes(g: lr.Lattice) -> List[Tuple[int, int, int, int]]:
    """Per tile (row-major) its contributing box as (y0, y1, x0, x1) in canvas coordinates."""
    out = []
    for r in range(g.rows):
        for c in range(g.cols):
            out.append((max(g.vs[r], 0), min(g.vs[r] + g.th, g.H), max(g.us[c], 0), min(g.us[c] + g.tw, g.W)))
    return out


def activity(g: lr.Lattice, mask: np.ndarray) -> List[int]:
    """mask [P, H, W] fp32 -> per tile 1 iff some element of its contributing box is not equal to zero."""
    assert mask.ndim == 3 and mask.shape[1:] == (g.H, g.W)
    return [int(np.any(~(mask[:, y0:y1, x0:x1] == 0))) for (y0, y1, x0, x1) in boxes(g)]


def slots(active: Sequence[int]) -> List[int]:
    out, n = [], 0
    for a in active:
        out.append(n if a else -1)
        n += 1 if a else 0
    return out


def ids(active: Sequence[int]) -> Tuple[int, ...]:
    return tuple(t for t, a in enumerate(active) if a)


def batching(num_active: int, tile_bs: int) -> Tuple[int, int]:
    """(num_batches, tile_bs) of the compact batches: the rule of mdtile_plan_create_subset."""
    nb = math.ceil(num_active / tile_bs)
    return nb, math.ceil(num_active / nb)


def live_map(g: lr.Lattice, active: Sequence[int]) -> np.ndarray:
    """[H, W] bool: every lattice tile that covers the pixel is active."""
    live = np.ones((g.H, g.W), bool)
    for a, (y0, y1, x0, x1) in zip(active, boxes(g)):
        if not a:
            live[y0:y1, x0:x1] = False
    return live


def gather(g: lr.Lattice, x: np.ndarray, tile_ids: Sequence[int]) -> np.ndarray:
    """x [N, C, H, W] -> the tiles `tile_ids` in that order, [len * N, C, th, tw], tile-major: the PUSHED-IN boxes."""
    return np.ascontiguousarray(np.concatenate([x[:, :, by:by + th, bx:bx + tw] for (bx, by, tw, th) in (g.boxes[t] for t in tile_ids)], axis=0))


def blend(g: lr.Lattice, method: str, compact_tiles: np.ndarray, N: int, active: Sequence[int], fill, tile_weight: Optional[np.ndarray] = None):
    """compact_tiles [Ta * N, C, th, tw] fp32 (the active tiles' outputs in ascending tile index, already rounded to fill's dtype); fill: a torch
    tensor [N, C, H, W] of the result's dtype.  -> torch tensor of that dtype: the full lattice blend rounded once where live, fill's bits
    elsewhere."""
    import torch
    act = ids(active)
    assert compact_tiles.shape[0] == len(act) * N
    full = np.full((len(g.boxes) * N,) + compact_tiles.shape[1:], np.nan, np.float32)
    for s, t in enumerate(act):
        full[t * N:(t + 1) * N] = compact_tiles[s * N:(s + 1) * N]
    with np.errstate(all="ignore"):
        res = lr.blend(g, method, full, N, tile_weight)
    return sr.select(live_map(g, active), torch.from_numpy(res).to(fill.dtype), fill)
