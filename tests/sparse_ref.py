"""Numpy restatement of tile skipping (include/mdtile.h: mdtile_tile_activity, mdtile_plan_create_subset, mdtile_blend_sparse) on
the plain grid: which tiles a mask touches (a slice test), the sparse plan of those tiles, the liveness map, and the blend as
`where(live, full blend, fill)` with the full blend the SEQUENTIAL fp32 `+=` loop over ALL grid tiles (tests/wrap_ref.py: blend, which on an
axis that does not wrap is the plain loop).  Shared by tests/test_sparse_host.py and tests/test_gpu_sparse.py; nothing here touches the library.

Half dtypes follow the project's rule (tests/test_gpu_blend_matrix.py): callers round the inputs to the dtype, evaluate the fp32 restatement on
those values and round the result once; `fill` is never converted -- it is selected as it is."""
import math
from typing import List, NamedTuple, Sequence, Tuple

import numpy as np

import wrap_ref as wr


def grid(W: int, H: int, tile_w: int, tile_h: int, overlap: int, tile_bs: int) -> wr.Grid:
    """The plain grid (init_grid_bbox + split_bboxes) in wrap_ref's form: no tile passes an edge."""
    tw, th, ov = wr.clamp(W, H, tile_w, tile_h, overlap)
    xs, ys = wr.plain_origins(W, tw, ov), wr.plain_origins(H, th, ov)
    boxes = tuple((x, y, tw, th) for y in ys for x in xs)
    T = len(boxes)
    nb = math.ceil(T / tile_bs)
    bs = math.ceil(T / nb)
    batches = tuple(tuple(range(i * bs, min((i + 1) * bs, T))) for i in range(nb))
    return wr.Grid(W, H, tw, th, ov, len(xs), len(ys), tuple(xs), tuple(ys), boxes, bs, batches)


def activity(g: wr.Grid, mask: np.ndarray) -> List[int]:
    """mask [P, H, W] fp32 -> per tile 1 iff some element under it is not equal to zero (NaN is not equal to zero; -0.0 is)."""
    assert mask.ndim == 3 and mask.shape[1:] == (g.H, g.W)
    return [int(np.any(~(mask[:, y:y + th, x:x + tw] == 0))) for (x, y, tw, th) in g.boxes]


class Subset(NamedTuple):
    active_ids: Tuple[int, ...]                         # parent tile indices, ascending
    boxes: Tuple[Tuple[int, int, int, int], ...]
    tile_bs: int
    batches: Tuple[Tuple[int, ...], ...]                # parent tile indices per compact batch, in slot order


def subset(g: wr.Grid, active: Sequence[int], tile_bs: int) -> Subset:
    """The sparse plan: the batching rule of the grid applied to the active tiles.  None of them: the library refuses."""
    ids = tuple(t for t, a in enumerate(active) if a)
    assert ids, "no active tile"
    nb = math.ceil(len(ids) / tile_bs)
    bs = math.ceil(len(ids) / nb)
    return Subset(ids, tuple(g.boxes[t] for t in ids), bs, tuple(ids[i * bs:(i + 1) * bs] for i in range(nb)))


def live_map(g: wr.Grid, active: Sequence[int]) -> np.ndarray:
    """[H, W] bool: every grid tile that covers the pixel is active."""
    live = np.ones((g.H, g.W), bool)
    for a, (x, y, tw, th) in zip(active, g.boxes):
        if not a:
            live[y:y + th, x:x + tw] = False
    return live


def gather(g: wr.Grid, x: np.ndarray, tile_ids: Sequence[int]) -> np.ndarray:
    """x [N, C, H, W] -> the tiles `tile_ids` in that order, [len * N, C, th, tw], tile-major."""
    return np.ascontiguousarray(np.concatenate([x[:, :, by:by + th, bx:bx + tw] for (bx, by, tw, th) in (g.boxes[t] for t in tile_ids)], axis=0))


def full_blend(g: wr.Grid, method: str, tiles: np.ndarray, N: int, weights, tile_weight=None, rescale=None) -> np.ndarray:
    """The sequential `+=` loop over all grid tiles and the method's epilogue: tiles [T * N, C, th, tw] fp32 -> [N, C, H, W] fp32."""
    return wr.blend(g, method, tiles, N, weights, tile_weight, rescale)


def select(live: np.ndarray, full, fill):
    """where(live, full, fill) on the BITS of two torch tensors of one dtype (numpy has no bfloat16), so that no NaN payload or zero sign of
    `fill` is touched."""
    import torch
    assert full.dtype == fill.dtype and full.shape == fill.shape
    iv = torch.int32 if full.dtype == torch.float32 else torch.int16
    out = torch.where(torch.from_numpy(live)[None, None], full.contiguous().view(iv), fill.contiguous().view(iv))
    return out.view(full.dtype)
