"""What tests/test_lattice_regions_host.py and tests/test_gpu_lattice_regions.py share: the lattices of DESIGN.md 3.18's set, their shifts, and the
region lists laid on them.  A plain module, imported by name; numpy only."""
from typing import List, Tuple

import numpy as np

import grid_lattice_ref as gl
import lattice_region_ref as rr

# id -> (W, H, requested tile_w, tile_h, overlap)
GEOMETRIES = {
    "odd": (37, 22, 16, 12, 4),             # odd extents, non-square tile, strides 12 and 8; the last quad of a row is 1 pixel
    "zero_ov": (40, 24, 16, 16, 0),         # at most 2 covering tiles per axis
    "deep": (33, 20, 16, 16, 12),           # stride 4: up to 16 tiles on a pixel
    "one_col": (16, 40, 16, 16, 4),         # the tile spans x: only y moves
}
# at rest the lattice is the plain plan: (W - tw) % stride == 0 on both axes.  (W, H, tile_w, tile_h, overlap, tile_bs)
REST = [(40, 28, 16, 16, 4, 4), (64, 64, 32, 32, 0, 3), (40, 28, 16, 12, 8, 4)]

Spec = Tuple[int, int, int, int, str]      # (x, y, w, h, "bg" | "fg")


def shifts(geom: str) -> List[Tuple[int, int]]:
    """(1, 1), at rest, (stride_x - 1, 3), (2, 1), each clipped to [1, stride]; an axis that does not move keeps 1."""
    Wc, Hc, tw, th, ov = GEOMETRIES[geom]
    stx, sty = (max(1, s) for s in gl.rest(Wc, Hc, tw, th, ov))
    out = []
    for sx, sy in [(1, 1), (stx, sty), (stx - 1, 3), (2, 1)]:
        s = (min(max(sx, 1), stx), min(max(sy, 1), sty))
        if s not in out:
            out.append(s)
    return out


def full_spec(W: int, H: int) -> List[Spec]:
    """In list order: a large BG region (it straddles every lattice border it meets and, at any shift but the rest, the part of the pushed-in
    edge tiles that does not contribute), an FG region over it, a second FG region over that one (fcnt = 2), a second BG region over the first,
    a BG region equal to the canvas, a 1 x 1 BG region in the last column and the last row, an FG region that ends at x = W (on `odd` inside a
    last quad of 1 pixel) and a BG column that ends at y = H."""
    spec = [(1, 2, W - 4, H // 2 + 3, "bg"), (W // 4, 4, W // 2, H // 2, "fg"), (W // 4 + 3, 6, max(W // 3, 2), max(H // 3, 2), "fg"),
            (W // 2 - 2, H // 3, max(W // 3, 2), H // 3, "bg"), (0, 0, W, H, "bg"), (W - 1, H - 1, 1, 1, "bg"), (W - 7, 1, 7, 5, "fg"),
            (2, H - 6, 3, 6, "bg")]
    assert all(rr.rect_valid(W, H, x, y, w, h) for (x, y, w, h, _) in spec), spec
    return spec


def disjoint_bg_spec(W: int, H: int) -> List[Spec]:
    """No pixel under two BG regions (where Mixture of Diffusers' grouping cannot differ from the plain path's running sum): one BG region, an
    FG region over it, a second FG region over that, a second BG region beside the first, the 1 x 1 BG corner, an FG region ending at x = W."""
    spec = [(1, 2, W // 2 - 2, H // 2 + 3, "bg"), (W // 4, 4, W // 2, H // 2, "fg"), (W // 4 + 3, 6, max(W // 3, 2), max(H // 3, 2), "fg"),
            (W // 2 + 1, 3, W // 3, H // 2, "bg"), (W - 1, H - 1, 1, 1, "bg"), (W - 7, 1, 7, 5, "fg")]
    assert all(rr.rect_valid(W, H, x, y, w, h) for (x, y, w, h, _) in spec), spec
    cnt = np.zeros((H, W), int)
    for (x, y, w, h, mode) in spec:
        if mode == "bg":
            cnt[y:y + h, x:x + w] += 1
    assert cnt.max() == 1
    return spec


def sixteen_spec(W: int, H: int) -> List[Spec]:
    """MDTILE_MAX_REGIONS regions, alternately BG and FG, staggered so that neighbours overlap."""
    spec = [(min(2 * i, W - 6), min(i, H - 5), 6, 5, "bg" if i % 2 == 0 else "fg") for i in range(16)]
    assert len(spec) == 16 and all(rr.rect_valid(W, H, x, y, w, h) for (x, y, w, h, _) in spec)
    return spec


def fg_only(spec: List[Spec]) -> List[Spec]:
    return [s for s in spec if s[4] == "fg"]
