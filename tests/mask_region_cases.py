"""The canvases and the region list that tests/test_gpu_mask_regions.py and tests/test_mask_regions_host.py share."""
import numpy as np

# W, H, tile_w, tile_h, overlap, tile batch size
CANVASES = {
    "base": (40, 24, 16, 16, 8, 4),
    "w38": (38, 20, 16, 16, 4, 4),            # the last quad of a row has 2 valid pixels
    "nonsquare": (36, 27, 16, 12, 6, 4),      # non-square tiles
}
# the launcher's 2-, 4- and 8-planes-per-thread forms: H * ceil(W / 4) * planes / PP >= 131072 -- W, H, tile, tile, overlap, bs, N, C
PLANES = {"planes2": (512, 128, 96, 96, 48, 8, 4, 4), "planes4": (512, 128, 96, 96, 48, 8, 4, 8), "planes8": (512, 128, 96, 96, 48, 8, 8, 8)}


def spec(W: int, H: int):
    """[(name, x, y, w, h, mode, cover uint8 [h, w] or None)] in ONE list; every cover touches all four sides of its rectangle, as the bounding box
    of a painted mask does.  Fits every canvas from 36 x 20 up."""
    assert W >= 36 and H >= 20
    out = []
    c = np.ones((9, 13), np.uint8)
    c[0:5, 6:] = 0
    out.append(("L-shaped BG", 2, 1, 13, 9, "bg", c))
    c = np.ones((8, 12), np.uint8)
    c[2:6, 3:9] = 0
    out.append(("BG with a hole", 10, 6, 12, 8, "bg", c))
    i, j = np.mgrid[0:10, 0:10]
    out.append(("FG upper-left triangle", 18, 1, 10, 10, "fg", (i + j <= 9).astype(np.uint8)))       # canvas x + y <= 28
    out.append(("FG lower-right triangle", 20, 3, 10, 10, "fg", (i + j >= 9).astype(np.uint8)))      # canvas x + y >= 32: boxes overlap, shapes do not
    i, j = np.mgrid[0:8, 0:12]
    out.append(("FG diamond", 3, 11, 12, 8, "fg", (np.abs(2 * i - 7) * 12 + np.abs(2 * j - 11) * 8 <= 12 * 8 + 4).astype(np.uint8)))
    c = np.ones((7, 12), np.uint8)
    c[0:3, 0:4] = 0
    out.append(("FG over the diamond", 8, 12, 12, 7, "fg", c))                                        # fcnt = 2 where both cover
    out.append(("one cell", 33, 0, 1, 1, "bg", np.ones((1, 1), np.uint8)))
    i, j = np.mgrid[0:7, 0:9]
    out.append(("FG staircase to the last column and row", W - 9, H - 7, 9, 7, "fg", ((j >= 8 - i) | (i == 6) | (j == 8)).astype(np.uint8)))
    c = np.zeros((5, 13), np.uint8)
    c[:, 0::2] = 1
    out.append(("BG stripes: a boundary inside every quad", 1, H - 6, 13, 5, "bg", c))
    out.append(("plain FG rectangle", 12, 4, 9, 7, "fg", None))
    for (name, x, y, w, h, mode, cover) in out:
        assert 0 <= x and x + w <= W and 0 <= y and y + h <= H, name
        if cover is not None:
            assert cover.shape == (h, w) and cover[0].any() and cover[-1].any() and cover[:, 0].any() and cover[:, -1].any(), name
    return out


def canvas_cover(W: int, H: int) -> np.ndarray:
    """A coverage [H, W] with a blob, a hole in it, a one-cell island and a run along the last column."""
    i, j = np.mgrid[0:H, 0:W]
    c = ((i - H * 0.45) ** 2 * 3 + (j - W * 0.4) ** 2 <= (W * 0.3) ** 2).astype(np.uint8)
    c[H // 2 - 1:H // 2 + 1, W // 3:W // 3 + 3] = 0
    c[1, W - 3] = 1
    c[H // 3:, W - 1] = 1
    return c
