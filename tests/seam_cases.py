"""Hand-built "finished tiles" for the seam-blend tests (tests/test_seam_host.py, tests/test_gpu_seam.py): tables in the form of
tests/seam_ref.py, legal and illegal, in the decoder's and the encoder's bbox convention.  Test infrastructure."""
import numpy as np

SPECIALS = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-40, 1.4e-45, 3.4028234e38, -3.4028234e38, 1.17549435e-38], dtype=np.float32)


def boxes(xs, ys, margin, is_decoder, sub=0):
    """(in_bboxes, out_bboxes, tile shapes) of the grid with column borders xs and row borders ys (output px), every tile padded by `margin`
    px on each side that has a neighbour (an int, or a function (tile index, side 0..3 = left right top bottom) -> px).  Decoder
    convention: out = in * 8 (borders and margins multiples of 8); encoder convention: out = in // 8, the input bbox being 8 * px + sub."""
    rows, cols = len(ys) - 1, len(xs) - 1
    ins, outs, shapes = [], [], []
    for r in range(rows):
        for c in range(cols):
            i = r * cols + c
            m = [(margin(i, s) if callable(margin) else margin) if has else 0
                 for s, has in enumerate((c > 0, c < cols - 1, r > 0, r < rows - 1))]
            ob = (xs[c], xs[c + 1], ys[r], ys[r + 1])
            pad = (ob[0] - m[0], ob[1] + m[1], ob[2] - m[2], ob[3] + m[3])
            if is_decoder:
                assert all(v % 8 == 0 for v in pad), pad
                ib = tuple(v // 8 for v in pad)
            else:
                ib = tuple(v * 8 + sub for v in pad)
            ins.append(ib)
            outs.append(ob)
            shapes.append((pad[3] - pad[2], pad[1] - pad[0]))
    return ins, outs, shapes


def table(xs, ys, margin, is_decoder, N, C, seed=0, special_band=0, common=None, sub=0):
    """The table of seeded randn tiles on that grid.  special_band = b > 0: NaN, +-inf, -0.0, denormals and fp32 max in every tile on both
    sides of every border, inside and outside the bands of half-width b.  common: an image [N, C, RH, RW] all tiles are cut from instead."""
    ins, outs, shapes = boxes(xs, ys, margin, is_decoder, sub)
    rng = np.random.RandomState(seed)
    out = []
    for i, (ib, ob, (th, tw)) in enumerate(zip(ins, outs, shapes)):
        ty, tx = (ib[2] * 8, ib[0] * 8) if is_decoder else (ib[2] // 8, ib[0] // 8)      # image position of the tile's element (0, 0)
        if common is not None:
            t = np.ascontiguousarray(common[:, :, ty:ty + th, tx:tx + tw]).astype(np.float32)
        else:
            t = rng.standard_normal((N, C, th, tw)).astype(np.float32)
        if special_band:
            b = special_band
            for X in xs[1:-1]:
                for j, x in enumerate((X - b - 1, X - b, X - 1, X, X + b - 1, X + b)):
                    if 0 <= x - tx < tw:
                        t[:, :, :, x - tx] = SPECIALS[(np.arange(th) + i + j) % len(SPECIALS)][None, None, :]
            for Y in ys[1:-1]:
                for j, y in enumerate((Y - b - 1, Y - b, Y - 1, Y, Y + b - 1, Y + b)):
                    if 0 <= y - ty < th:
                        t[:, :, y - ty, :] = SPECIALS[(np.arange(tw) * 3 + i + j) % len(SPECIALS)][None, None, :]
        out.append((t, ib, ob))
    return out


# id -> (xs, ys, margin, is_decoder, band, (N, C)): the legal synthetic cases
LEGAL = {
    # the four grid forms, b = 1, both N C pairs
    "1x2_b1": ([0, 16, 40], [0, 16], 8, True, 1, (2, 3)),
    "2x1_b1": ([0, 24], [0, 16, 40], 8, True, 1, (1, 4)),
    "2x2_b1": ([0, 16, 40], [0, 24, 40], 8, True, 1, (2, 3)),
    "3x3_b1": ([0, 16, 32, 56], [0, 8, 24, 40], 8, True, 1, (1, 4)),
    # the interior tile is exactly 2 b wide and tall: its two bands touch
    "3x3_touch": ([0, 16, 32, 56], [0, 24, 40, 56], 8, True, 8, (2, 3)),
    # b equal to the margin: the band's outermost pixel is the padded tile's outermost
    "2x2_margin": ([0, 16, 40], [0, 24, 40], 8, True, 8, (1, 4)),
    "3x3_margin16": ([0, 32, 64, 104], [0, 32, 72, 104], 16, True, 16, (2, 3)),
    # 36 tiles: more than one launch of MDTILE_VAE_BLEND_CHUNK (and than MDTILE_VAE_ASSEMBLE_CHUNK), neighbours in another chunk
    "6x6_chunks": ([0, 8, 16, 24, 32, 40, 48], [0, 8, 16, 24, 32, 40, 48], 8, True, 2, (1, 4)),
    # encoder convention: odd origins, RW = 43 (no multiple of 4), tile pitches 18 / 25 / 12, 26 / 27 and 20 / 36 (16-byte and element copy paths)
    "enc_odd": ([0, 15, 34, 43], [0, 9, 20, 31], 3, False, 3, (2, 3)),
    "enc_1x2": ([0, 21, 43], [0, 7], 5, False, 4, (1, 4)),
    "enc_wide_pitch": ([0, 16, 48], [0, 13, 30], 4, False, 2, (1, 4)),
}

# id -> (xs, ys, margin, is_decoder, band, reason of tests/seam_ref.check_grid): hand-made illegal tables
ILLEGAL = {
    "band_wider_than_tile": ([0, 40, 56], [0, 24], 24, True, 17, "wider"),
    "band_taller_than_edge_tile": ([0, 24], [0, 32, 40], 16, True, 9, "wider"),
    "bands_overlap": ([0, 16, 32, 56], [0, 24], 16, True, 9, "overlap"),
    "margin_smaller_than_band": ([0, 16, 40], [0, 24, 48], 8, True, 9, "margin"),
    "band_zero": ([0, 16, 40], [0, 24], 8, True, 0, "band"),
    "band_negative": ([0, 16, 40], [0, 24], 8, True, -3, "band"),
}

# what the C call's and the host function's messages say for each reason
REASON_TEXT = {"wider": "wider than the tile|taller than the tile", "overlap": "bands overlap", "margin": "margin smaller than the band",
               "band": "band", "grid": "grid"}


def with_hole(tab):
    """The table with its second tile's out box (and input bbox) moved one 8-px step to the right: a hole in the grid."""
    t, ib, ob = tab[1]
    tab = list(tab)
    tab[1] = (t, (ib[0] + 1, ib[1] + 1, ib[2], ib[3]), (ob[0] + 8, ob[1] + 8, ob[2], ob[3]))
    return tab


def result_size(case):
    xs, ys = case[0], case[1]
    return ys[-1], xs[-1]
