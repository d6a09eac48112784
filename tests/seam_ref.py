"""numpy restatement of mdtile_vae_assemble_blend (include/mdtile.h): the grid check, the integer ramp weights, the fp32
loop with np.float32 operations in the stated order, and the plain crop outside the bands.  Test infrastructure: nothing here is imported
by the product.

A table is a list of (tile [N, C, th, tw] float32, in_bbox (x1, x2, y1, y2), out_bbox (x1, x2, y1, y2)) in row-major grid order."""
import numpy as np


def margins(in_bbox, out_bbox, is_decoder):
    """(left, right, top, bottom) px of padding around the out box inside the padded tile (crop_valid_region's rule)."""
    m = [out_bbox[k] - (in_bbox[k] * 8 if is_decoder else in_bbox[k] // 8) for k in range(4)]
    return m[0], -m[1], m[2], -m[3]


def check_grid(table, rows, cols, RH, RW, band, is_decoder):
    """None when the table is legal, else the reason (the words the C call and the host function use)."""
    if band < 1:
        return "band"
    if rows < 1 or cols < 1 or len(table) != rows * cols:
        return "grid"
    xs = [table[c][2][0] for c in range(cols)] + [table[cols - 1][2][1]]
    ys = [table[r * cols][2][2] for r in range(rows)] + [table[(rows - 1) * cols][2][3]]
    if xs[0] != 0 or xs[-1] != RW or ys[0] != 0 or ys[-1] != RH or any(b <= a for a, b in zip(xs, xs[1:])) or any(b <= a for a, b in zip(ys, ys[1:])):
        return "grid"
    for i, (t, ib, ob) in enumerate(table):
        r, c = divmod(i, cols)
        if tuple(ob) != (xs[c], xs[c + 1], ys[r], ys[r + 1]):
            return "grid"
        ml, mr, mt, mb = margins(ib, ob, is_decoder)
        th, tw = t.shape[2:]
        if min(ml, mr, mt, mb) < 0 or tw - ml - mr != ob[1] - ob[0] or th - mt - mb != ob[3] - ob[2]:
            return "bboxes"
        nbx, nby = (c > 0) + (c < cols - 1), (r > 0) + (r < rows - 1)
        for extent, nb in ((ob[1] - ob[0], nbx), (ob[3] - ob[2], nby)):
            if extent < band * nb:                       # two bands in a tile narrower than 2 b overlap; one band in a tile narrower than b leaves it
                return "overlap" if nb == 2 and extent >= band else "wider"
        if (c > 0 and ml < band) or (c < cols - 1 and mr < band) or (r > 0 and mt < band) or (r < rows - 1 and mb < band):
            return "margin"
    return None


def ramp(band):
    """(a_first, a_second) over the 2 b positions of a band: the weights of the tile before the border (left / top) and behind it."""
    a2 = 2 * np.arange(2 * band, dtype=np.int64) + 1           # 2 (x - X + b) + 1 for x - X + b = 0 .. 2 b - 1
    return 4 * band - a2, a2


def segments(edges, band):
    """One axis cut into runs of equal contributors: [(lo, hi, (tile index along the axis, ...), weights or None)] -- a run outside the
    bands has one contributor and no weights; a band has two and their integer weight vectors."""
    n = len(edges) - 1
    a1, a2 = ramp(band)
    out = []
    for k in range(n):
        lo = edges[k] + (band if k > 0 else 0)
        hi = edges[k + 1] - (band if k < n - 1 else 0)
        if k > 0:
            out.append((edges[k] - band, edges[k] + band, (k - 1, k), (a1, a2)))
        if hi > lo:
            out.append((lo, hi, (k,), None))
    return out


def _window(table, k, is_decoder, y0, y1, x0, x1):
    """Image rows [y0, y1) x columns [x0, x1) read from tile k's padded output."""
    t, ib, ob = table[k]
    ml, _, mt, _ = margins(ib, ob, is_decoder)
    ty, tx = ob[2] - mt, ob[0] - ml
    assert 0 <= y0 - ty and y1 - ty <= t.shape[2] and 0 <= x0 - tx and x1 - tx <= t.shape[3], "read outside the padded tile"
    return t[:, :, y0 - ty:y1 - ty, x0 - tx:x1 - tx]


def contributions(table, rows, cols, band):
    """[(y0, y1, x0, x1, [(tile index, integer weight image [h, w])] in ascending tile index, D)] covering the result once; one
    contributor (weight image None, D = 1) outside the bands."""
    xs = [table[c][2][0] for c in range(cols)] + [table[cols - 1][2][1]]
    ys = [table[r * cols][2][2] for r in range(rows)] + [table[(rows - 1) * cols][2][3]]
    out = []
    for y0, y1, rr, wy in segments(ys, band):
        for x0, x1, cc, wx in segments(xs, band):
            if wy is None and wx is None:
                out.append((y0, y1, x0, x1, [(rr[0] * cols + cc[0], None)], 1))
                continue
            vy = wy if wy is not None else (np.ones(y1 - y0, dtype=np.int64),)
            vx = wx if wx is not None else (np.ones(x1 - x0, dtype=np.int64),)
            D = (4 * band if wy is not None else 1) * (4 * band if wx is not None else 1)
            terms = [(r * cols + c, np.outer(vy[i], vx[j])) for i, r in enumerate(rr) for j, c in enumerate(cc)]
            assert [k for k, _ in terms] == sorted(k for k, _ in terms)
            out.append((y0, y1, x0, x1, terms, D))
    return out


def assemble_plain(table, RH, RW, is_decoder):
    """mdtile_vae_assemble: crop_valid_region of every tile pasted into its out box."""
    N, C = table[0][0].shape[:2]
    out = np.full((N, C, RH, RW), np.nan, dtype=np.float32)
    for k, (t, ib, ob) in enumerate(table):
        out[:, :, ob[2]:ob[3], ob[0]:ob[1]] = _window(table, k, is_decoder, ob[2], ob[3], ob[0], ob[1])
    return out


def band_mask(table, rows, cols, RH, RW, band):
    """bool [RH, RW]: the pixels inside at least one band."""
    m = np.zeros((RH, RW), dtype=bool)
    for y0, y1, x0, x1, terms, D in contributions(table, rows, cols, band):
        if D != 1:
            m[y0:y1, x0:x1] = True
    return m


def assemble_blend(table, rows, cols, RH, RW, band, is_decoder):
    """The definition: outside the bands the owner's bits; in a band acc = +0; acc = acc + f32(w_k) * v_k in ascending tile index (product
    and sum rounded to fp32 once each); out = acc / f32(D)."""
    why = check_grid(table, rows, cols, RH, RW, band, is_decoder)
    if why is not None:
        raise ValueError(why)
    N, C = table[0][0].shape[:2]
    out = np.full((N, C, RH, RW), np.nan, dtype=np.float32)
    with np.errstate(all="ignore"):
        for y0, y1, x0, x1, terms, D in contributions(table, rows, cols, band):
            if D == 1:
                out[:, :, y0:y1, x0:x1] = _window(table, terms[0][0], is_decoder, y0, y1, x0, x1)
                continue
            acc = np.zeros((N, C, y1 - y0, x1 - x0), dtype=np.float32)
            for k, w in terms:
                assert w.max() < 2 ** 24
                prod = w.astype(np.float32)[None, None] * _window(table, k, is_decoder, y0, y1, x0, x1).astype(np.float32)
                assert prod.dtype == np.float32
                acc = acc + prod
            out[:, :, y0:y1, x0:x1] = acc / np.float32(D)
    assert out.dtype == np.float32
    return out
