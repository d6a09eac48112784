"""numpy restatement of mdtile_mask_activity_u8 and mdtile_vae_assemble_sparse (include/mdtile.h).  Test infrastructure:
nothing here is imported by the product.

A box is (x1, x2, y1, y2) in image px, the order mdtile_vae_split_tiles returns.  A tile table is a list of (tile [N, C, th, tw] float32,
in_bbox, out_bbox) as in tests/seam_ref.py, decoder convention (out = in * 8)."""
import numpy as np

import seam_ref as sr

MAX_BOXES = 4096


def activity(mask, boxes):
    """[1 iff some byte of mask[y1:y2, x1:x2] is not zero, else 0] per box; ValueError with the C call's word for what it refuses."""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim == 2
    RH, RW = mask.shape
    if not 1 <= len(boxes) <= MAX_BOXES:
        raise ValueError("n_boxes")
    for x1, x2, y1, y2 in boxes:
        if not (x1 < x2 and y1 < y2):
            raise ValueError("empty")
        if not (0 <= x1 and 0 <= y1 and x2 <= RW and y2 <= RH):
            raise ValueError("outside")
    return [int(mask[y1:y2, x1:x2].any()) for x1, x2, y1, y2 in boxes]


def fill_value(byte):
    """(float)byte / 127.5f - 1.0f: one fp32 division, one fp32 subtraction."""
    b = np.asarray(byte, dtype=np.uint8).astype(np.float32)
    out = b / np.float32(127.5) - np.float32(1.0)
    assert out.dtype == np.float32
    return out


def check_sparse(tiles, fill_boxes, RH, RW):
    """None when the call is legal, else the reason (a word of the C call's message)."""
    boxes = [tuple(ob) for _, _, ob in tiles] + [tuple(b) for b in fill_boxes]
    if len(boxes) > MAX_BOXES:
        return "more than"
    for t, ib, ob in tiles:
        ml, mr, mt, mb = sr.margins(ib, ob, True)
        th, tw = t.shape[2:]
        if min(ml, mr, mt, mb) < 0 or tw - ml - mr != ob[1] - ob[0] or th - mt - mb != ob[3] - ob[2] or ob[1] <= ob[0] or ob[3] <= ob[2]:
            return "bboxes"
        if not (0 <= ob[0] and 0 <= ob[2] and ob[1] <= RW and ob[3] <= RH):
            return "outside"
    for x1, x2, y1, y2 in fill_boxes:
        if not (x1 < x2 and y1 < y2):
            return "empty"
        if not (0 <= x1 and 0 <= y1 and x2 <= RW and y2 <= RH):
            return "outside"
    n = len(tiles)
    for i, p in enumerate(boxes):
        for j, q in enumerate(boxes[:i]):
            if p[0] >= q[1] or q[0] >= p[1] or p[2] >= q[3] or q[2] >= p[3]:
                continue
            return "also tile" if p == q and i >= n > j else "overlap"
    if sum((b[1] - b[0]) * (b[3] - b[2]) for b in boxes) != RH * RW:
        return "area sum"
    return None


def assemble_sparse(tiles, fill_boxes, fill, N, C, RH, RW):
    """The definition: crop_valid_region of every tile pasted into its out box (tests/seam_ref.py's crop rule, bits copied), every fill box
    written as fill_value(fill[y, x, c]) for every n -- fill: uint8 [RH, RW, C] -- or as +0.0 when fill is None.  ValueError(reason) for a
    call the C entry point refuses."""
    why = check_sparse(tiles, fill_boxes, RH, RW)
    if why is not None:
        raise ValueError(why)
    out = np.full((N, C, RH, RW), np.nan, dtype=np.float32)
    written = np.zeros((RH, RW), dtype=np.int32)
    for k, (t, ib, ob) in enumerate(tiles):
        assert t.shape[:2] == (N, C)
        out[:, :, ob[2]:ob[3], ob[0]:ob[1]] = sr._window(tiles, k, True, ob[2], ob[3], ob[0], ob[1])
        written[ob[2]:ob[3], ob[0]:ob[1]] += 1
    if fill is not None:
        fill = np.asarray(fill)
        assert fill.dtype == np.uint8 and fill.shape == (RH, RW, C)
    for x1, x2, y1, y2 in fill_boxes:
        if fill is None:
            out[:, :, y1:y2, x1:x2] = np.float32(0.0)
        else:
            out[:, :, y1:y2, x1:x2] = fill_value(fill[y1:y2, x1:x2]).transpose(2, 0, 1)[None]
        written[y1:y2, x1:x2] += 1
    assert (written == 1).all(), "every pixel is written exactly once"
    return out


def round_trip(values, truncate):
    """What a host makes of the fill's values on the way back to bytes: (x + 1) / 2 * 255 in fp32, clipped, then rounded (np.rint) or
    truncated (astype(uint8), the webui's)."""
    x = np.clip((np.asarray(values, dtype=np.float32) + np.float32(1.0)) / np.float32(2.0) * np.float32(255.0), 0, 255)
    return (x if truncate else np.rint(x)).astype(np.uint8)
