"""Free-form mask regions (mdtile_mask_cover_u8, mdtile_mask_region, mdtile_blend_mask_regions, mdtile_region_noise_masked; csrc/mask_regions.hip and
the MASKED form of k_blend in csrc/blend.hip) on the GPU, BITWISE against the numpy restatement tests/mask_region_ref.py: one
region list (tests/mask_region_cases.py) for both methods in fp32, fp16 and bf16, with the grid and without; NaN under every pixel a region does
not cover; the equalities with mdtile_blend, mdtile_feather_mask and mdtile_region_noise; every planes-per-thread form; every refusal with its
output left untouched; and both delegates with two mask files and one rectangle.  No tolerance appears in this file; half types follow
tests/test_gpu_blend_matrix.py (inputs rounded to the dtype, the fp32 restatement evaluated on those values, rounded once).

N = 2, C = 4 unless a case is there for the planes; the shapes are the smallest at which each branch can go wrong."""
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from hostsim import stub_host as sh
from oracle import blend_oracle as bo

import mask_region_cases as cases
import mask_region_ref as rr
from wrap_common import DT, NAN, N, C, assert_bitwise as _assert_bitwise

pytestmark = pytest.mark.gpu


def _method(E, method):
    return E.METHOD_MD if method == "md" else E.METHOD_MOD


@functools.lru_cache(maxsize=None)
def _data(key, dt, n, c):
    """(boxes, tiles, regions) on the CPU: the model outputs of the grid's tiles and of every region of the list in the dtype (random normal), a
    feather for the FG regions (the chessboard feather of their cover at ratio 0.5) and the Gaussian of the BG ones."""
    W, H, tw, th, ov, bs = (cases.CANVASES.get(key) or cases.PLANES[key])[:6]
    boxes = bo.init_grid(W, H, tw, th, ov, bs)[0]
    torch.manual_seed(len(boxes) * 3 + n * c)
    tiles = torch.randn(len(boxes) * n, c, boxes[0][3], boxes[0][2]).to(DT[dt])
    regions = []
    for (name, x, y, w, h, mode, cover) in cases.spec(W, H):
        out = torch.randn(n, c, h, w).to(DT[dt])
        if mode == "fg":
            weight = rr.feather(np.ones((h, w), np.uint8) if cover is None else cover, 0.5)
        else:
            weight = bo.gaussian_weights(w, h).numpy()
        regions.append((x, y, w, h, mode, out, weight, cover))
    return tuple(boxes), tiles, tuple(regions)


def _maps(E, cuda, plan, method, regions, grid):
    """The host's maps made the way the delegates make them, each checked against the restatement's: (weights, tile_w, rescale, per-region weight on
    the device, the same four as numpy)."""
    W, H = plan.w, plan.h
    tile_w = E.gaussian_weights(plan.tile_w, plan.tile_h, cuda) if method == "mod" else None
    weights = torch.zeros(H, W, device=cuda)
    if grid:
        E.weight_map_add_grid(plan, tile_w, weights)
    grid_np = weights.cpu().numpy().copy()
    ref_regions = [rr.Region(x, y, w, h, mode, None, None, cover) for (x, y, w, h, mode, _, _, cover) in regions]
    gauss = [wt for (_, _, _, _, _, _, wt, _) in regions]
    for (x, y, w, h, mode, _, wt, cover) in regions:
        if mode == "bg":
            cov = torch.ones(h, w) if cover is None else torch.from_numpy(cover).float()
            E.weight_map_add_rect(weights, x, y, w, h, (cov if method == "md" else torch.from_numpy(wt) * cov).to(cuda).contiguous(), 1.0)
    want_w = rr.weight_sum(grid_np, method, ref_regions, gauss)
    _assert_bitwise(weights, torch.from_numpy(want_w), f"weight sum {method}")
    rescale = E.reciprocal(weights) if method == "mod" else None
    with np.errstate(all="ignore"):
        want_r = (np.float32(1.0) / want_w).astype(np.float32) if method == "mod" else None
    dev_w, np_w = [], []
    for R, (x, y, w, h, mode, _, wt, cover) in zip(ref_regions, regions):
        if mode == "fg":
            dev_w.append(torch.from_numpy(wt).to(cuda)); np_w.append(wt)
        elif method == "md":
            dev_w.append(None); np_w.append(None)
        else:
            cov = torch.ones(h, w) if cover is None else torch.from_numpy(cover).float()
            t = (torch.from_numpy(wt) * cov).to(cuda).contiguous().view(1, 1, h, w)
            E.rect_mul_canvas(t, rescale, x, y, w, h)
            want = rr.premultiplied(wt, R, want_r)
            _assert_bitwise(t.view(h, w), torch.from_numpy(want), f"premultiplied weight of region at ({x}, {y})")
            dev_w.append(t); np_w.append(want)
    return weights, tile_w, rescale, dev_w, want_w, None if tile_w is None else tile_w.cpu().numpy(), want_r, np_w


def _plan(E, key):
    W, H, tw, th, ov, bs = (cases.CANVASES.get(key) or cases.PLANES[key])[:6]
    plan = E.Plan(W, H, tw, th, ov, bs)
    assert [tuple(b) for b in plan.bboxes] == [tuple(b) for b in bo.init_grid(W, H, tw, th, ov, bs)[0]]
    return plan


def _batches(plan, tiles, n, cuda):
    first = np.cumsum([0] + [len(b) for b in plan.batches])
    return [tiles[first[i] * n:first[i + 1] * n].contiguous().to(cuda) for i in range(plan.num_batches)]


def _case(E, cuda, key, method, dt, grid, n=N, c=C, plant=False, covers="spec"):
    """One launch against the restatement -> (got, the arguments of the same call for mdtile_blend).  plant: NaN in every region output and weight
    under the pixels the region does not cover.  covers: "spec" | "null" | "ones"."""
    dtype = DT[dt]
    plan = _plan(E, key)
    boxes, tiles, regions = _data(key, dt, n, c)
    if covers != "spec":
        regions = tuple((x, y, w, h, mode, out, wt, None if covers == "null" else np.ones((h, w), np.uint8)) for (x, y, w, h, mode, out, wt, _) in regions)
    weights, tile_w, rescale, dev_w, np_weights, np_tile_w, np_rescale, np_w = _maps(E, cuda, plan, method, regions, grid)
    specs, ref = [], []
    for (x, y, w, h, mode, out, _, cover), dw, nw in zip(regions, dev_w, np_w):
        out = out.clone()
        if plant and cover is not None:
            hole = torch.from_numpy(cover == 0)
            out[:, :, hole] = NAN
            if dw is not None:
                dw = dw.clone()
                dw.view(h, w)[hole.to(cuda)] = NAN
                nw = nw.copy()
                nw[cover == 0] = NAN
        specs.append(E.RegionSpec(x, y, w, h, E.REGION_FG if mode == "fg" else E.REGION_BG, out.to(cuda), dw,
                                  None if cover is None else torch.from_numpy(cover).to(cuda)))
        ref.append(rr.Region(x, y, w, h, mode, out.float().numpy(), nw, cover))
    batch = _batches(plan, tiles, n, cuda) if grid else []
    out = torch.full((n, c, plan.h, plan.w), NAN, dtype=dtype, device=cuda)
    kw = dict(weights=weights) if method == "md" else dict(tile_w=tile_w if grid else None, rescale=rescale)
    got = E.blend_mask_regions(plan, _method(E, method), batch, n, c, regions=specs, out=out, dtype=dtype, device=cuda, **kw)
    want = rr.blend(plan.w, plan.h, boxes, method, tiles.float().numpy() if grid else None, n, c, ref, np_weights, np_tile_w, np_rescale)
    _assert_bitwise(got, torch.from_numpy(want).to(dtype), f"{key} {method} {dt} grid={grid} covers={covers} plant={plant}")
    return got, (plan, batch, specs, kw)


# ---- the blend against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [True, False])
@pytest.mark.parametrize("key", list(cases.CANVASES))
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_blend_mask_regions_bitwise(plugin, cuda, key, method, dt, grid):
    """The whole list -- an L, a hole, two FG triangles whose boxes overlap and whose shapes do not, two FG covers that overlap, one cell, a cover
    ending at the last column and row, stripes that put a boundary inside every quad, a plain rectangle -- with the grid and with regions only."""
    _case(plugin.engine, cuda, key, method, dt, grid)


@pytest.mark.parametrize("key,dt", [(k, dt) for k in ("planes2", "planes4") for dt in DT] + [("planes8", "f32")])
@pytest.mark.parametrize("method", ["md", "mod"])
def test_every_planes_per_thread_form(plugin, cuda, key, method, dt):
    E = plugin.engine
    n, c = cases.PLANES[key][6:]
    # the masked call never takes the LDS kernel: its planes per thread are k_blend's, which the query reports for a call without a grid
    d = E.blend_dispatch(_plan(E, key), DT[dt], n, c, num_batches=0)
    assert not d.lds and d.planes == {"planes2": 2, "planes4": 4, "planes8": 8}[key]
    _case(E, cuda, key, method, dt, True, n, c)


@pytest.mark.parametrize("method", ["md", "mod"])
def test_shapes_do_not_leak_into_each_other(plugin, cuda, method):
    """The case a zero weight gets wrong: the two FG triangles alone, feather 1.0, no grid.  Each shape's pixels carry its own region's output, bit
    for bit; the strip between them, inside both boxes, carries nothing."""
    E = plugin.engine
    plan = _plan(E, "base")
    W, H = plan.w, plan.h
    _, _, regions = _data("base", "f32", N, C)
    tri = [r for r in regions if r[4] == "fg"][:2]
    specs = [E.RegionSpec(x, y, w, h, E.REGION_FG, out.to(cuda), torch.ones(h, w, device=cuda), torch.from_numpy(cover).to(cuda))
             for (x, y, w, h, _, out, _, cover) in tri]
    zeros = torch.zeros(H, W, device=cuda)
    kw = dict(weights=zeros) if method == "md" else dict(rescale=zeros)
    got = E.blend_mask_regions(plan, _method(E, method), [], N, C, regions=specs, dtype=torch.float32, device=cuda, **kw).cpu()
    painted = torch.zeros(H, W, dtype=torch.bool)
    for (x, y, w, h, _, out, _, cover) in tri:
        m = torch.from_numpy(cover != 0)
        assert not painted[y:y + h, x:x + w][m].any(), "the shapes overlap"
        painted[y:y + h, x:x + w] |= m
        _assert_bitwise(got[:, :, y:y + h, x:x + w][:, :, m], out[:, :, m], f"{method}: the pixels of the shape at ({x}, {y})")
    (ax, ay, aw, ah), (bx, by, bw, bh) = [r[:4] for r in tri]
    both = torch.zeros(H, W, dtype=torch.bool)
    both[max(ay, by):min(ay + ah, by + bh), max(ax, bx):min(ax + aw, bx + bw)] = True
    assert (both & ~painted).any() and (both & painted).any(), "the boxes overlap, over covered and uncovered pixels"
    assert (got[:, :, ~painted] == 0).all()


@pytest.mark.parametrize("grid", [True, False])
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_nan_under_uncovered_pixels_never_reaches_the_image(plugin, cuda, method, dt, grid):
    E = plugin.engine
    got, _ = _case(E, cuda, "w38", method, dt, grid, plant=True)
    assert torch.isfinite(got).all(), "a value under a pixel its region does not cover reached the output"
    clean, _ = _case(E, cuda, "w38", method, dt, grid)
    _assert_bitwise(got, clean.cpu(), "the planted values change the output")


@pytest.mark.parametrize("covers", ["null", "ones"])
@pytest.mark.parametrize("key", ["base", "w38", "planes2"])
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_without_shapes_it_is_mdtile_blend(plugin, cuda, key, method, dt, covers):
    E = plugin.engine
    n, c = cases.PLANES[key][6:] if key in cases.PLANES else (N, C)
    got, (plan, batch, specs, kw) = _case(E, cuda, key, method, dt, True, n, c, covers=covers)
    plain = [E.RegionSpec(r.x, r.y, r.w, r.h, r.mode, r.out, r.weight) for r in specs]
    want = E.blend(plan, _method(E, method), batch, n, c, regions=plain, **kw)
    _assert_bitwise(got, want.cpu(), f"{key} {method} {dt} covers={covers} against mdtile_blend")


# ---- mask -> coverage -----------------------------------------------------------------------------------------------------------------
def _mask(Hm, Wm, seed):
    """Random bytes (a cell's sum lands on either side of the threshold), a band of zeros around them and a block of 255."""
    g = torch.Generator().manual_seed(seed)
    m = torch.randint(0, 256, (Hm, Wm), generator=g, dtype=torch.int32).to(torch.uint8)
    m[:Hm // 6] = 0
    m[:, :Wm // 5] = 0
    m[-(Hm // 8):] = 0
    m[Hm // 2:Hm // 2 + Hm // 6, Wm // 2:Wm // 2 + Wm // 6] = 255
    return m


@pytest.mark.parametrize("W,H", [(40, 24), (38, 20), (64, 20)])
@pytest.mark.parametrize("scale", [(8, 0, 0), (8, 5, 3), (4, 0, 0), (1, 0, 0)])
def test_mask_cover_u8(plugin, cuda, W, H, scale):
    """Masks of 8H x 8W (8-byte loads), (8H + 5) x (8W + 3) (ragged boxes, byte loads), 4H x 4W (4-byte loads) and H x W; W = 64 takes the box
    kernel's 16-byte form.  Cover and box bitwise; the outputs start as garbage."""
    E = plugin.engine
    s, dh, dw = scale
    mask = _mask(s * H + dh, s * W + dw, W + s)
    want_c, want_b = rr.cover_u8(mask.numpy(), W, H)
    cover, box = E.mask_cover_u8(mask.to(cuda), W, H)
    assert cover.dtype == torch.uint8 and box.dtype == torch.int32
    assert torch.equal(cover.cpu(), torch.from_numpy(want_c)) and box.tolist() == want_b
    assert 0 < want_b[4] < W * H and want_b[0] > 0 and want_b[1] > 0
    again, box2 = E.mask_cover_u8(mask.to(cuda), W, H)
    assert torch.equal(again, cover) and torch.equal(box2, box)


def test_mask_cover_u8_at_the_8k_size(plugin, cuda):
    """Hm = Wm = 8192 at H = W = 1024, the 8K job's mask: every cell owns an 8 x 8 box, so the expected sums are a reshape.  The box kernel's 16-byte
    form runs 64 iterations per thread here and the row offsets pass 2^24."""
    E = plugin.engine
    M, S = 8192, 1024
    mask = np.random.default_rng(8).integers(0, 256, (M, M), dtype=np.uint8)
    mask[:700] = 0
    mask[:, :1300] = 0
    mask[-90:] = 0
    mask[4096:4500, 5000:7000] = 255
    s = mask.reshape(S, 8, S, 8).sum(axis=(1, 3), dtype=np.int64)
    want = (2 * s >= 255 * 64).astype(np.uint8)
    cover, box = E.mask_cover_u8(torch.from_numpy(mask).to(cuda), S, S)
    assert torch.equal(cover.cpu(), torch.from_numpy(want)) and box.tolist() == rr.box_of(want)
    assert 0 < box.tolist()[4] < S * S and box.tolist()[0] >= 1300 // 8 and box.tolist()[1] >= 700 // 8


def test_mask_cover_u8_edge_masks(plugin, cuda):
    E = plugin.engine
    W, H = 40, 24
    cover, box = E.mask_cover_u8(torch.zeros(8 * H, 8 * W, dtype=torch.uint8, device=cuda), W, H)
    assert box.tolist() == [0, 0, 0, 0, 0] and not cover.any()
    cover, box = E.mask_cover_u8(torch.full((8 * H, 8 * W), 255, dtype=torch.uint8, device=cuda), W, H)
    assert box.tolist() == [0, 0, W, H, W * H] and cover.all()
    one = torch.zeros(8 * H, 8 * W, dtype=torch.uint8)
    one[8 * 23:, 8 * 39:] = 255
    cover, box = E.mask_cover_u8(one.to(cuda), W, H)
    assert box.tolist() == [39, 23, 40, 24, 1]
    # the threshold: a 2 x 2 box of {255, 255, 0, 0} is covered, {255, 254, 0, 0} is not
    m = torch.zeros(2, 4, dtype=torch.uint8)
    m[0, 0], m[0, 1], m[0, 2], m[0, 3] = 255, 255, 255, 254
    cover, box = E.mask_cover_u8(m.to(cuda), 2, 1)
    assert cover.tolist() == [[1, 0]] and box.tolist() == [0, 0, 1, 1, 1]


# ---- coverage -> a region's tensors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ratio", [0.0, 0.2, 1.0])
def test_mask_region(plugin, cuda, ratio):
    E = plugin.engine
    W, H = 40, 24
    cov = cases.canvas_cover(W, H)
    box = rr.box_of(cov)
    rects = [(box[0], box[1], box[2] - box[0], box[3] - box[1]), (0, 0, W, H), (5, 3, 21, 14), (W - 1, H - 6, 1, 6), (10, 8, 1, 1)]
    for (x, y, w, h) in rects:
        want_c, want_f = rr.region_tensors(cov, x, y, w, h, ratio)
        rcover, feather = E.mask_region(torch.from_numpy(cov).to(cuda), x, y, w, h, ratio)
        assert torch.equal(rcover.cpu(), torch.from_numpy(want_c)), (x, y, w, h)
        _assert_bitwise(feather, torch.from_numpy(want_f), f"feather of {(x, y, w, h)} at {ratio}")
        rcover, none = E.mask_region(torch.from_numpy(cov).to(cuda), x, y, w, h, None)
        assert none is None and torch.equal(rcover.cpu(), torch.from_numpy(want_c))
    full = torch.ones(H, W, dtype=torch.uint8, device=cuda)
    for (w, h) in [(8, 6), (14, 10), (12, 12), (2, 2), (30, 4)]:      # a fully covered rectangle of even size: upstream's feather_mask
        _, feather = E.mask_region(full, 3, 2, w, h, ratio)
        _assert_bitwise(feather, E.feather_mask(w, h, ratio, cuda).cpu(), f"full {w}x{h} at {ratio} against mdtile_feather_mask")


# ---- the noise ------------------------------------------------------------------------------------------------------------------------
def test_region_noise_masked(plugin, cuda):
    E = plugin.engine
    W, H = 40, 24
    torch.manual_seed(5)
    noise = torch.randn(N, C, H, W)
    regions = [(x, y, w, h, mode, torch.randn(1, C, h, w), cover) for (_, x, y, w, h, mode, cover) in cases.spec(W, H)]
    code = {"bg": E.REGION_BG, "fg": E.REGION_FG}
    dev = [(x, y, w, h, code[m], r.to(cuda), None if cv is None else torch.from_numpy(cv).to(cuda)) for (x, y, w, h, m, r, cv) in regions]
    got = E.region_noise_masked(noise.to(cuda), dev)
    want = rr.region_noise(noise.numpy(), [(x, y, w, h, m, r.numpy(), cv) for (x, y, w, h, m, r, cv) in regions])
    _assert_bitwise(got, torch.from_numpy(want), "region_noise_masked")
    assert not torch.equal(got.cpu(), noise)
    null = [r[:6] + (None,) for r in dev]
    _assert_bitwise(E.region_noise_masked(noise.to(cuda), null), E.region_noise(noise.to(cuda), [r[:6] for r in dev]).cpu(), "NULL covers against region_noise")


# ---- refused calls --------------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(plugin, cuda):
    """Every refusal is MDTILE_E_ARG with a text that names the reason, and leaves the NaN- / 7-painted outputs as they are."""
    E = plugin.engine
    plan = _plan(E, "base")
    W, H = plan.w, plan.h
    ones = [torch.ones(len(b) * N, C, plan.tile_h, plan.tile_w, device=cuda) for b in plan.batches]
    out = torch.full((N, C, H, W), NAN, device=cuda)
    some_map = torch.ones(H, W, device=cuda)

    def region(x, y, w, h, mode=E.REGION_BG, weight=True):
        return E.RegionSpec(x, y, w, h, mode, torch.ones(N, C, h, w, device=cuda), torch.ones(h, w, device=cuda) if weight else None,
                            torch.ones(h, w, dtype=torch.uint8, device=cuda))

    def refused(text, plan_=plan, method=E.METHOD_MD, batch=None, **kw):
        args = dict(regions=[], weights=some_map, out=out, dtype=torch.float32, device=cuda)
        args.update(kw)
        with pytest.raises(E.MdtileError, match=r"mdtile_blend_mask_regions failed \(rc=-1\).*" + text):
            E.blend_mask_regions(plan_, method, ones if batch is None else batch, N, C, **args)

    refused("wrap-x plan", plan_=E.Plan(W, H, 16, 16, 8, 4, wrap_x=True), batch=[])
    sparse = plan.subset([1] + [0] * (plan.num_tiles - 1), 4)
    refused("sparse plan", plan_=sparse, batch=[])
    refused(r"no MDTILE_BLEND_\* flags", flags=E.BLEND_PARTIAL)
    refused(r"no MDTILE_BLEND_\* flags", flags=E.BLEND_PACKED)
    refused("no row band", row_range=(0, 8))
    refused("17 regions", regions=[region(1, 1, 2, 2)] * 17)
    for (x, y, w, h) in [(W - 3, 1, 4, 4), (1, H - 3, 4, 4), (0, 0, W + 1, 2), (0, 0, 2, H + 1), (-1, 1, 4, 4)]:
        refused(r"region 1 \(.*\) leaves the %dx%d canvas" % (W, H), regions=[region(1, 1, 4, 4), region(x, y, w, h)])
    refused("region 0 bad mode 7", regions=[region(1, 1, 4, 4, mode=7)])
    refused("region 0 needs a weight", regions=[region(1, 1, 4, 4, E.REGION_FG, weight=False)])
    refused("bad method", method=9)
    refused("batches given", batch=ones[:-1] if len(ones) > 1 else ones + ones)
    refused("needs d_weights", weights=None)
    lib, check = E.lib(), E._check

    def raw(text, n=N, c=C, dtype=0, nb=None, x_out=True, batches=ones):
        """The C call itself: what the Python wrapper would stop first."""
        a = E._BlendArgs(E.METHOD_MD, dtype, n, c, 0, 0, 0, 0, 0, some_map.data_ptr(), None, None, out.data_ptr() if x_out else None)
        ptrs = (E.ctypes.c_void_p * max(1, len(batches)))(*[t.data_ptr() for t in batches])
        rc = lib.mdtile_blend_mask_regions(plan.handle, E.ctypes.byref(a), ptrs, len(batches) if nb is None else nb, None, 0, None)
        with pytest.raises(E.MdtileError, match=r"mdtile_blend_mask_regions failed \(rc=-1\).*" + text):
            check(rc, "mdtile_blend_mask_regions")

    raw("bad dtype 3", dtype=3)
    raw("bad dtype -1", dtype=-1)
    raw("bad N=65536 C=1", n=65536, c=1)
    raw("bad N=0", n=0)
    raw("null output", x_out=False)
    raw(r"%d batches \(max %d" % (E.MAX_BATCHES + 1, E.MAX_BATCHES), nb=E.MAX_BATCHES + 1)
    raw("bad num_batches -1", nb=-1)
    with pytest.raises(E.MdtileError, match=r"mdtile_blend_mask_regions failed \(rc=-1\).*null plan"):
        check(lib.mdtile_blend_mask_regions(None, None, None, 0, None, 0, None), "mdtile_blend_mask_regions")
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused blend wrote to its output"

    cover = torch.full((H, W), 7, dtype=torch.uint8, device=cuda)
    box = torch.full((5,), 7, dtype=torch.int32, device=cuda)
    mask = torch.zeros(8 * H, 8 * W, dtype=torch.uint8, device=cuda)
    for text, args in [("null", (None, 8 * W, 8 * H, W, H, cover.data_ptr(), box.data_ptr())),
                       ("null", (mask.data_ptr(), 8 * W, 8 * H, W, H, None, box.data_ptr())),
                       ("null", (mask.data_ptr(), 8 * W, 8 * H, W, H, cover.data_ptr(), None)),
                       ("bad canvas", (mask.data_ptr(), 8 * W, 8 * H, 0, H, cover.data_ptr(), box.data_ptr())),
                       ("smaller than the latent canvas", (mask.data_ptr(), W - 1, 8 * H, W, H, cover.data_ptr(), box.data_ptr())),
                       ("smaller than the latent canvas", (mask.data_ptr(), 8 * W, H - 1, W, H, cover.data_ptr(), box.data_ptr()))]:
        with pytest.raises(E.MdtileError, match=r"mdtile_mask_cover_u8 failed \(rc=-1\).*" + text):
            check(lib.mdtile_mask_cover_u8(*args, None), "mdtile_mask_cover_u8")
    rcover = torch.full((H, W), 7, dtype=torch.uint8, device=cuda)
    feather = torch.full((H, W), NAN, device=cuda)
    for text, args in [("null", (None, W, H, 0, 0, 4, 4, 0.2, rcover.data_ptr(), feather.data_ptr())),
                       ("null", (cover.data_ptr(), W, H, 0, 0, 4, 4, 0.2, None, feather.data_ptr())),
                       ("leaves the", (cover.data_ptr(), W, H, W - 3, 0, 4, 4, 0.2, rcover.data_ptr(), feather.data_ptr())),
                       ("leaves the", (cover.data_ptr(), W, H, 0, -1, 4, 4, 0.2, rcover.data_ptr(), feather.data_ptr())),
                       ("leaves the", (cover.data_ptr(), W, H, 0, 0, 4, 0, 0.2, rcover.data_ptr(), feather.data_ptr())),
                       ("feather_ratio", (cover.data_ptr(), W, H, 0, 0, 4, 4, 1.5, rcover.data_ptr(), feather.data_ptr())),
                       ("feather_ratio", (cover.data_ptr(), W, H, 0, 0, 4, 4, NAN, rcover.data_ptr(), feather.data_ptr()))]:
        with pytest.raises(E.MdtileError, match=r"mdtile_mask_region failed \(rc=-1\).*" + text):
            check(lib.mdtile_mask_region(*args, None), "mdtile_mask_region")
    noise = torch.full((N, C, H, W), NAN, device=cuda)
    rand = torch.ones(1, C, 4, 4, device=cuda)
    with pytest.raises(E.MdtileError, match=r"mdtile_region_noise_masked failed \(rc=-1\).*region 1 rect .* leaves the"):
        E.region_noise_masked(noise, [(0, 0, 4, 4, E.REGION_BG, rand, None), (W - 3, 0, 4, 4, E.REGION_BG, rand, None)])
    with pytest.raises(E.MdtileError, match=r"mdtile_region_noise_masked failed \(rc=-1\).*17 regions"):
        E.region_noise_masked(noise, [(0, 0, 4, 4, E.REGION_BG, rand, None)] * 17)
    with pytest.raises(E.MdtileError, match=r"mdtile_region_noise_masked failed \(rc=-1\).*mode 7"):
        E.region_noise_masked(noise, [(0, 0, 4, 4, 7, rand, None)])
    with pytest.raises(E.MdtileError, match=r"mdtile_region_noise_masked failed \(rc=-1\).*null"):
        check(lib.mdtile_region_noise_masked(None, N, C, H, W, None, 0, None), "mdtile_region_noise_masked")
    torch.cuda.synchronize()
    assert (cover == 7).all() and (box == 7).all() and (rcover == 7).all() and torch.isnan(feather).all() and torch.isnan(noise).all()


# ---- the delegates --------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def masks_dir(tmp_path):
    """The stub host with --mdtile-region-masks DIR; gone afterwards."""
    _, shared = sh.host()
    shared.cmd_opts.mdtile_region_masks = str(tmp_path)
    try:
        yield tmp_path, shared
    finally:
        if hasattr(shared.cmd_opts, "mdtile_region_masks"):
            delattr(shared.cmd_opts, "mdtile_region_masks")


@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_with_two_mask_files_and_a_rectangle(plugin, cuda, masks_dir, method, monkeypatch):
    """MultiDiffusion / MixtureOfDiffusers with region1.png (BG) and region3.png (FG) in the directory and region 2 a rectangle: rectangles, covers
    and feather are the restatement's of the files; the model ran on each rectangle; the result is the restatement's fed the same outputs.  Then
    the same job without the directory: no masked call is made."""
    folder, shared = masks_dir
    Wc, Hc, tw, th, ov, bs = cases.CANVASES["base"]
    E, U = plugin.engine, plugin.utils
    big = {1: np.kron(cases.canvas_cover(Wc, Hc), np.ones((8, 8), np.uint8)) * 255,
           3: np.kron(np.flipud(cases.canvas_cover(Wc, Hc)), np.ones((8, 8), np.uint8)) * 200}
    for k, m in big.items():
        Image.fromarray(m.astype(np.uint8), "L").save(os.path.join(folder, f"region{k}.png"))
    settings = {0: U.BBoxSettings(True, 0.9, 0.9, 0.05, 0.05, "", "", "Background", 0.2, -1),
                1: U.BBoxSettings(True, 0.2, 0.1, 0.6, 0.5, "", "", "Background", 0.2, -1),
                2: U.BBoxSettings(True, 0.0, 0.0, 0.1, 0.1, "", "", "Foreground", 0.3, -1)}
    cls = plugin.multidiffusion.MultiDiffusion if method == "md" else plugin.mixtureofdiffusers.MixtureOfDiffusers
    masked_calls = []
    real = E.blend_mask_regions
    monkeypatch.setattr(E, "blend_mask_regions", lambda *a, **k: (masked_calls.append(1), real(*a, **k))[1])

    def job():
        p = sh.make_processing(Wc * 8, Hc * 8)
        d = cls(p, sh.kdiff_sampler())
        d.init_grid_bbox(tw, th, ov, bs)
        d.init_custom_bbox(settings, True, False)
        d.init_done()
        if d.pbar is not None:
            d.pbar.close()
        d.update_pbar = lambda: None
        return d

    def evaluate(d, x):
        calls = []

        def model(t):
            calls.append(t.clone())
            return t * (-2.0) ** ((len(calls) % 5) - 2)
        if method == "md":
            out = d.sample_one_step(x.to(cuda), None, lambda xt, b: model(xt), lambda xt, i, b: model(xt))
        else:
            shared.sd_model.apply_model_original_md = lambda x_, t_, c_: model(x_)
            d.custom_apply_model = lambda xt, t_in, c_in, i, b: model(xt)
            cond = {"c_crossattn": [torch.zeros(N, 77, 768, device=cuda)], "c_concat": [torch.zeros(N, 5, 1, 1, device=cuda)]}
            out = d.apply_model_hijack(x.to(cuda), torch.zeros(N, device=cuda), cond)
        return out, calls

    d = job()
    assert d.mask_regions and len(d.custom_bboxes) == 3
    cov = {k: rr.cover_u8(m.astype(np.uint8), Wc, Hc) for k, m in big.items()}
    want_boxes = [(cov[1][1][0], cov[1][1][1], cov[1][1][2] - cov[1][1][0], cov[1][1][3] - cov[1][1][1]), (8, 2, 24, 12),
                  (cov[3][1][0], cov[3][1][1], cov[3][1][2] - cov[3][1][0], cov[3][1][3] - cov[3][1][1])]
    assert [(b.x, b.y, b.w, b.h) for b in d.custom_bboxes] == want_boxes
    rc1, _ = rr.region_tensors(cov[1][0], *want_boxes[0], None)
    rc3, f3 = rr.region_tensors(cov[3][0], *want_boxes[2], 0.3)
    assert torch.equal(d.custom_bboxes[0].cover.cpu(), torch.from_numpy(rc1)) and d.custom_bboxes[1].cover is None
    assert torch.equal(d.custom_bboxes[2].cover.cpu(), torch.from_numpy(rc3))
    _assert_bitwise(d.custom_bboxes[2].feather_mask, torch.from_numpy(f3), "the FG region's feather")
    torch.manual_seed(3)
    x = torch.randn(N, C, Hc, Wc)
    out, calls = evaluate(d, x)
    assert masked_calls == [1]
    plan = d.plan
    nb = plan.num_batches
    assert len(calls) == nb + 3
    cut = lambda box: np.ascontiguousarray(x.numpy()[:, :, box[1]:box[1] + box[3], box[0]:box[0] + box[2]])
    for i, box in enumerate(want_boxes):
        _assert_bitwise(calls[nb + i], torch.from_numpy(cut(box)), f"the tile of region {i}")
    scale = lambda k: np.float32((-2.0) ** (((k + 1) % 5) - 2))
    tiles = np.concatenate([calls[b].cpu().numpy() * scale(b) for b in range(nb)], axis=0)
    boxes = [tuple(b) for b in plan.bboxes]
    gauss = [bo.gaussian_weights(b[2], b[3]).numpy() for b in want_boxes]
    shapes = [rr.Region(*want_boxes[0], "bg", None, None, rc1), rr.Region(*want_boxes[1], "bg", None, None, None),
              rr.Region(*want_boxes[2], "fg", None, None, rc3)]
    tile_w = bo.gaussian_weights(plan.tile_w, plan.tile_h).numpy() if method == "mod" else None
    grid_w = bo.grid_weight_map(Wc, Hc, boxes, 1.0 if method == "md" else torch.from_numpy(tile_w)).numpy()[0, 0]
    weights = rr.weight_sum(grid_w, method, shapes, gauss)
    _assert_bitwise(d.weights[0, 0], torch.from_numpy(weights), "the delegate's weight sum")
    with np.errstate(all="ignore"):
        rescale = (np.float32(1.0) / weights).astype(np.float32)
    ref = []
    for i, R in enumerate(shapes):
        wgt = f3 if R.mode == "fg" else (None if method == "md" else rr.premultiplied(gauss[i], R, rescale))
        ref.append(R._replace(out=cut(want_boxes[i]) * scale(nb + i), weight=wgt))
    want = rr.blend(Wc, Hc, boxes, method, tiles, N, C, ref, weights, tile_w, rescale)
    _assert_bitwise(out, torch.from_numpy(want), f"delegate {method} with mask regions")

    # no mask: the calls of before
    delattr(shared.cmd_opts, "mdtile_region_masks")
    masked_calls.clear()
    monkeypatch.setattr(E, "mask_cover_u8", lambda *a, **k: pytest.fail("mask_cover_u8 called without a mask"))
    monkeypatch.setattr(E, "mask_region", lambda *a, **k: pytest.fail("mask_region called without a mask"))
    d = job()
    assert not d.mask_regions and all(b.cover is None for b in d.custom_bboxes) and len(d.custom_bboxes) == 3
    evaluate(d, x)
    assert masked_calls == []
