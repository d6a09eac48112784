"""Region control on a wrap-around canvas (mdtile_blend_wrap_regions and the three rect calls, csrc/wrap_regions.hip) on the GPU,
BITWISE against the numpy restatement tests/wrap_region_ref.py: background and foreground regions that cross one seam or both, overlapping
regions of each kind, a region as wide as the canvas, a 1 x 1 region in the last column, regions only, on the grid at rest and shifted; both
methods in fp32, fp16 and bf16; every planes-per-thread instantiation; the equalities with mdtile_blend_shift / mdtile_blend and with the plain
rect calls; every refusal by name with its output left untouched; and both delegates with --mdtile-wrap-x --mdtile-wrap-regions, with and
without --mdtile-grid-shift.  No tolerance appears in this file; half types follow tests/test_gpu_blend_matrix.py (inputs rounded to the dtype, the
fp32 restatement evaluated on those values, rounded once).

The shapes are the smallest at which each branch can go wrong (a seam inside a quad, a last quad of 2 pixels, a shift that cuts the stored quad),
not the workload's.  Every case runs N = 2, C = 4 unless it is there for the planes."""
import functools

import numpy as np
import pytest
import torch

from hostsim import stub_host as sh

import shift_ref as sr
import wrap_ref as wr
import wrap_region_ref as rr
from wrap_common import DT, NAN, N, C, assert_bitwise as _assert_bitwise, maps as _maps, set_options as _set_options, take as _take

pytestmark = pytest.mark.gpu

# id -> (W, H, requested tile_w, tile_h, overlap, wrap_x, wrap_y, tile_bs)
CASES = {
    "cylinder": (40, 24, 24, 24, 16, 1, 0, 2),     # the wrap tests' shape: columns 0, 8, .., 32, three tiles on every pixel
    "torus": (40, 40, 24, 24, 16, 1, 1, 2),        # 3 x 3 tiles on every pixel
    "w38": (38, 20, 16, 16, 4, 1, 1, 4),           # the last quad has 2 valid pixels; 1 - 4 tiles on a pixel
    "strip_y": (36, 27, 16, 12, 6, 0, 1, 4),       # wrap-y only: plain columns under cyclic rows
}
# the launcher's 2- and 4-planes-per-thread forms: H * ceil(W / 4) * planes / 2 = 131072 at 16 planes, / 4 = 131072 at 32
PLANES = {"planes2": (512, 128, 96, 96, 48, 1, 1, 8, 4, 4), "planes4": (512, 128, 96, 96, 48, 1, 1, 8, 4, 8)}      # .. N, C


@functools.lru_cache(maxsize=None)
def _grid(case):
    W, H, tw, th, ov, wx, wy, bs = (CASES.get(case) or PLANES[case])[:8]
    g = wr.grid(W, H, tw, th, ov, bs, bool(wx), bool(wy))
    assert g is not None
    return g


def _flags(case):
    return tuple(bool(v) for v in (CASES.get(case) or PLANES[case])[5:7])


def _shifts(case):
    """At rest, an odd shift, next to both seams, one axis only -- each restricted to the axes that wrap."""
    g, (wx, wy) = _grid(case), _flags(case)
    out = []
    for sx, sy in [(0, 0), (5, 3), (g.W - 1, g.H - 1), (7, 0), (0, 2)]:
        s = (sx if wx else 0, sy if wy else 0)
        if s not in out:
            out.append(s)
    return out


def _spec(case):
    """(x, y, w, h, mode) in list order: a BG region across the x seam, an FG region across both seams of a torus, a second FG region over it
    (fcnt = 2), two overlapping BG regions wholly inside, a BG band as wide as the canvas, a 1 x 1 BG region in the last column, an FG column as
    tall as the canvas.  On an axis that does not wrap the same regions lie inside.  FG over BG over grid happens where they meet."""
    g, (wx, wy) = _grid(case), _flags(case)
    W, H = g.W, g.H
    xs, ys = (W - 6 if wx else 3), (H - 4 if wy else 2)
    spec = [(xs, 2, 14, 8, "bg"), (W - 5 if wx else 5, ys, 11, 9, "fg"), (W - 2 if wx else 9, (ys + 3) % H if wy else ys + 1, 9, 7, "fg"),
            (4, 3, 10, 8, "bg"), (8, 5, 10, 8, "bg"), (10 if wx else 0, 6, W, 3, "bg"), (W - 1, 0, 1, 1, "bg"), (2, 5 if wy else 0, 3, H, "fg")]
    assert all(rr.rect_valid(W, H, x, y, w, h, wx, wy) for (x, y, w, h, _) in spec), spec
    assert (not wx or sum(x + w > W for (x, _, w, _, _) in spec) >= 4) and (not wy or sum(y + h > H for (_, y, _, h, _) in spec) >= 3)
    return spec


@functools.lru_cache(maxsize=None)
def _data(case, dt, n=N, c=C):
    """(tile batches, regions) on the CPU in the dtype: random normal model outputs, feather masks in [0, 1), the raw Gaussian of every BG region."""
    g = _grid(case)
    torch.manual_seed(len(case) + 41)
    tiles = [torch.randn(len(b) * n, c, g.th, g.tw).to(DT[dt]) for b in g.batches]
    regions = []
    for (x, y, w, h, mode) in (_spec(case) if case in CASES else [(500, 120, 40, 20, "bg"), (250, 100, 33, 60, "fg"), (508, 3, 9, 9, "fg")]):
        out = torch.randn(n, c, h, w).to(DT[dt])
        weight = torch.rand(h, w) if mode == "fg" else torch.from_numpy(wr.gaussian(w, h))
        regions.append((x, y, w, h, mode, out, weight))
    return tiles, regions


def _ref_regions(regions, method):
    return [rr.Region(x, y, w, h, mode, out.float().numpy(), None if (mode == "bg" and method == "md") else weight.numpy())
            for (x, y, w, h, mode, out, weight) in regions]


def _dev_regions(E, regions, method, cuda):
    return [E.RegionSpec(x, y, w, h, E.REGION_FG if mode == "fg" else E.REGION_BG, out.to(cuda),
                         None if (mode == "bg" and method == "md") else weight.to(cuda)) for (x, y, w, h, mode, out, weight) in regions]


def _region_w(E, g, regions, method, cuda, flags):
    """The background regions' weight sum through the library, checked against the restatement."""
    m = torch.zeros(g.H, g.W, device=cuda)
    for (x, y, w, h, mode, _, weight) in regions:
        if mode == "bg":
            E.weight_map_add_rect_wrap(m, x, y, w, h, None if method == "md" else weight.to(cuda), 1.0, wrap_x=flags[0], wrap_y=flags[1])
    want = rr.region_w_map(g.W, g.H, method, _ref_regions(regions, method))
    _assert_bitwise(m, torch.from_numpy(want), f"region_w {method}")
    return m, want


def _plan(E, case):
    W, H, tw, th, ov, wx, wy, bs = (CASES.get(case) or PLANES[case])[:8]
    plan = E.Plan(W, H, tw, th, ov, bs, wrap_x=bool(wx), wrap_y=bool(wy))
    g = _grid(case)
    assert plan.bboxes == list(g.boxes) and plan.tile_bs == g.tile_bs and plan.num_batches == len(g.batches)
    return plan


def _method(E, method):
    return E.METHOD_MD if method == "md" else E.METHOD_MOD


def _blend_case(plugin, cuda, case, method, dt, shifts, n=N, c=C, with_grid=True):
    E, g, dtype, flags = plugin.engine, _grid(case), DT[dt], _flags(case)
    plan = _plan(E, case)
    m = _maps(E, plan, cuda)
    tiles, regions = _data(case, dt, n, c)
    region_w, region_w_np = _region_w(E, g, regions, method, cuda, flags)
    grid_w = (m.weights if method == "md" else m.gsum) if with_grid else None
    tile_w = m.tile_w if method == "mod" and with_grid else None
    batch = [t.to(cuda) for t in tiles] if with_grid else []
    dev_regions = _dev_regions(E, regions, method, cuda)
    ref_regions = _ref_regions(regions, method)
    ref_tiles = torch.cat(tiles, dim=0).float().numpy() if with_grid else None
    for (sx, sy) in shifts:
        out = torch.full((n, c, g.H, g.W), NAN, dtype=dtype, device=cuda)
        got = E.blend_wrap_regions(plan, _method(E, method), batch, n, c, regions=dev_regions, grid_w=grid_w, region_w=region_w, sx=sx, sy=sy,
                                   tile_w=tile_w, out=out)
        assert got.dtype == dtype
        want = rr.blend(g, method, ref_tiles, n, c, sx, sy, None if grid_w is None else grid_w.cpu().numpy(), region_w_np, ref_regions,
                        None if tile_w is None else tile_w.cpu().numpy())
        if with_grid:
            assert np.isfinite(want).all()
        _assert_bitwise(got, torch.from_numpy(want).to(dtype), f"{case} {method} {dt} blend_wrap_regions ({sx}, {sy})")


# ---- the blend ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_blend_wrap_regions_bitwise(plugin, cuda, case, method, dt):
    """Grid, then BG regions, the MultiDiffusion division, then the FG composite -- equal to the sequential fp32 loop, rounded once, at every shift."""
    _blend_case(plugin, cuda, case, method, dt, _shifts(case))


@pytest.mark.parametrize("case", list(PLANES))
@pytest.mark.parametrize("method", ["md", "mod"])
def test_every_planes_per_thread_form(plugin, cuda, case, method):
    n, c = PLANES[case][8:]
    work = 128 * (512 // 4) * n * c
    assert (work // 4 >= 131072) == (case == "planes4") and work // 2 >= 131072
    _blend_case(plugin, cuda, case, method, "f32", [(5, 3)], n, c)


@pytest.mark.parametrize("method", ["md", "mod"])
def test_regions_only(plugin, cuda, method):
    """num_batches = 0: no grid is drawn, grid_w is None; a pixel nobody covers comes out +0.0 (Mixture of Diffusers never multiplies its inf)."""
    g = _grid("torus")
    regions = [r for r in _data("torus", "f32")[1] if r[2] < g.W and r[3] < g.H]
    cover = np.zeros((g.H, g.W), bool)
    for (x, y, w, h, *_r) in regions:
        cover[rr.index(g.W, g.H, x, y, w, h)] = True
    assert not cover.all() and cover.any()
    E, flags = plugin.engine, _flags("torus")
    plan = _plan(E, "torus")
    region_w, region_w_np = _region_w(E, g, regions, method, cuda, flags)
    for (sx, sy) in [(0, 0), (5, 3)]:
        out = torch.full((N, C, g.H, g.W), NAN, device=cuda)
        got = E.blend_wrap_regions(plan, _method(E, method), [], N, C, regions=_dev_regions(E, regions, method, cuda), grid_w=None, region_w=region_w,
                                   sx=sx, sy=sy, out=out)
        want = rr.blend(g, method, None, N, C, sx, sy, None, region_w_np, _ref_regions(regions, method))
        assert (want[:, :, ~cover] == 0).all() and np.isfinite(want).all()
        _assert_bitwise(got, torch.from_numpy(want), f"regions only {method} ({sx}, {sy})")


@pytest.mark.parametrize("case", ["cylinder", "torus", "w38"])
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_without_regions_it_is_the_shifted_blend(plugin, cuda, case, method, dt):
    """No regions and a zero region_w: mdtile_blend_shift with the plan's own maps, bit for bit; at shift 0 mdtile_blend."""
    E, g, dtype = plugin.engine, _grid(case), DT[dt]
    plan = _plan(E, case)
    m = _maps(E, plan, cuda)
    batch = [t.to(cuda) for t in _data(case, dt)[0]]
    zeros = torch.zeros(g.H, g.W, device=cuda)
    kw = dict(weights=m.weights) if method == "md" else dict(tile_w=m.tile_w, rescale=m.rescale)
    for (sx, sy) in _shifts(case):
        out = torch.full((N, C, g.H, g.W), NAN, dtype=dtype, device=cuda)
        got = E.blend_wrap_regions(plan, _method(E, method), batch, N, C, grid_w=m.weights if method == "md" else m.gsum, region_w=zeros, sx=sx, sy=sy,
                                   tile_w=m.tile_w if method == "mod" else None, out=out)
        _assert_bitwise(got, E.blend_shift(plan, _method(E, method), batch, N, C, sx=sx, sy=sy, **kw).cpu(), f"{case} {method} {dt} vs blend_shift ({sx}, {sy})")
        if (sx, sy) == (0, 0):
            _assert_bitwise(got, E.blend(plan, _method(E, method), batch, N, C, **kw).cpu(), f"{case} {method} {dt} vs blend")


# ---- the rect calls ----------------------------------------------------------------------------------------------------------------
RECTS = [(36, 20, 9, 11), (0, 0, 40, 24), (39, 23, 1, 1), (39, 0, 40, 5), (7, 23, 5, 24), (3, 4, 10, 9)]      # on a 40 x 24 torus; the last lies inside


@pytest.mark.parametrize("dt", list(DT))
def test_gather_rect_wrap(plugin, cuda, dt):
    E = plugin.engine
    torch.manual_seed(3)
    x = torch.randn(N, C, 24, 40).to(DT[dt])
    xd = x.to(cuda)
    raw = x.view(torch.int32 if dt == "f32" else torch.int16).numpy()
    for (rx, ry, w, h) in RECTS:
        got = E.gather_rect_wrap(xd, rx, ry, w, h, wrap_x=True, wrap_y=True)
        want = np.take(np.take(raw, ry + np.arange(h), axis=-2, mode="wrap"), rx + np.arange(w), axis=-1, mode="wrap")
        assert np.array_equal(got.cpu().view(torch.from_numpy(raw).dtype).numpy(), want), (dt, rx, ry, w, h)
    rx, ry, w, h = RECTS[-1]
    for flags in ((True, True), (False, False), (True, False)):
        got = E.gather_rect_wrap(xd, rx, ry, w, h, wrap_x=flags[0], wrap_y=flags[1])
        _assert_bitwise(got, E.gather_rect(xd, rx, ry, w, h).cpu(), f"gather_rect_wrap inside the canvas {flags}")


def test_weight_map_add_rect_wrap(plugin, cuda):
    E = plugin.engine
    torch.manual_seed(4)
    base = torch.rand(24, 40)
    got, want = base.to(cuda), base.numpy().copy()
    for i, (rx, ry, w, h) in enumerate(RECTS):
        rect_w = torch.rand(h, w) if i % 2 == 0 else None
        E.weight_map_add_rect_wrap(got, rx, ry, w, h, None if rect_w is None else rect_w.to(cuda), 0.75, wrap_x=True, wrap_y=True)
        rr.weight_map_add_rect(want, rx, ry, w, h, None if rect_w is None else rect_w.numpy(), 0.75)
        _assert_bitwise(got, torch.from_numpy(want), f"weight_map_add_rect_wrap {(rx, ry, w, h)}")
    rx, ry, w, h = RECTS[-1]
    rect_w = torch.rand(h, w, device=cuda)
    a, b = base.to(cuda), base.to(cuda)
    E.weight_map_add_rect_wrap(a, rx, ry, w, h, rect_w, wrap_x=True, wrap_y=False)
    E.weight_map_add_rect(b, rx, ry, w, h, rect_w)
    _assert_bitwise(a, b.cpu(), "weight_map_add_rect_wrap inside the canvas")


def test_region_noise_wrap(plugin, cuda):
    E = plugin.engine
    torch.manual_seed(5)
    noise = torch.randn(N, C, 24, 40)
    modes = ["bg", "fg", "bg", "bg", "fg", "fg"]
    regions = [(rx, ry, w, h, mode, torch.randn(1, C, h, w)) for (rx, ry, w, h), mode in zip(RECTS, modes)]
    code = {"bg": E.REGION_BG, "fg": E.REGION_FG}
    for picked in (regions, regions[:1] + regions[2:3] + regions[4:], regions[2:4]):
        got = E.region_noise_wrap(noise.to(cuda), [(x, y, w, h, code[m], r.to(cuda)) for (x, y, w, h, m, r) in picked], wrap_x=True, wrap_y=True)
        want = rr.region_noise(noise.numpy(), [(x, y, w, h, m, r.numpy()) for (x, y, w, h, m, r) in picked])
        _assert_bitwise(got, torch.from_numpy(want), f"region_noise_wrap, {len(picked)} regions")
    inside = [(3, 4, 10, 9, E.REGION_BG, torch.randn(1, C, 9, 10, device=cuda)), (8, 6, 12, 10, E.REGION_BG, torch.randn(1, C, 10, 12, device=cuda)),
              (30, 10, 10, 14, E.REGION_FG, torch.randn(1, C, 14, 10, device=cuda))]
    got = E.region_noise_wrap(noise.to(cuda), inside, wrap_x=True, wrap_y=False)
    _assert_bitwise(got, E.region_noise(noise.to(cuda), inside).cpu(), "region_noise_wrap inside the canvas")


# ---- refused calls -----------------------------------------------------------------------------------------------------------------
BAD_RECTS = [  # (x, y, w, h, wrap_x, wrap_y, the text) on a 40 x 24 canvas
    (0, 0, 41, 5, True, True, "does not fit"), (0, 0, 5, 25, True, True, "does not fit"), (40, 0, 5, 5, True, True, "does not fit"),
    (-1, 0, 5, 5, True, True, "does not fit"), (0, 24, 5, 5, True, True, "does not fit"), (0, -2, 5, 5, True, True, "does not fit"),
    (0, 0, 0, 5, True, True, "does not fit"), (36, 2, 9, 5, False, True, "passes the right edge.*x axis does not wrap"),
    (3, 20, 9, 5, True, False, "passes the bottom edge.*y axis does not wrap"),
]


def test_refused_rect_calls_write_nothing(plugin, cuda):
    E = plugin.engine
    assert E.E_ARG == -1
    x = torch.zeros(N, C, 24, 40, device=cuda)
    for (rx, ry, w, h, wx, wy, text) in BAD_RECTS:
        out = torch.full((N, C, 30, 50), NAN, device=cuda)
        with pytest.raises(E.MdtileError, match=r"mdtile_gather_rect_wrap failed \(rc=-1\).*" + text):
            E.gather_rect_wrap(x, rx, ry, max(w, 0), max(h, 0), wrap_x=wx, wrap_y=wy, out=out)
        weights = torch.full((24, 40), NAN, device=cuda)
        rect_w = torch.ones(max(h, 1), max(w, 1), device=cuda)
        with pytest.raises(E.MdtileError, match=r"mdtile_weight_map_add_rect_wrap failed \(rc=-1\).*" + text):
            E._check(E.lib().mdtile_weight_map_add_rect_wrap(weights.data_ptr(), 40, 24, rx, ry, w, h, rect_w.data_ptr(), 1.0, int(wx), int(wy), None),
                     "mdtile_weight_map_add_rect_wrap")
        noise = torch.full((N, C, 24, 40), NAN, device=cuda)
        good = (3, 4, 10, 9, E.REGION_BG, torch.ones(1, C, 9, 10, device=cuda))
        bad = (rx, ry, w, h, E.REGION_FG, torch.ones(1, C, max(h, 1), max(w, 1), device=cuda))
        arr = (E._Region * 2)(E._Region(*good[:5], 0, good[5].data_ptr(), None), E._Region(*bad[:5], 0, bad[5].data_ptr(), None))
        with pytest.raises(E.MdtileError, match=r"mdtile_region_noise_wrap failed \(rc=-1\).*region 1 rect.*" + text):
            E._check(E.lib().mdtile_region_noise_wrap(noise.data_ptr(), N, C, 24, 40, arr, 2, int(wx), int(wy), None), "mdtile_region_noise_wrap")
        torch.cuda.synchronize()
        assert torch.isnan(out).all() and torch.isnan(weights).all() and torch.isnan(noise).all(), f"a refused call wrote to its output: {(rx, ry, w, h)}"
    noise = torch.full((N, C, 24, 40), NAN, device=cuda)
    many = [(1, 1, 2, 2, E.REGION_BG, torch.ones(1, C, 2, 2, device=cuda))] * 17
    with pytest.raises(E.MdtileError, match=r"mdtile_region_noise_wrap failed \(rc=-1\).*17 regions"):
        E.region_noise_wrap(noise, many, wrap_x=True, wrap_y=True)
    with pytest.raises(E.MdtileError, match=r"mdtile_gather_rect_wrap failed \(rc=-1\).*null"):
        E._check(E.lib().mdtile_gather_rect_wrap(0, N, C, 40, 24, None, 0, 0, 4, 4, 1, 1, noise.data_ptr(), None), "mdtile_gather_rect_wrap")
    with pytest.raises(E.MdtileError, match=r"mdtile_weight_map_add_rect_wrap failed \(rc=-1\).*null"):
        E._check(E.lib().mdtile_weight_map_add_rect_wrap(None, 40, 24, 0, 0, 4, 4, None, 1.0, 1, 1, None), "mdtile_weight_map_add_rect_wrap")
    with pytest.raises(E.MdtileError, match=r"mdtile_region_noise_wrap failed \(rc=-1\).*null"):
        E._check(E.lib().mdtile_region_noise_wrap(None, N, C, 24, 40, None, 0, 1, 1, None), "mdtile_region_noise_wrap")
    torch.cuda.synchronize()
    assert torch.isnan(noise).all()


def test_refused_blends_write_nothing(plugin, cuda):
    E = plugin.engine
    W, H, tw, th, ov, _, _, bs = CASES["torus"]
    torus, ring = _plan(E, "torus"), _plan(E, "strip_y")
    out = torch.full((N, C, H, W), NAN, device=cuda)
    zeros, ones = torch.zeros(H, W, device=cuda), torch.ones(H, W, device=cuda)

    def batches(plan):
        return [torch.ones(len(b) * N, C, plan.tile_h, plan.tile_w, device=cuda) for b in plan.batches]

    def region(x, y, w, h, mode=E.REGION_BG, weight=True):
        return E.RegionSpec(x, y, w, h, mode, torch.ones(N, C, h, w, device=cuda), torch.ones(h, w, device=cuda) if weight else None)

    def refused(text, plan=torus, method=E.METHOD_MD, batch=None, o=out, **kw):
        args = dict(regions=[], grid_w=ones, region_w=zeros, out=o, dtype=torch.float32, device=cuda)
        args.update(kw)
        with pytest.raises(E.MdtileError, match=r"mdtile_blend_wrap_regions failed \(rc=-1\).*" + text):
            E.blend_wrap_regions(plan, method, batches(plan) if batch is None else batch, N, C, **args)

    # the rectangles
    for (rx, ry, w, h, text) in [(0, 0, W + 1, 5, "does not fit"), (0, 0, 5, H + 1, "does not fit"), (W, 0, 5, 5, "does not fit"), (0, H, 5, 5, "does not fit"),
                                 (-1, 0, 5, 5, "does not fit"), (0, -1, 5, 5, "does not fit")]:
        refused("region 1.*" + text, regions=[region(1, 1, 4, 4), region(rx, ry, w, h)])
    ring_out = torch.full((N, C, ring.h, ring.w), NAN, device=cuda)
    ring_maps = dict(grid_w=torch.ones(ring.h, ring.w, device=cuda), region_w=torch.zeros(ring.h, ring.w, device=cuda), o=ring_out)
    refused("region 0.*passes the right edge.*x axis does not wrap", plan=ring, regions=[region(30, 2, 9, 5)], **ring_maps)
    # the plan and the shift
    plain = E.Plan(W, H, tw, th, ov, bs)
    refused("plain plan", plan=plain)
    refused("sparse plan", plan=plain.subset([1] + [0] * (plain.num_tiles - 2) + [1], bs))
    for (sx, sy) in ((W, 0), (0, H), (-1, 0), (0, -3)):
        refused("out of range", sx=sx, sy=sy)
    refused("x axis does not wrap", plan=ring, sx=1, sy=0, **ring_maps)
    # the count, the flags, the maps, the pointers
    refused("17 regions", regions=[region(1, 1, 2, 2)] * 17)
    refused("d_weights and d_rescale must be NULL", weights=ones)
    refused("d_weights and d_rescale must be NULL", method=E.METHOD_MOD, tile_w=torch.ones(th, tw, device=cuda), rescale=ones)
    refused("null d_region_w", region_w=None)
    refused("d_grid_w must be NULL iff num_batches == 0", grid_w=None)
    refused("d_grid_w must be NULL iff num_batches == 0", batch=[])
    refused("batches given", batch=batches(torus)[:1])
    refused("Mixture of Diffusers needs d_tile_w", method=E.METHOD_MOD)
    refused("region 0 needs a weight", regions=[region(1, 1, 4, 4, E.REGION_FG, weight=False)])
    refused("region 0 needs a weight", method=E.METHOD_MOD, tile_w=torch.ones(th, tw, device=cuda), regions=[region(1, 1, 4, 4, weight=False)])
    refused("region 0 bad mode", regions=[region(1, 1, 4, 4, mode=7)])
    a = E._BlendArgs(E.METHOD_MD, E.DT_F32, N, C, 0, 0, 0, 0, 0, None, None, None, out.data_ptr())
    ptrs = (E.c_void_p * torus.num_batches)(*[t.data_ptr() for t in batches(torus)])
    wr_ = E._WrapRegions(None, 0, ones.data_ptr(), zeros.data_ptr(), 0, 0)
    call = E.lib().mdtile_blend_wrap_regions
    for flags, rows, text in ((E.BLEND_PARTIAL, (0, 0), "no MDTILE_BLEND_\\* flags"), (E.BLEND_PACKED, (0, 0), "no MDTILE_BLEND_\\* flags"),
                              (E.BLEND_TILE_RANGE, (0, 0), "no MDTILE_BLEND_\\* flags"), (0, (0, 8), "no row band")):
        a.flags, a.row_lo, a.row_hi = flags, rows[0], rows[1]
        with pytest.raises(E.MdtileError, match=text):
            E._check(call(torus.handle, E.ctypes.byref(a), ptrs, torus.num_batches, E.ctypes.byref(wr_), None), "mdtile_blend_wrap_regions")
    a.flags, a.row_lo, a.row_hi = 0, 0, 0
    for plan_h, args, wrp, text in ((None, E.ctypes.byref(a), E.ctypes.byref(wr_), "null plan"), (torus.handle, None, E.ctypes.byref(wr_), "null plan"),
                                    (torus.handle, E.ctypes.byref(a), None, "null plan")):
        with pytest.raises(E.MdtileError, match=text):
            E._check(call(plan_h, args, ptrs, torus.num_batches, wrp, None), "mdtile_blend_wrap_regions")
    a.d_x_out = None
    with pytest.raises(E.MdtileError, match="null output"):
        E._check(call(torus.handle, E.ctypes.byref(a), ptrs, torus.num_batches, E.ctypes.byref(wr_), None), "mdtile_blend_wrap_regions")
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ring_out).all(), "a refused blend wrote to its output"
    # and the calls of before keep refusing regions on such a plan
    with pytest.raises(E.MdtileError, match="takes no custom regions"):
        E.blend(torus, E.METHOD_MD, batches(torus), N, C, weights=ones, regions=[region(1, 1, 4, 4)], out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- the delegates with the options set ----------------------------------------------------------------------------------------------
@pytest.fixture
def options():
    """set(shift) puts --mdtile-wrap-x --mdtile-wrap-regions (and --mdtile-grid-shift) on the stub host's command line; all gone afterwards."""
    _, shared = sh.host()

    def clear():
        _set_options(shared, False, False)
        for name in ("mdtile_grid_shift", "mdtile_wrap_regions"):
            if hasattr(shared.cmd_opts, name):
                delattr(shared.cmd_opts, name)

    def set_(shift):
        clear()
        shared.cmd_opts.mdtile_wrap_x = shared.cmd_opts.mdtile_wrap_regions = True
        if shift:
            shared.cmd_opts.mdtile_grid_shift = True
        return shared

    clear()
    step = shared.state.sampling_step
    try:
        yield set_
    finally:
        clear()
        shared.state.sampling_step = step


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_blends_regions_across_the_seam(plugin, cuda, options, method, shift):
    """MultiDiffusion / MixtureOfDiffusers with a BG and an FG region that cross the seam, over two sampler steps: the result is the
    restatement's fed the same outputs, the stand-in model ran once per tile batch and once per region, and every region's tile is the wrapped
    cut of x_in.  The stand-in multiplies its input by a power of two that depends on which call it is."""
    W, H, tw, th, ov, bs, seed = 37, 22, 16, 12, 6, 4, 1234567
    g = wr.grid(W, H, tw, th, ov, bs, True, False)
    shared = options(shift)
    U = plugin.utils
    cls = plugin.multidiffusion.MultiDiffusion if method == "md" else plugin.mixtureofdiffusers.MixtureOfDiffusers
    p = sh.make_processing(W * 8, H * 8)
    p.all_seeds = [seed]
    d = cls(p, sh.kdiff_sampler())
    d.init_grid_bbox(tw, th, ov, bs)
    settings = {0: U.BBoxSettings(True, 0.9, 0.5, 0.4, 0.3, "", "", "Background", 0.2, -1),
                1: U.BBoxSettings(True, 0.95, 0.1, 0.2, 0.2, "", "", "Foreground", 0.3, -1)}
    d.init_custom_bbox(settings, True, False)
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    d.update_pbar = lambda: None
    assert d.wrap_regions and d.grid_shift == shift and d.plan.bboxes == list(g.boxes) and p.extra_generation_params["Tiled Diffusion wrap regions"] is True
    boxes = [(b.x, b.y, b.w, b.h) for b in d.custom_bboxes]
    assert boxes == [(33, 11, 15, 7), (35, 2, 8, 5)] and d.wrap_ext >= 11
    grid_w = d.weights.cpu().numpy()[0, 0]
    tile_w = d.get_tile_weights().cpu().numpy() if method == "mod" else None
    feather = d.custom_bboxes[1].feather_mask.cpu().numpy().reshape(5, 8)
    bg_w = d.custom_weights[0].cpu().numpy().reshape(7, 15) if method == "mod" else None
    torch.manual_seed(9)
    x = torch.randn(N, C, H, W)
    scale = lambda k: (-2.0) ** ((k % 5) - 2)
    for step in range(2):
        shared.state.sampling_step = step
        sx = sr.PINNED[(seed, step, 0, W)] if shift else 0
        calls = []

        def model(t):
            calls.append(t.clone())
            return t * scale(len(calls) - 1)

        if method == "md":
            out = d.sample_one_step(x.to(cuda), None, lambda xt, bboxes: model(xt), lambda xt, bbox_id, bbox: model(xt))
        else:
            d.custom_apply_model = lambda xt, t_in, c_in, bbox_id, bbox: model(xt)
            shared.sd_model.apply_model_original_md = lambda x_, t_, c_: model(x_)
            cond = {"c_crossattn": [torch.zeros(N, 77, 768, device=cuda)], "c_concat": [torch.zeros(N, 5, 1, 1, device=cuda)]}
            out = d.apply_model_hijack(x.to(cuda), torch.zeros(N, device=cuda), cond)
        nb = len(g.batches)
        assert len(calls) == nb + 2, "one call per tile batch and one per region"
        tiles = [sr.gather(g, x.numpy(), b, sx, 0) for b in range(nb)]
        for b in range(nb):
            _assert_bitwise(calls[b], torch.from_numpy(tiles[b]), f"{method} step {step}: the model's input of batch {b}")
        for i, box in enumerate(boxes):
            _assert_bitwise(calls[nb + i], torch.from_numpy(np.ascontiguousarray(_take(x, box))), f"{method} step {step}: the tile of region {i}")
        ref_tiles = np.concatenate([t * np.float32(scale(b)) for b, t in enumerate(tiles)], axis=0)
        outs = [np.ascontiguousarray(_take(x, box)) * np.float32(scale(nb + i)) for i, box in enumerate(boxes)]
        regions = [rr.Region(*boxes[0], "bg", outs[0], bg_w), rr.Region(*boxes[1], "fg", outs[1], feather)]
        region_w = rr.region_w_map(W, H, method, regions)
        _assert_bitwise(d.region_w[0, 0], torch.from_numpy(region_w), f"{method}: the delegate's region_w")
        want = rr.blend(g, method, ref_tiles, N, C, sx, 0, grid_w, region_w, regions, tile_w)
        _assert_bitwise(out, torch.from_numpy(want), f"delegate {method} step {step} shift ({sx}, 0)")
