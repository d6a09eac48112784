"""Region prompt control under the jittered grid (mdtile_blend_lattice_regions, csrc/lattice.hip) on the GPU, BITWISE
against the numpy restatement tests/lattice_region_ref.py: background and foreground regions on the lattices of DESIGN.md 3.18's set at rest and
shifted, both methods in fp32, fp16 and bf16, tile batches of 1 and 4; the three identities -- (A) without regions it is mdtile_blend_lattice,
(B) at rest on an exact-fit canvas it is mdtile_blend on the plain plan with the same regions, (C) NaN / inf in the part of a pushed-in tile that
does not contribute never reaches the output; special values on region borders; every planes-per-thread form; misaligned pointers; every
refusal with its output left untouched; and both delegates with --mdtile-grid-jitter --mdtile-jitter-regions over three sampler steps.  No
tolerance appears in this file; half types follow tests/test_gpu_blend_matrix.py (inputs rounded to the dtype, the fp32 restatement evaluated on
those values, rounded once).

N = 2, C = 4 unless a case is there for the planes; the shapes are the smallest at which each branch can go wrong."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from hostsim import stub_host as sh

import grid_lattice_ref as gl
import lattice_region_ref as rr
import lattice_region_cases as cases
from wrap_common import DT, NAN, N, C, PLUGIN, SPECIALS, assert_bitwise as _assert_bitwise, on_device as _on_device

pytestmark = pytest.mark.gpu

GEOMETRIES = cases.GEOMETRIES
TILE_BS = [1, 4]


@functools.lru_cache(maxsize=None)
def _lat(geom, bs, sx, sy):
    g = gl.lattice(*GEOMETRIES[geom], bs, sx, sy)
    assert g is not None
    return g


def _lattice(E, geom, bs, sx, sy):
    """The library's lattice, checked against the restatement's."""
    lat = E.Lattice(*GEOMETRIES[geom], bs, sx, sy)
    g = _lat(geom, bs, sx, sy)
    assert lat.bboxes == list(g.boxes) and lat.tile_bs == g.tile_bs and lat.num_batches == len(g.batches), (lat.bboxes, g.boxes)
    return lat, g


def _method(E, method):
    return E.METHOD_MD if method == "md" else E.METHOD_MOD


@functools.lru_cache(maxsize=None)
def _tiles(tw, th, T, dt, n=N, c=C):
    """The model outputs of T tiles on the CPU in the dtype, tile-major: random normal."""
    torch.manual_seed(T * 7 + tw)
    return torch.randn(T * n, c, th, tw).to(DT[dt])


def _split(g, tiles, n=N):
    return [tiles[b[0] * n:(b[-1] + 1) * n].contiguous() for b in g.batches]


@functools.lru_cache(maxsize=None)
def _region_data(spec, dt, n=N, c=C):
    """[(x, y, w, h, mode, out, weight)] on the CPU: random normal outputs in the dtype, feather masks in [0, 1), the raw Gaussian of a BG region."""
    torch.manual_seed(len(spec) + 41)
    out = []
    for (x, y, w, h, mode) in spec:
        o = torch.randn(n, c, h, w).to(DT[dt])
        weight = torch.rand(h, w) if mode == "fg" else torch.from_numpy(gl.gaussian(w, h))
        out.append((x, y, w, h, mode, o, weight))
    return tuple(out)


def _ref_regions(regions, method):
    return [rr.Region(x, y, w, h, mode, out.float().numpy(), None if (mode == "bg" and method == "md") else weight.numpy())
            for (x, y, w, h, mode, out, weight) in regions]


def _dev_regions(E, regions, method, cuda, misaligned=False):
    return [E.RegionSpec(x, y, w, h, E.REGION_FG if mode == "fg" else E.REGION_BG, _on_device(out, cuda, misaligned),
                         None if (mode == "bg" and method == "md") else _on_device(weight, cuda, misaligned))
            for (x, y, w, h, mode, out, weight) in regions]


def _region_w(E, W, H, regions, method, cuda):
    """(device map or None, numpy map or None): the BG regions' weight sum through mdtile_weight_map_add_rect on zeros in list order, checked against
    the restatement; None when the list holds no BG region."""
    if not any(r[4] == "bg" for r in regions):
        return None, None
    m = torch.zeros(H, W, device=cuda)
    for (x, y, w, h, mode, _, weight) in regions:
        if mode == "bg":
            E.weight_map_add_rect(m, x, y, w, h, None if method == "md" else weight.to(cuda), 1.0)
    want = rr.region_w_map(W, H, method, _ref_regions(regions, method))
    _assert_bitwise(m, torch.from_numpy(want), f"region_w {method}")
    return m, want


def _tile_w(E, g, method, cuda):
    return E.gaussian_weights(g.tw, g.th, cuda) if method == "mod" else None


def _run(E, cuda, lat, g, method, dt, tiles, regions, what, n=N, c=C, misaligned=False, zero_map=False):
    """One launch against the restatement."""
    dtype = DT[dt]
    tile_w = _tile_w(E, g, method, cuda)
    region_w, region_w_np = _region_w(E, g.W, g.H, regions, method, cuda)
    if region_w is None and zero_map:
        region_w, region_w_np = torch.zeros(g.H, g.W, device=cuda), np.zeros((g.H, g.W), np.float32)
    batch = [_on_device(t, cuda, misaligned) for t in _split(g, tiles, n)]
    out = torch.full((n, c, g.H, g.W), NAN, dtype=dtype, device=cuda)
    got = E.blend_lattice_regions(lat, _method(E, method), batch, n, c, regions=_dev_regions(E, regions, method, cuda, misaligned), region_w=region_w,
                                  tile_w=tile_w, out=out)
    assert got.dtype == dtype
    want = rr.blend(g, method, tiles.float().numpy(), n, _ref_regions(regions, method), region_w_np, None if tile_w is None else tile_w.cpu().numpy())
    _assert_bitwise(got, torch.from_numpy(want).to(dtype), what)
    return got


# ---- against the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", TILE_BS)
@pytest.mark.parametrize("geom", list(GEOMETRIES))
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_blend_lattice_regions_bitwise(plugin, cuda, geom, method, dt, bs):
    """The full region list (a BG region across lattice borders and the hidden part of the pushed-in edge tiles, an FG region over it, two
    overlapping FG and two overlapping BG regions, a region equal to the canvas, the 1 x 1 corner, a region ending at x = W) at every shift of
    the set: the sequential fp32 loop, grid tiles then regions in list order, rounded once."""
    E = plugin.engine
    Wc, Hc = GEOMETRIES[geom][:2]
    regions = _region_data(tuple(cases.full_spec(Wc, Hc)), dt)
    for (sx, sy) in cases.shifts(geom):
        lat, g = _lattice(E, geom, bs, sx, sy)
        _run(E, cuda, lat, g, method, dt, _tiles(g.tw, g.th, len(g.boxes), dt), regions, f"{geom} {method} {dt} bs {bs} ({sx}, {sy})")


@pytest.mark.parametrize("geom", ["odd", "deep"])
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_foreground_only_and_sixteen_regions(plugin, cuda, geom, method, dt):
    """FG regions only with a NULL d_region_w (the grid's sum alone is the weight sum), and MDTILE_MAX_REGIONS regions."""
    E = plugin.engine
    Wc, Hc = GEOMETRIES[geom][:2]
    fg = _region_data(tuple(cases.fg_only(cases.full_spec(Wc, Hc))), dt)
    many = _region_data(tuple(cases.sixteen_spec(Wc, Hc)), dt)
    assert len(fg) == 3 and len(many) == E.MAX_REGIONS == 16
    for (sx, sy) in cases.shifts(geom)[:3]:
        lat, g = _lattice(E, geom, 4, sx, sy)
        tiles = _tiles(g.tw, g.th, len(g.boxes), dt)
        _run(E, cuda, lat, g, method, dt, tiles, fg, f"{geom} {method} {dt} FG only, NULL map ({sx}, {sy})")
        _run(E, cuda, lat, g, method, dt, tiles, many, f"{geom} {method} {dt} 16 regions ({sx}, {sy})")


@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_misaligned_pointers(plugin, cuda, method, dt):
    """Every batch tensor, region output and region weight one element into its storage: no vector access of them is aligned."""
    E = plugin.engine
    geom = "zero_ov"
    Wc, Hc = GEOMETRIES[geom][:2]
    regions = _region_data(tuple(cases.full_spec(Wc, Hc)), dt)
    for (sx, sy) in [(16, 16), (4, 4), (5, 3)]:
        lat, g = _lattice(E, geom, 4, sx, sy)
        _run(E, cuda, lat, g, method, dt, _tiles(g.tw, g.th, len(g.boxes), dt), regions, f"misaligned {method} {dt} ({sx}, {sy})", misaligned=True)


@pytest.mark.parametrize("method", ["md", "mod"])
def test_plane_walk_wraps(plugin, cuda, method):
    """N C = 2 x 36 = 72 planes > kPlaneBlocks = 64 (one plane per thread on a canvas this small): the plane walk goes round."""
    E = plugin.engine
    n, c = 2, 36
    blocks = [int(b) for b in re.findall(r"constexpr int kPlaneBlocks = (\d+);", open(os.path.join(PLUGIN, "csrc", "lattice.hip")).read())]
    assert blocks == [64] and 64 < n * c < 128, "one definition of the number of plane blocks, which the planes of this case pass"
    lat, g = _lattice(E, "odd", 4, 2, 1)
    Wc, Hc = g.W, g.H
    spec = tuple(cases.full_spec(Wc, Hc)[:3] + cases.full_spec(Wc, Hc)[5:7])
    _run(E, cuda, lat, g, method, "f32", _tiles(g.tw, g.th, len(g.boxes), "f32", n, c), _region_data(spec, "f32", n, c), f"plane walk {method}", n, c)


@pytest.mark.parametrize("method", ["md", "mod"])
def test_planes_per_thread_forms(plugin, cuda, method):
    """The launcher's 2- and 4-planes-per-thread kernels (N C = 8): H ceil(W / 4) 8 / 2 = 131072 at 512 x 256, / 4 = 131072 at 1024 x 256, with one
    BG and one FG region, against the same call made one plane at a time (the one-plane kernel, which the restatement has checked)."""
    E = plugin.engine
    for (Wc, Hc) in ((512, 256), (1024, 256)):
        lat = E.Lattice(Wc, Hc, 128, 128, 8, 8, 7, 3)
        tile_w = E.gaussian_weights(128, 128, cuda) if method == "mod" else None
        torch.manual_seed(Wc)
        tiles = [torch.randn(len(b) * N, C, 128, 128, device=cuda) for b in lat.batches]
        boxes = [(Wc // 2 - 37, 50, 141, 99, E.REGION_BG), (Wc - 90, 120, 90, 136, E.REGION_FG)]      # across tile borders; the FG one ends at both far edges
        outs = [torch.randn(N, C, h, w, device=cuda) for (_, _, w, h, _) in boxes]
        weights = [E.gaussian_weights(boxes[0][2], boxes[0][3], cuda) if method == "mod" else None, torch.rand(boxes[1][3], boxes[1][2], device=cuda)]
        region_w = torch.zeros(Hc, Wc, device=cuda)
        E.weight_map_add_rect(region_w, *boxes[0][:4], weights[0], 1.0)
        specs = lambda sel: [E.RegionSpec(*b, sel(o), wt) for b, o, wt in zip(boxes, outs, weights)]
        got = E.blend_lattice_regions(lat, _method(E, method), tiles, N, C, regions=specs(lambda o: o), region_w=region_w, tile_w=tile_w)
        for n in range(N):
            for c in range(C):
                one = [t.view(-1, N, C, 128, 128)[:, n, c].reshape(-1, 1, 128, 128).contiguous() for t in tiles]
                want = E.blend_lattice_regions(lat, _method(E, method), one, 1, 1, regions=specs(lambda o: o[n:n + 1, c:c + 1].contiguous()),
                                               region_w=region_w, tile_w=tile_w)
                _assert_bitwise(got[n:n + 1, c:c + 1], want.cpu(), f"{Wc}x{Hc} {method} plane ({n}, {c})")


# ---- (A) without regions: mdtile_blend_lattice ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMETRIES))
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_a_without_regions_it_is_blend_lattice(plugin, cuda, geom, method, dt):
    """num_regions = 0 with a NULL map and with a map of zeros: mdtile_blend_lattice's bits."""
    E, dtype = plugin.engine, DT[dt]
    for (sx, sy) in cases.shifts(geom):
        lat, g = _lattice(E, geom, 4, sx, sy)
        tile_w = _tile_w(E, g, method, cuda)
        batch = [t.to(cuda) for t in _split(g, _tiles(g.tw, g.th, len(g.boxes), dt))]
        want = E.blend_lattice(lat, _method(E, method), batch, N, C, tile_w=tile_w).cpu()
        for region_w in (None, torch.zeros(g.H, g.W, device=cuda)):
            out = torch.full((N, C, g.H, g.W), NAN, dtype=dtype, device=cuda)
            got = E.blend_lattice_regions(lat, _method(E, method), batch, N, C, region_w=region_w, tile_w=tile_w, out=out)
            _assert_bitwise(got, want, f"{geom} {method} {dt} ({sx}, {sy}) {'NULL' if region_w is None else 'zero'} map")


# ---- (B) at rest on an exact-fit canvas: mdtile_blend on the plain plan ---------------------------------------------------------------
@pytest.mark.parametrize("geom", cases.REST, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_b_at_rest_it_is_the_plain_blend(plugin, cuda, geom, method, dt):
    """The plain plan's maps made the way the delegates make them -- weight_map_add_grid on zeros, weight_map_add_rect per BG region, reciprocal,
    rect_mul_canvas on each BG Gaussian -- and mdtile_blend with the same regions.  MultiDiffusion: the full list, overlapping BG regions
    included.  Mixture of Diffusers: no pixel under two BG regions."""
    E, dtype = plugin.engine, DT[dt]
    Wc, Hc, tw, th, ov, bs = geom
    plan = E.Plan(Wc, Hc, tw, th, ov, bs)
    stx, sty = gl.rest(Wc, Hc, tw, th, ov)
    lat = E.Lattice(Wc, Hc, tw, th, ov, bs, stx, sty)
    assert lat.bboxes == plan.bboxes and lat.num_batches == plan.num_batches and lat.tile_bs == plan.tile_bs
    spec = cases.full_spec(Wc, Hc) if method == "md" else cases.disjoint_bg_spec(Wc, Hc)
    regions = _region_data(tuple(spec), dt)
    tiles = _tiles(plan.tile_w, plan.tile_h, plan.num_tiles, dt)
    first = np.cumsum([0] + [len(b) for b in lat.batches])      # the library's batches list their boxes: tile-major rows by their lengths
    batch = [tiles[first[i] * N:first[i + 1] * N].contiguous().to(cuda) for i in range(lat.num_batches)]
    tile_w = E.gaussian_weights(plan.tile_w, plan.tile_h, cuda) if method == "mod" else None
    region_w, _ = _region_w(E, Wc, Hc, regions, method, cuda)
    got = E.blend_lattice_regions(lat, _method(E, method), batch, N, C, regions=_dev_regions(E, regions, method, cuda), region_w=region_w, tile_w=tile_w)
    # the plain path
    weights = torch.zeros(Hc, Wc, device=cuda)
    E.weight_map_add_grid(plan, tile_w, weights)
    plain = []
    for (x, y, w, h, mode, out, weight) in regions:
        if mode == "bg":
            E.weight_map_add_rect(weights, x, y, w, h, None if method == "md" else weight.to(cuda), 1.0)
    rescale = E.reciprocal(weights) if method == "mod" else None
    for (x, y, w, h, mode, out, weight) in regions:
        wt = weight.to(cuda) if (mode == "fg" or method == "mod") else None
        if mode == "bg" and method == "mod":
            wt = wt.clone().view(1, 1, h, w)
            E.rect_mul_canvas(wt, rescale, x, y, w, h)
        plain.append(E.RegionSpec(x, y, w, h, E.REGION_FG if mode == "fg" else E.REGION_BG, out.to(cuda), wt))
    kw = dict(weights=weights) if method == "md" else dict(tile_w=tile_w, rescale=rescale)
    want = E.blend(plan, _method(E, method), batch, N, C, regions=plain, **kw)
    assert want.dtype == dtype and torch.isfinite(want).all()
    _assert_bitwise(got, want.cpu(), f"{geom} {method} {dt} at rest")


# ---- (C) and special values ----------------------------------------------------------------------------------------------------------
def _parts(g, t):
    """Of tile t, in pushed-in coordinates: the rows [y0, y1) and columns [x0, x1) that contribute (its lattice box, clipped to the canvas)."""
    r, c = divmod(t, g.cols)
    y0, y1 = max(g.vs[r], 0) - g.ys[r], min(g.vs[r] + g.th, g.H) - g.ys[r]
    x0, x1 = max(g.us[c], 0) - g.xs[c], min(g.us[c] + g.tw, g.W) - g.xs[c]
    return y0, y1, x0, x1


@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("geom,shift", [("odd", (2, 1)), ("deep", (3, 3)), ("zero_ov", (1, 1))])
def test_c_hidden_parts_never_reach_the_output(plugin, cuda, geom, shift, method):
    """NaN and +-inf painted over the part of every pushed-in tile that does NOT contribute, under the full region list: the result is the
    restatement's (which never indexes those parts), it is finite everywhere, and a second run with those parts zeroed gives the same bits."""
    E = plugin.engine
    lat, g = _lattice(E, geom, 4, *shift)
    regions = _region_data(tuple(cases.full_spec(g.W, g.H)), "f32")
    tiles = _tiles(g.tw, g.th, len(g.boxes), "f32").clone()
    clean = tiles.clone()
    hidden = 0
    for t in range(len(g.boxes)):
        y0, y1, x0, x1 = _parts(g, t)
        outside = torch.ones(g.th, g.tw, dtype=torch.bool)
        outside[y0:y1, x0:x1] = False
        hidden += int(outside.sum())
        tiles[t * N:(t + 1) * N][:, :, outside] = torch.tensor([NAN, float("inf"), float("-inf")])[torch.arange(int(outside.sum())) % 3]
        clean[t * N:(t + 1) * N][:, :, outside] = 0.0
    assert hidden > 0 and torch.isnan(tiles).any()
    got = _run(E, cuda, lat, g, method, "f32", tiles, regions, f"{geom} {method} hidden parts painted")
    assert torch.isfinite(got).all(), "a value outside a tile's lattice box reached the output"
    again = _run(E, cuda, lat, g, method, "f32", clean, regions, f"{geom} {method} hidden parts zeroed")
    _assert_bitwise(again, got.cpu(), f"{geom} {method}: the non-contributing parts change the output")


@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("geom,shift", [("odd", (2, 1)), ("zero_ov", (5, 3))])
def test_special_values_on_region_borders(plugin, cuda, geom, shift, method):
    """+-0, +-inf, NaN, denormals, fp16 max and values near fp32 max in the first and last rows and columns of every region's output."""
    E = plugin.engine
    lat, g = _lattice(E, geom, 4, *shift)
    vals = torch.tensor(SPECIALS)
    regions = []
    for k, (x, y, w, h, mode, out, weight) in enumerate(_region_data(tuple(cases.full_spec(g.W, g.H)), "f32")):
        out = out.clone()
        for i, yy in enumerate({0, h - 1}):
            out[:, :, yy, :] = vals[(torch.arange(w) + i + k) % len(vals)]
        for i, xx in enumerate({0, w - 1}):
            out[:, :, :, xx] = vals[(torch.arange(h) * 3 + i + k) % len(vals)]
        regions.append((x, y, w, h, mode, out, weight))
    assert any(torch.isnan(r[5]).any() and (r[5] == 65504.0).any() and ((r[5] != 0) & (r[5].abs() < 1e-38)).any() for r in regions)
    _run(E, cuda, lat, g, method, "f32", _tiles(g.tw, g.th, len(g.boxes), "f32"), tuple(regions), f"{geom} {method} specials on region borders")


# ---- refused calls -----------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(plugin, cuda):
    """Every refusal is MDTILE_E_ARG with a text that names the reason, and leaves the NaN-painted output as it is."""
    E = plugin.engine
    lat, g = _lattice(E, "odd", 4, 2, 1)
    W, H = g.W, g.H
    ones = [torch.ones(len(b) * N, C, g.th, g.tw, device=cuda) for b in g.batches]
    out = torch.full((N, C, H, W), NAN, device=cuda)
    zeros, some_map = torch.zeros(H, W, device=cuda), torch.ones(H, W, device=cuda)
    tile_w = E.gaussian_weights(g.tw, g.th, cuda)

    def region(x, y, w, h, mode=E.REGION_BG, weight=True):
        return E.RegionSpec(x, y, w, h, mode, torch.ones(N, C, h, w, device=cuda), torch.ones(h, w, device=cuda) if weight else None)

    def refused(text, method=E.METHOD_MD, batch=None, **kw):
        args = dict(regions=[], region_w=zeros, out=out)
        args.update(kw)
        with pytest.raises(E.MdtileError, match=r"mdtile_blend_lattice_regions failed \(rc=-1\).*" + text):
            E.blend_lattice_regions(lat, method, ones if batch is None else batch, N, C, **args)

    def raw(text, block=True, **kw):
        _, a, ptrs = E._blend_operands(lat, E.METHOD_MD, ones, N, C, torch.float32, torch.float32, cuda, out, None, None, None, **kw)
        lr_ = E._LatticeRegions(None, 0, None)
        rc = E.lib().mdtile_blend_lattice_regions(lat.ref, E.ctypes.byref(a), ptrs, len(ones), E.ctypes.byref(lr_) if block else None, E._stream())
        with pytest.raises(E.MdtileError, match=text):
            E._check(rc, "mdtile_blend_lattice_regions")

    # what mdtile_blend_lattice refuses
    refused("batches given", batch=ones[:-1])
    refused("d_weights and d_rescale must be NULL", weights=some_map)
    refused("d_weights and d_rescale must be NULL", method=E.METHOD_MOD, tile_w=tile_w, rescale=some_map)
    refused("Mixture of Diffusers needs d_tile_w", method=E.METHOD_MOD)
    raw(r"no MDTILE_BLEND_\* flags", flags=E.BLEND_PARTIAL)
    raw(r"no MDTILE_BLEND_\* flags", flags=E.BLEND_TILE_RANGE, tile_range=(0, 2))
    raw("no row band", row_range=(0, 8))
    # the regions block
    raw("null regions block", block=False)
    refused("17 regions", regions=[region(1, 1, 2, 2)] * 17)
    for (x, y, w, h) in [(W - 3, 1, 4, 4), (1, H - 3, 4, 4), (0, 0, W + 1, 2), (0, 0, 2, H + 1)]:
        refused(r"region 1 \(.*\) does not lie on the %dx%d canvas" % (W, H), regions=[region(1, 1, 4, 4), region(x, y, w, h)])
    for (x, y, w, h) in [(-1, 1, 4, 4), (1, -1, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0)]:      # an empty rectangle comes with empty tensors
        refused(r"region 0 \(.*\) does not lie on", regions=[region(x, y, w, h)])
    refused("region 0 bad mode 7", regions=[region(1, 1, 4, 4, mode=7)])
    refused(r"region 0 \(foreground\) needs its feather mask", regions=[region(1, 1, 4, 4, E.REGION_FG, weight=False)])
    refused(r"region 0 \(background, Mixture of Diffusers\) needs its raw Gaussian", method=E.METHOD_MOD, tile_w=tile_w,
            regions=[region(1, 1, 4, 4, weight=False)])
    refused("null d_region_w with 1 background region", regions=[region(1, 1, 4, 4)], region_w=None)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused blend wrote to its output"
    # and the call of before keeps its behaviour: no regions parameter, the same refusals
    with pytest.raises(TypeError):
        E.blend_lattice(lat, E.METHOD_MD, ones, N, C, regions=[region(1, 1, 4, 4)], out=out)
    with pytest.raises(E.MdtileError, match=r"mdtile_blend_lattice failed \(rc=-1\).*d_weights and d_rescale must be NULL"):
        E.blend_lattice(lat, E.METHOD_MD, ones, N, C, weights=some_map, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ---- the delegates with the options set ----------------------------------------------------------------------------------------------
@pytest.fixture
def options():
    """The stub host with --mdtile-grid-jitter --mdtile-jitter-regions; both gone and the step counter back afterwards."""
    _, shared = sh.host()
    step = shared.state.sampling_step
    shared.cmd_opts.mdtile_grid_jitter = shared.cmd_opts.mdtile_jitter_regions = True
    try:
        yield shared
    finally:
        for name in ("mdtile_grid_jitter", "mdtile_jitter_regions"):
            if hasattr(shared.cmd_opts, name):
                delattr(shared.cmd_opts, name)
        shared.state.sampling_step = step


@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_keeps_the_moving_grid_with_regions(plugin, cuda, options, method):
    """MultiDiffusion / MixtureOfDiffusers with both switches, one BG and one FG region, over three sampler steps with pinned, pairwise different
    lattices: the model ran once per tile batch of the step's lattice and once per region, on the pushed-in boxes and on the regions where the
    user put them, with the image conditioning cut alike; the result is the restatement's fed the same outputs.  The stand-in model
    multiplies its input by a power of two that depends on which call it is."""
    shared, seed = options, 1234567
    Wc, Hc, tw, th, ov = GEOMETRIES["odd"]
    U = plugin.utils
    cls = plugin.multidiffusion.MultiDiffusion if method == "md" else plugin.mixtureofdiffusers.MixtureOfDiffusers
    p = sh.make_processing(Wc * 8, Hc * 8)
    p.all_seeds = [seed]
    d = cls(p, sh.kdiff_sampler())
    d.init_grid_bbox(tw, th, ov, 4)
    settings = {0: U.BBoxSettings(True, 0.2, 0.1, 0.6, 0.5, "", "", "Background", 0.2, -1),
                1: U.BBoxSettings(True, 0.5, 0.3, 0.5, 0.7, "", "", "Foreground", 0.3, -1)}
    d.init_custom_bbox(settings, True, False)
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    d.update_pbar = lambda: None
    assert d.grid_jitter and d.jitter_regions and d.total_bboxes == 4 + 2      # up to 4 x 4 tiles in batches of 4, and the two regions
    boxes = [(b.x, b.y, b.w, b.h) for b in d.custom_bboxes]
    assert boxes == [(7, 2, 23, 11), (18, 6, 19, 16)]                          # the FG region ends at x = W and y = H
    tile_w = d.get_tile_weights().cpu().numpy() if method == "mod" else None
    feather = d.custom_bboxes[1].feather_mask.cpu().numpy().reshape(16, 19)
    bg_w = d.raw_custom_weights[0].cpu().numpy().reshape(11, 23) if method == "mod" else None
    if method == "mod":
        _assert_bitwise(d.raw_custom_weights[0].reshape(11, 23), torch.from_numpy(gl.gaussian(23, 11)), "the raw Gaussian of the BG region")
        assert not torch.equal(d.custom_weights[0], d.raw_custom_weights[0]), "the fixed grid's copy is premultiplied"
    torch.manual_seed(9)
    x = torch.randn(N, C, Hc, Wc)
    icond = torch.randn(N, 5, Hc, Wc)
    cond = {"c_crossattn": [torch.zeros(N, 77, 768, device=cuda)], "c_concat": [icond.to(cuda)]}
    cut = lambda src, box: np.ascontiguousarray(src.numpy()[:, :, box[1]:box[1] + box[3], box[0]:box[0] + box[2]])
    scale = lambda k: (-2.0) ** ((k % 5) - 2)
    pinned = [(10, 6), (4, 8), (6, 7)]                # lattice_shift(1234567, step, axis, 12 | 8), steps 0 .. 2
    counts = []
    for step, (sx, sy) in enumerate(pinned):
        shared.state.sampling_step = step
        assert gl.step_shift(Wc, Hc, tw, th, ov, seed, step) == (sx, sy)
        g = gl.lattice(Wc, Hc, tw, th, ov, 4, sx, sy)
        counts.append(len(g.boxes))
        calls, seen = [], []

        def model(t):
            calls.append(t.clone())
            return t * scale(len(calls) - 1)

        if method == "md":
            def repeat(xt, bboxes):
                seen.append(d.get_icond(d.repeat_cond_dict(cond, bboxes)))
                return model(xt)

            def custom(xt, bbox_id, bbox):
                seen.append(d.slice_icond(d.get_icond(cond), bbox))
                return model(xt)
            out = d.sample_one_step(x.to(cuda), None, repeat, custom)
        else:
            def tile_model(x_, t_, c_):
                seen.append(d.get_icond(c_))
                return model(x_)

            def custom_apply(xt, t_in, c_in, bbox_id, bbox):
                seen.append(d.slice_icond(d.get_icond(c_in), bbox))
                return model(xt)
            shared.sd_model.apply_model_original_md = tile_model
            d.custom_apply_model = custom_apply
            out = d.apply_model_hijack(x.to(cuda), torch.zeros(N, device=cuda), cond)
        nb = len(g.batches)
        assert len(calls) == nb + 2 == len(seen), "one call per tile batch of the step's lattice and one per region"
        tiles = [gl.gather(g, x.numpy(), b) for b in range(nb)]
        for b in range(nb):
            _assert_bitwise(calls[b], torch.from_numpy(tiles[b]), f"{method} step {step}: the model's input of batch {b}")
            want = np.concatenate([cut(icond, g.boxes[t]) for t in g.batches[b]], axis=0)
            _assert_bitwise(seen[b], torch.from_numpy(want), f"{method} step {step}: image conditioning of batch {b}")
        for i, box in enumerate(boxes):
            _assert_bitwise(calls[nb + i], torch.from_numpy(cut(x, box)), f"{method} step {step}: the tile of region {i}")
            _assert_bitwise(seen[nb + i], torch.from_numpy(cut(icond, box)), f"{method} step {step}: image conditioning of region {i}")
        ref_tiles = np.concatenate([t * np.float32(scale(b)) for b, t in enumerate(tiles)], axis=0)
        outs = [cut(x, box) * np.float32(scale(nb + i)) for i, box in enumerate(boxes)]
        regions = [rr.Region(*boxes[0], "bg", outs[0], bg_w), rr.Region(*boxes[1], "fg", outs[1], feather)]
        region_w = rr.region_w_map(Wc, Hc, method, regions)
        _assert_bitwise(d.region_w[0, 0], torch.from_numpy(region_w), f"{method}: the delegate's region_w")
        want = rr.blend(g, method, ref_tiles, N, regions, region_w, tile_w)
        _assert_bitwise(out, torch.from_numpy(want), f"delegate {method} step {step} lattice ({sx}, {sy})")
    assert len(set(pinned)) == 3 and counts == [9, 12, 12]
    assert p.extra_generation_params["Tiled Diffusion jitter regions"] is True and p.extra_generation_params["Tiled Diffusion grid jitter"] is True
