"""The jittered tile grid on a plain canvas (mdtile_lattice_weight_map / mdtile_gather_all_lattice / mdtile_blend_lattice, csrc/lattice.hip,
DESIGN.md 3.18) on the GPU, BITWISE: against the numpy restatement tests/grid_lattice_ref.py and, at rest on a canvas the stride divides, against the
existing path on the plain plan.  Gather, weight map and blend of both methods in fp32, fp16 and bf16, special values, the refused calls, and the
delegates with --mdtile-grid-jitter over three sampler steps.  No tolerance appears in this file; half types follow
tests/test_gpu_blend_matrix.py (inputs and tile outputs rounded to the dtype, the fp32 restatement evaluated on those values, rounded once).

N = 2, C = 4 unless a case says otherwise; a test is one lattice per shift of its geometry and one launch per lattice."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from hostsim import stub_host as sh

import grid_lattice_ref as lr
from wrap_common import (DT, NAN, N, C, PLUGIN, SPECIALS, assert_bitwise as _assert_bitwise, tile_fn as _tile_fn, on_device as _on_device,
                         make_delegate)

pytestmark = pytest.mark.gpu

# id -> (W, H, requested tile_w, tile_h, overlap)
GEOMETRIES = {
    "odd": (37, 22, 16, 12, 4),             # odd extents, non-square tile; strides 12 and 8
    "zero_ov": (40, 24, 16, 16, 0),         # at most 2 covering tiles per axis
    "deep": (33, 20, 16, 16, 12),           # stride 4: 4 covering tiles per axis away from the edges, 16 on a pixel
    "one_col": (16, 40, 16, 16, 4),         # the tile spans x: only y moves
    "aligned64": (64, 64, 32, 32, 0),       # every origin of an aligned shift a multiple of 4
}
# aligned64 also runs with every batch tensor one element into its storage: no vector access of a batch is aligned
ALL_GEOMETRIES = list(GEOMETRIES) + ["aligned64_misaligned"]
TILE_BS = [1, 4]


def _base(geom):
    return geom[:-len("_misaligned")] if geom.endswith("_misaligned") else geom


def _shifts(geom):
    """(1, 1), at rest, (2, 1), (stride_x - 1, 3), (4, 4), (stride_x, 1), each clipped to [1, stride]; an axis that does not move keeps 1."""
    Wc, Hc, tw, th, ov = GEOMETRIES[_base(geom)]
    stx, sty = (max(1, s) for s in lr.rest(Wc, Hc, tw, th, ov))
    raw = [(1, 1), (stx, sty), (2, 1), (stx - 1, 3), (4, 4), (stx, 1)]
    out = []
    for sx, sy in raw:
        s = (min(max(sx, 1), stx), min(max(sy, 1), sty))
        if s not in out:
            out.append(s)
    return out


@functools.lru_cache(maxsize=None)
def _lat(geom, bs, sx, sy):
    g = lr.lattice(*GEOMETRIES[_base(geom)], bs, sx, sy)
    assert g is not None
    return g


def _lattice(E, geom, bs, sx, sy):
    """The library's lattice, checked against the restatement's."""
    lat = E.Lattice(*GEOMETRIES[_base(geom)], bs, sx, sy)
    g = _lat(geom, bs, sx, sy)
    assert lat.bboxes == list(g.boxes) and lat.tile_bs == g.tile_bs and lat.num_batches == len(g.batches), (lat.bboxes, g.boxes)
    return lat, g


@functools.lru_cache(maxsize=None)
def _canvas(geom, dt, n=N, c=C):
    Wc, Hc = GEOMETRIES[geom][:2]
    torch.manual_seed(len(geom) + 31)
    return torch.randn(n, c, Hc, Wc).to(DT[dt])


@functools.lru_cache(maxsize=None)
def _tiles(geom, dt, bs, sx, sy, n=N, c=C):
    """The model outputs of every batch of one lattice on the CPU, in the dtype."""
    g = _lat(geom, bs, sx, sy)
    x = _canvas(geom, dt, n, c)
    return tuple(_tile_fn(torch.from_numpy(lr.gather(g, x.float().numpy(), b)).to(DT[dt])) for b in range(len(g.batches)))


@functools.lru_cache(maxsize=None)
def _tile_w(cuda_index, tw, th):
    import mdtile
    return mdtile.gaussian_weights(tw, th, torch.device("cuda", cuda_index))


def _method(E, method):
    return E.METHOD_MD if method == "md" else E.METHOD_MOD


def _blend_ref(g, method, tiles, tile_w, dtype, n=N):
    t = torch.cat(list(tiles), dim=0).float().numpy()
    ref = lr.blend(g, method, t, n, tile_w.cpu().numpy() if method == "mod" else None)
    return torch.from_numpy(ref).to(dtype)


# ---- against the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bs", TILE_BS)
@pytest.mark.parametrize("geom", ALL_GEOMETRIES)
@pytest.mark.parametrize("dt", list(DT))
def test_gather_all_lattice_bitwise(plugin, cuda, geom, dt, bs):
    """x_tile[i N + n, c, ty, tx] = x_in[n, c, y'_r + ty, x'_c + tx]: the pushed-in boxes, tile-major compact batches, the last one short."""
    E = plugin.engine
    x = _canvas(_base(geom), dt)
    xd = x.to(cuda)
    for (sx, sy) in _shifts(geom):
        lat, g = _lattice(E, geom, bs, sx, sy)
        out = [_on_device(torch.full((len(b) * N, C, g.th, g.tw), NAN, dtype=x.dtype), cuda, geom.endswith("_misaligned")) for b in g.batches]
        got = E.gather_all_lattice(lat, xd, out=out)
        for b in range(len(g.batches)):
            want = torch.from_numpy(lr.gather(g, x.float().numpy(), b)).to(x.dtype)
            _assert_bitwise(got[b], want, f"{geom} {dt} bs {bs} gather_all_lattice ({sx}, {sy}) batch {b}")


@pytest.mark.parametrize("geom", list(GEOMETRIES))
@pytest.mark.parametrize("method", ["md", "mod"])
def test_lattice_weight_map_bitwise(plugin, cuda, geom, method):
    """The weight sum of every shift: the count of covering tiles, or the Gaussian read in lattice coordinates and summed in tile order.  The map
    is written, not added: the output starts as NaN."""
    E = plugin.engine
    for (sx, sy) in _shifts(geom):
        lat, g = _lattice(E, geom, 4, sx, sy)
        tile_w = _tile_w(cuda.index or 0, g.tw, g.th) if method == "mod" else None
        out = torch.full((g.H, g.W), NAN, device=cuda)
        got = E.lattice_weight_map(lat, tile_w, out=out)
        want = lr.weight_map(g, tile_w.cpu().numpy() if method == "mod" else None)
        _assert_bitwise(got, torch.from_numpy(want), f"{geom} {method} lattice_weight_map ({sx}, {sy})")
        if method == "md":
            most = {"zero_ov": 4, "deep": 16, "one_col": 2}.get(geom)
            assert want.min() >= 1 and (most is None or want.max() <= most), (geom, want.min(), want.max())


@pytest.mark.parametrize("bs", TILE_BS)
@pytest.mark.parametrize("geom", ALL_GEOMETRIES)
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_blend_lattice_bitwise(plugin, cuda, geom, method, dt, bs):
    """mdtile_blend_lattice == the sequential fp32 `+=` loop in tile order over the lattice boxes, values read at the pushed-in coordinates, with
    the step's own weight sum, then the epilogue, rounded once."""
    E, dtype = plugin.engine, DT[dt]
    for (sx, sy) in _shifts(geom):
        lat, g = _lattice(E, geom, bs, sx, sy)
        tile_w = _tile_w(cuda.index or 0, g.tw, g.th) if method == "mod" else None
        tiles = _tiles(_base(geom), dt, bs, sx, sy)
        batch = [_on_device(t, cuda, geom.endswith("_misaligned")) for t in tiles]
        out = torch.full((N, C, g.H, g.W), NAN, dtype=dtype, device=cuda)
        got = E.blend_lattice(lat, _method(E, method), batch, N, C, tile_w=tile_w, out=out)
        assert got.dtype == dtype
        _assert_bitwise(got, _blend_ref(g, method, tiles, tile_w, dtype), f"{geom} {method} {dt} bs {bs} blend_lattice ({sx}, {sy})")


def _plane_blocks():
    """kPlaneBlocks of csrc/lattice.hip: the most blocks along grid.y; the kernels walk the planes from blockIdx.y in steps of gridDim.y."""
    src = open(os.path.join(PLUGIN, "csrc", "lattice.hip")).read()
    return int(re.search(r"constexpr int kPlaneBlocks = (\d+);", src).group(1))


@pytest.mark.parametrize("method", ["md", "mod"])
def test_plane_walk_wraps(plugin, cuda, method):
    """N C = 2 x 36 = 72 planes > kPlaneBlocks = 64 (one plane per thread on a canvas this small): the plane walk of the gather and of the blend goes
    round, blocks 0 .. 7 own two planes each."""
    E = plugin.engine
    n, c = 2, 36
    assert _plane_blocks() == 64 < n * c < 2 * _plane_blocks()
    geom, bs, (sx, sy) = "odd", 4, (2, 1)
    lat, g = _lattice(E, geom, bs, sx, sy)
    x = _canvas(geom, "f32", n, c)
    got = E.gather_all_lattice(lat, x.to(cuda))
    for b in range(len(g.batches)):
        _assert_bitwise(got[b], torch.from_numpy(lr.gather(g, x.numpy(), b)), f"plane walk gather batch {b}")
    tile_w = _tile_w(cuda.index or 0, g.tw, g.th) if method == "mod" else None
    tiles = _tiles(geom, "f32", bs, sx, sy, n, c)
    out = torch.full((n, c, g.H, g.W), NAN, device=cuda)
    E.blend_lattice(lat, _method(E, method), [t.to(cuda) for t in tiles], n, c, tile_w=tile_w, out=out)
    _assert_bitwise(out, _blend_ref(g, method, tiles, tile_w, torch.float32, n), f"plane walk blend {method}")


@pytest.mark.parametrize("method", ["md", "mod"])
def test_planes_per_thread_forms(plugin, cuda, method):
    """The launcher's 2- and 4-planes-per-thread kernels (N C = 8): H ceil(W / 4) 8 / 2 = 131072 at 512 x 256, / 4 = 131072 at 1024 x 256, against
    the one-plane kernel on the same tiles plane by plane (the restatement has checked that one)."""
    E = plugin.engine
    for (Wc, Hc) in ((512, 256), (1024, 256)):
        lat = E.Lattice(Wc, Hc, 128, 128, 8, 8, 7, 3)
        tile_w = _tile_w(cuda.index or 0, 128, 128) if method == "mod" else None
        torch.manual_seed(Wc)
        x = torch.randn(N, C, Hc, Wc, device=cuda)
        tiles = [_tile_fn(t) for t in E.gather_all_lattice(lat, x)]
        got = E.blend_lattice(lat, _method(E, method), tiles, N, C, tile_w=tile_w)
        for n in range(N):
            for c in range(C):
                one = [t.view(-1, N, C, 128, 128)[:, n, c].reshape(-1, 1, 128, 128).contiguous() for t in tiles]
                want = E.blend_lattice(lat, _method(E, method), one, 1, 1, tile_w=tile_w)
                _assert_bitwise(got[n:n + 1, c:c + 1], want.cpu(), f"{Wc}x{Hc} {method} plane ({n}, {c})")


# ---- at rest against the existing path ---------------------------------------------------------------------------------------------
REST = [(40, 28, 16, 16, 4, 4), (64, 64, 32, 32, 0, 3), (40, 28, 16, 12, 8, 4)]      # (W - tw) % stride == 0 on both axes


@pytest.mark.parametrize("geom", REST, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("dt", list(DT))
def test_at_rest_equals_the_plain_plan(plugin, cuda, geom, dt):
    """The lattice at (stride_x, stride_y) is the plain plan: gather == mdtile_gather_all, weight map == mdtile_weight_map_add_grid on zeros, blend
    == mdtile_blend given the same tile outputs and the plan's own maps, both methods."""
    E, dtype = plugin.engine, DT[dt]
    Wc, Hc, tw, th, ov, bs = geom
    plan = E.Plan(Wc, Hc, tw, th, ov, bs)
    stx, sty = lr.rest(Wc, Hc, tw, th, ov)
    assert (Wc - plan.tile_w) % stx == 0 and (Hc - plan.tile_h) % sty == 0
    lat = E.Lattice(Wc, Hc, tw, th, ov, bs, stx, sty)
    assert lat.bboxes == plan.bboxes and lat.num_batches == plan.num_batches and lat.tile_bs == plan.tile_bs
    torch.manual_seed(Wc + Hc)
    x = torch.randn(N, C, Hc, Wc).to(dtype).to(cuda)
    tiles = E.gather_all_lattice(lat, x)
    for b, t in enumerate(E.gather_all(plan, x)):
        _assert_bitwise(tiles[b], t.cpu(), f"{geom} {dt} gather batch {b}")
    outs = [_tile_fn(t) for t in tiles]
    tile_w = E.gaussian_weights(plan.tile_w, plan.tile_h, cuda)
    for method, tw_ in (("md", None), ("mod", tile_w)):
        wsum = torch.zeros(Hc, Wc, device=cuda)
        E.weight_map_add_grid(plan, tw_, wsum)
        _assert_bitwise(E.lattice_weight_map(lat, tw_, device=cuda), wsum.cpu(), f"{geom} {method} weight map")
        kw = dict(weights=wsum) if method == "md" else dict(tile_w=tile_w, rescale=E.reciprocal(wsum))
        want = E.blend(plan, _method(E, method), outs, N, C, **kw)
        got = E.blend_lattice(lat, _method(E, method), outs, N, C, tile_w=tw_)
        _assert_bitwise(got, want.cpu(), f"{geom} {method} {dt} blend")


# ---- special values ----------------------------------------------------------------------------------------------------------------
def _parts(g, t):
    """Of tile t, in pushed-in coordinates: the rows [y0, y1) and columns [x0, x1) that contribute (its lattice box, clipped to the canvas)."""
    r, c = divmod(t, g.cols)
    y0, y1 = max(g.vs[r], 0) - g.ys[r], min(g.vs[r] + g.th, g.H) - g.ys[r]
    x0, x1 = max(g.us[c], 0) - g.xs[c], min(g.us[c] + g.tw, g.W) - g.xs[c]
    return y0, y1, x0, x1


@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("geom,shift", [("odd", (2, 1)), ("deep", (3, 3)), ("zero_ov", (1, 1))])
def test_special_values_bitwise(plugin, cuda, geom, shift, method):
    """+-0, +-inf, NaN, denormals and fp16 max on both sides of every lattice border of every tile (its first and last contributing rows and
    columns); and the part of every pushed-in tile that does NOT contribute painted with NaN and inf, which must not reach the output: a
    second run with those parts zeroed gives the same bits, and pixels whose contributing values are all finite come out finite."""
    E = plugin.engine
    lat, g = _lattice(E, geom, 4, *shift)
    tile_w = _tile_w(cuda.index or 0, g.tw, g.th) if method == "mod" else None
    torch.manual_seed(7)
    T = len(g.boxes)
    tiles = torch.randn(T * N, C, g.th, g.tw)
    vals = torch.tensor(SPECIALS)
    finite = np.ones((g.H, g.W), bool)
    hidden = 0
    for t in range(T):
        y0, y1, x0, x1 = _parts(g, t)
        v = tiles[t * N:(t + 1) * N]
        special = torch.zeros(g.th, g.tw, dtype=torch.bool)
        for i, yy in enumerate({y0, y1 - 1}):
            v[:, :, yy, x0:x1] = vals[(torch.arange(x1 - x0) + i + t) % len(vals)]
            special[yy, x0:x1] = True
        for i, xx in enumerate({x0, x0 + 1, x1 - 1}):
            v[:, :, y0:y1, xx] = vals[(torch.arange(y1 - y0) * 3 + i + t) % len(vals)]
            special[y0:y1, xx] = True
        r, c = divmod(t, g.cols)
        finite[g.ys[r] + y0:g.ys[r] + y1, g.xs[c] + x0:g.xs[c] + x1] &= ~special[y0:y1, x0:x1].numpy()
        outside = torch.ones(g.th, g.tw, dtype=torch.bool)
        outside[y0:y1, x0:x1] = False
        hidden += int(outside.sum())
        v[:, :, outside] = torch.tensor([NAN, float("inf"), float("-inf")])[torch.arange(int(outside.sum())) % 3]
    assert hidden > 0 and finite.any() and torch.isnan(tiles).any() and (tiles == 65504.0).any() and ((tiles != 0) & (tiles.abs() < 1e-38)).any()
    split = lambda tt: [tt[g.batches[b][0] * N:(g.batches[b][-1] + 1) * N].contiguous() for b in range(len(g.batches))]
    got = E.blend_lattice(lat, _method(E, method), [t.to(cuda) for t in split(tiles)], N, C, tile_w=tile_w)
    _assert_bitwise(got, _blend_ref(g, method, split(tiles), tile_w, torch.float32), f"{geom} {method} specials")
    assert torch.isfinite(got.cpu()[:, :, torch.from_numpy(finite)]).all(), "a value outside a tile's lattice box reached the output"
    clean = tiles.clone()
    for t in range(T):
        y0, y1, x0, x1 = _parts(g, t)
        outside = torch.ones(g.th, g.tw, dtype=torch.bool)
        outside[y0:y1, x0:x1] = False
        clean[t * N:(t + 1) * N][:, :, outside] = 0.0
    again = E.blend_lattice(lat, _method(E, method), [t.to(cuda) for t in split(clean)], N, C, tile_w=tile_w)
    _assert_bitwise(again, got.cpu(), f"{geom} {method}: the non-contributing parts change the output")


# ---- refused calls -----------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(plugin, cuda):
    """Every refusal is MDTILE_E_ARG with a text that names the reason, and leaves NaN-painted outputs as they are."""
    E, L = plugin.engine, plugin.engine.lib()
    assert E.E_ARG == -1
    lat, g = _lattice(E, "odd", 4, 2, 1)
    x = torch.zeros(N, C, g.H, g.W, device=cuda)
    tiles = [torch.full((len(b) * N, C, g.th, g.tw), NAN, device=cuda) for b in g.batches]
    ones = [torch.ones_like(t) for t in tiles]
    out = torch.full((N, C, g.H, g.W), NAN, device=cuda)
    wmap = torch.full((g.H, g.W), NAN, device=cuda)
    some_map = torch.ones(g.H, g.W, device=cuda)
    tile_w = _tile_w(cuda.index or 0, g.tw, g.th)

    with pytest.raises(E.MdtileError, match=r"mdtile_lattice_make failed \(rc=-1\).*sx = 13 outside \[1, 12\]"):
        E.Lattice(*GEOMETRIES["odd"], 4, 13, 1)
    with pytest.raises(E.MdtileError, match=r"mdtile_lattice_make failed \(rc=-1\).*sy = 0 outside \[1, 8\]"):
        E.Lattice(*GEOMETRIES["odd"], 4, 1, 0)
    with pytest.raises(E.MdtileError, match=r"mdtile_gather_all_lattice failed \(rc=-1\).*batches given"):
        E.gather_all_lattice(lat, x, out=tiles[:-1])
    with pytest.raises(E.MdtileError, match=r"mdtile_blend_lattice failed \(rc=-1\).*batches given"):
        E.blend_lattice(lat, E.METHOD_MD, ones[:-1], N, C, out=out)
    with pytest.raises(E.MdtileError, match="d_weights and d_rescale must be NULL"):
        E.blend_lattice(lat, E.METHOD_MD, ones, N, C, weights=some_map, out=out)
    with pytest.raises(E.MdtileError, match="d_weights and d_rescale must be NULL"):
        E.blend_lattice(lat, E.METHOD_MOD, ones, N, C, tile_w=tile_w, rescale=some_map, out=out)
    with pytest.raises(E.MdtileError, match="Mixture of Diffusers needs d_tile_w"):
        E.blend_lattice(lat, E.METHOD_MOD, ones, N, C, out=out)

    def raw_blend(text, lat_c=None, **kw):
        _, a, ptrs = E._blend_operands(lat, E.METHOD_MD, ones, N, C, torch.float32, torch.float32, cuda, out, None, None, None, **kw)
        ref = ctypes.byref(lat_c) if lat_c is not None else lat.ref
        assert L.mdtile_blend_lattice(ref, ctypes.byref(a), ptrs, len(ones), E._stream()) == E.E_ARG
        assert re.search(text, L.mdtile_last_error().decode()), L.mdtile_last_error()

    raw_blend(r"no MDTILE_BLEND_\* flags", flags=E.BLEND_PARTIAL)
    raw_blend(r"no MDTILE_BLEND_\* flags", flags=E.BLEND_TILE_RANGE, tile_range=(0, 2))
    raw_blend("no row band", row_range=(0, 8))
    # a struct whose shift was changed behind mdtile_lattice_make's back, or whose counts no longer fit it
    for field, value, text in (("sx", 0, r"sx = 0 outside \[1, 12\]"), ("sy", 9, r"sy = 9 outside \[1, 8\]"), ("sx", 12, "tiles along x"), ("rows", 9, "tiles along y")):
        c = E._Lattice(*[getattr(lat._c, n) for n, _ in E._Lattice._fields_])
        setattr(c, field, value)
        raw_blend(text, lat_c=c)
        ptrs = (ctypes.c_void_p * len(tiles))(*[t.data_ptr() for t in tiles])
        assert L.mdtile_gather_all_lattice(ctypes.byref(c), 0, N, C, x.data_ptr(), ptrs, len(tiles), E._stream()) == E.E_ARG
        assert L.mdtile_lattice_weight_map(ctypes.byref(c), None, wmap.data_ptr(), E._stream()) == E.E_ARG
    many = E.Lattice(100, 100, 10, 10, 5, 1, 5, 5)
    assert many.num_batches == 361 > E.MAX_BATCHES
    with pytest.raises(E.MdtileError, match=r"rc=-1.*MDTILE_MAX_BATCHES"):
        E.blend_lattice(many, E.METHOD_MD, [torch.ones(N, C, 10, 10, device=cuda)] * 361, N, C, out=torch.full((N, C, 100, 100), NAN, device=cuda))
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in tiles), "a refused gather wrote to its output"
    assert torch.isnan(out).all(), "a refused blend wrote to its output"
    assert torch.isnan(wmap).all(), "a refused weight map wrote to its output"


# ---- the delegates with the option set -----------------------------------------------------------------------------------------------
@pytest.fixture
def jitter_option():
    """The stub host with --mdtile-grid-jitter; the option is gone and the step counter is back afterwards."""
    _, shared = sh.host()
    step = shared.state.sampling_step
    shared.cmd_opts.mdtile_grid_jitter = True
    try:
        yield shared
    finally:
        if hasattr(shared.cmd_opts, "mdtile_grid_jitter"):
            del shared.cmd_opts.mdtile_grid_jitter
        shared.state.sampling_step = step


@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_jitters_the_grid_every_step(plugin, cuda, jitter_option, method):
    """MultiDiffusion / MixtureOfDiffusers with --mdtile-grid-jitter over three sampler steps: every step's result is the restatement's at that
    step's pinned lattice, the lattices differ pairwise (and in their tile count), and the image conditioning fed to the model with every batch
    is cut at the pushed-in boxes."""
    shared, seed = jitter_option, 1234567
    Wc, Hc, tw, th, ov = GEOMETRIES["odd"]
    d, p = make_delegate(plugin, method, Wc, Hc, tw, th, ov, 4)
    p.all_seeds = [seed]
    assert d.grid_jitter and d.total_bboxes == 4      # up to 4 x 4 tiles in batches of 4; the fixed grid has 9 in 3 batches of 3
    x = _canvas("odd", "f32")
    torch.manual_seed(3)
    icond = torch.randn(N, 5, Hc, Wc)
    cond = {"c_crossattn": [torch.zeros(N, 77, 768, device=cuda)], "c_concat": [icond.to(cuda)]}
    tile_w = d.get_tile_weights() if method == "mod" else None
    pinned = [(10, 6), (4, 8), (6, 7)]                # lattice_shift(1234567, step, axis, 12 | 8), steps 0 .. 2
    counts = []
    for step, (sx, sy) in enumerate(pinned):
        shared.state.sampling_step = step
        assert lr.step_shift(Wc, Hc, tw, th, ov, seed, step) == (sx, sy)
        g = lr.lattice(Wc, Hc, tw, th, ov, 4, sx, sy)
        counts.append(len(g.boxes))
        seen = []
        if method == "md":
            def repeat(xt, bboxes):
                seen.append(d.get_icond(d.repeat_cond_dict(cond, bboxes)))
                return _tile_fn(xt)
            out = d.sample_one_step(x.to(cuda), None, repeat, None)
        else:
            def model(x_, t_, c_):
                seen.append(d.get_icond(c_))
                return _tile_fn(x_)
            shared.sd_model.apply_model_original_md = model
            out = d.apply_model_hijack(x.to(cuda), torch.zeros(N, device=cuda), cond)
        tiles = [_tile_fn(torch.from_numpy(lr.gather(g, x.numpy(), b))) for b in range(len(g.batches))]
        _assert_bitwise(out, _blend_ref(g, method, tiles, tile_w, torch.float32), f"delegate {method} step {step} lattice ({sx}, {sy})")
        assert len(seen) == len(g.batches)
        for b, batch in enumerate(g.batches):
            want = torch.cat([icond[:, :, y:y + h, x_:x_ + w] for (x_, y, w, h) in (g.boxes[t] for t in batch)], dim=0)
            _assert_bitwise(seen[b], want.contiguous(), f"delegate {method} step {step} image conditioning of batch {b}")
    assert len(set(pinned)) == 3 and counts == [9, 12, 12]
    assert p.extra_generation_params["Tiled Diffusion grid jitter"] is True
