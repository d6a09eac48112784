"""--mdtile-jitter-regions without a GPU: the numpy restatement tests/lattice_region_ref.py against the restatements it must
agree with -- without regions tests/grid_lattice_ref.py's blend, at rest on an exact-fit canvas the plain region blend of oracle/blend_oracle.py --
and a literal example of the one place where the grouping of the weight sum may differ; header = library = binding for the new struct; every
refusal by name (argument checks happen before any device is touched); the option; and the delegates' wiring on the CPU stub host with engine
doubles: one lattice per step, the raw weights and region_w handed to blend_lattice_regions, Noise Inversion's own evaluations on mdtile.blend
with the premultiplied weights, every not-applied line once per job, the bar's size, the infotext, no random generator touched.  The kernel is
tested in tests/test_gpu_lattice_regions.py."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import blend_oracle as bo

import grid_lattice_ref as gl
import lattice_region_ref as rr
import lattice_region_cases as cases
from wrap_common import host, wired, delegate, load_preload      # noqa: F401  (host, wired: fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, TILE, OV, BS = 40, 24, 16, 4, 4      # stride 12: 3 columns at rest, 4 at any other shift; 2 rows at shifts 4 .. 12, 3 below
SEED = 1234567
N, C = 2, 4
OLD_REASON = ("[Tiled Diffusion] --mdtile-grid-jitter not applied: region prompt control is enabled (custom regions, or no background to draw); "
              "the grid stays where it is.")


# ---- symbols ---------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(built_lib):
    name = "mdtile_blend_lattice_regions"
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdtile.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mdtile_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(built_lib.LIB_PATH)
    assert name in declared, f"{name} is not declared in include/mdtile.h"
    assert hasattr(lib, name), f"libmdtile.so does not export {name}"
    assert name in built_lib.exported_symbols(), f"the binding has no signature for {name}"
    params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
    assert len(built_lib._SIGNATURES[name][1]) == len(params.split(",")) == 6, f"{name}: the binding's argument count is not the header's"
    assert sorted(built_lib.exported_symbols()) == sorted(declared)
    assert built_lib.lib().mdtile_version() == 100
    fields = re.search(r"typedef struct mdtile_lattice_regions \{(.*?)\} mdtile_lattice_regions;", src, flags=re.S).group(1)
    decls = re.findall(r"(const\s+\w+\s*\*|int)\s*(\w+)\s*;", fields)
    assert [n for _, n in decls] == [n for n, _ in built_lib._LatticeRegions._fields_] == ["regions", "num_regions", "d_region_w"]
    kinds = ["pointer" if "*" in t else "int" for t, _ in decls]
    want = ["int" if t is ctypes.c_int else "pointer" for _, t in built_lib._LatticeRegions._fields_]
    assert kinds == want == ["pointer", "int", "pointer"], "the binding's struct is not the header's, field for field"
    assert ctypes.sizeof(built_lib._LatticeRegions) == 24
    assert callable(built_lib.blend_lattice_regions)


def test_no_cpu_fallback(built_lib):
    """The new call takes device tensors only, as its neighbours."""
    lat = built_lib.Lattice(W, H, TILE, TILE, OV, BS, 5, 5)
    tiles = [torch.zeros(len(b) * N, C, TILE, TILE) for b in lat.batches]
    with pytest.raises((AssertionError, built_lib.MdtileError, RuntimeError)):
        built_lib.blend_lattice_regions(lat, built_lib.METHOD_MD, tiles, N, C)


# ---- the restatement against the restatements it must agree with -----------------------------------------------------------------------
def _regions(spec, method, seed, n=N, c=C, gaussian=gl.gaussian, feather=None):
    rng = np.random.default_rng(seed)
    out = []
    for (x, y, w, h, mode) in spec:
        o = rng.standard_normal((n, c, h, w)).astype(np.float32)
        if mode == "fg":
            wgt = rng.random((h, w)).astype(np.float32) if feather is None else feather(w, h)
        else:
            wgt = None if method == "md" else gaussian(w, h)
        out.append(rr.Region(x, y, w, h, mode, o, wgt))
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


@pytest.mark.parametrize("geom", list(cases.GEOMETRIES))
@pytest.mark.parametrize("method", ["md", "mod"])
def test_a_without_regions_it_is_the_lattice_blend(geom, method):
    """(A) num_regions = 0 with no map, or with a map of zeros: grid_lattice_ref.blend, bit for bit, at every shift of the set."""
    Wc, Hc, tw, th, ov = cases.GEOMETRIES[geom]
    for (sx, sy) in cases.shifts(geom):
        g = gl.lattice(Wc, Hc, tw, th, ov, 4, sx, sy)
        tile_w = gl.gaussian(g.tw, g.th) if method == "mod" else None
        tiles = np.random.default_rng(sx * 31 + sy).standard_normal((len(g.boxes) * N, C, g.th, g.tw)).astype(np.float32)
        want = gl.blend(g, method, tiles, N, tile_w)
        assert np.isfinite(want).all()
        for region_w in (None, np.zeros((Hc, Wc), np.float32)):
            got = rr.blend(g, method, tiles, N, (), region_w, tile_w)
            assert np.array_equal(_bits(got), _bits(want)), (geom, method, sx, sy, region_w is None)


@pytest.mark.parametrize("geom", cases.REST, ids=lambda g: "x".join(map(str, g)))
@pytest.mark.parametrize("method", ["md", "mod"])
def test_b_at_rest_it_is_the_plain_region_blend(geom, method):
    """(B) at rest on a canvas the stride divides the lattice is the plain plan, and the result is the plain region blend's (the oracle the
    existing blend tests check mdtile_blend against: running `+=` weight map, reciprocal, premultiplied region Gaussians), bit for bit.
    MultiDiffusion: any regions, overlapping BG regions included.  Mixture of Diffusers: no pixel under two BG regions."""
    Wc, Hc, tw, th, ov, bs = geom
    stx, sty = gl.rest(Wc, Hc, tw, th, ov)
    g = gl.lattice(Wc, Hc, tw, th, ov, bs, stx, sty)
    spec = cases.full_spec(Wc, Hc) if method == "md" else cases.disjoint_bg_spec(Wc, Hc)
    oracle = bo.BlendOracle(method, Wc, Hc, tw, th, ov, bs, [bo.Region(x, y, w, h, bo.BG if mode == "bg" else bo.FG, 0.3) for (x, y, w, h, mode) in spec])
    assert [tuple(b) for b in oracle.boxes] == list(g.boxes), "at rest the lattice is not the plain plan"
    regions = _regions(spec, method, 5, gaussian=lambda w, h: bo.gaussian_weights(w, h).numpy(),
                       feather=lambda w, h: bo.feather_mask(w, h, 0.3).numpy())
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((N, C, Hc, Wc)).astype(np.float32))
    want = oracle.evaluate(x, bo.synthetic_denoiser, lambda xr, i: torch.from_numpy(regions[i].out)).numpy()
    tiles = np.concatenate([bo.synthetic_denoiser(torch.from_numpy(gl.gather(g, x.numpy(), b))).numpy() for b in range(len(g.batches))], axis=0)
    tile_w = bo.gaussian_weights(g.tw, g.th).numpy() if method == "mod" else None
    region_w = rr.region_w_map(Wc, Hc, method, regions)
    got = rr.blend(g, method, tiles, N, regions, region_w, tile_w)
    assert np.isfinite(want).all()
    assert np.array_equal(_bits(got), _bits(want)), (geom, method)
    if method == "md":
        assert np.array_equal(_bits(gl.weight_map(g) + region_w), _bits(oracle.weights.numpy()[0, 0])) and oracle.weights.max() >= 4


def test_two_background_regions_group_the_weight_sum_differently():
    """Mixture of Diffusers under two overlapping BG regions: the definition adds the regions' map to the grid's sum, gw + (c1 + c2); the plain
    path's running sum is (gw + c1) + c2.  With gw = 1 and c1 = c2 = 2^-24 (half an ulp of 1) the first is 1 + 2^-23, the second 1."""
    one, c = np.float32(1.0), np.float32(2.0 ** -24)
    grouped, running = one + (c + c), (one + c) + c
    assert grouped == np.float32(1.0 + 2.0 ** -23) and running == one and grouped != running
    # the same through the restatement: one 8 x 8 tile of weight 1 spanning an 8 x 8 canvas, two BG regions of weight 2^-24 that overlap in x = 2 .. 5
    g = gl.lattice(8, 8, 8, 8, 0, 1, 1, 1)
    assert g.boxes == ((0, 0, 8, 8),)
    tiles = np.ones((1, 1, 8, 8), np.float32)
    regions = [rr.Region(0, 0, 6, 8, "bg", np.zeros((1, 1, 8, 6), np.float32), np.full((8, 6), c)),
               rr.Region(2, 0, 6, 8, "bg", np.zeros((1, 1, 8, 6), np.float32), np.full((8, 6), c))]
    region_w = rr.region_w_map(8, 8, "mod", regions)
    assert region_w[0, 3] == c + c and region_w[0, 0] == c
    got = rr.blend(g, "mod", tiles, 1, regions, region_w, np.ones((8, 8), np.float32))
    assert got[0, 0, 0, 3] == one / grouped != one            # the definition: 1 * (1 * (1 / (1 + 2^-23)))
    assert got[0, 0, 0, 0] == one                             # under one region: 1 + 2^-24 rounds to 1 either way
    plain = np.ones((8, 8), np.float32)                       # the plain path: the grid's sum, then `+=` per region
    for R in regions:
        rr.wrap_region_ref.weight_map_add_rect(plain, R.x, R.y, R.w, R.h, R.weight)
    assert plain[0, 3] == one, "the running sum of the plain path stays at 1"


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _fake(n):
    """n pointers that are not null and are never followed: a refused call reads no device memory."""
    return (ctypes.c_void_p * n)(*([0x1000] * n))


def test_calls_refuse_before_any_device_is_touched(built_lib):
    E, L = built_lib, built_lib.lib()
    lat = E.Lattice(W, H, TILE, TILE, OV, BS, 5, 5)
    nb = lat.num_batches

    def region(x=1, y=1, w=4, h=4, mode=E.REGION_BG, out=0x1000, weight=0x1000):
        return E._Region(x, y, w, h, mode, 0, out, weight)

    def blend(text, regions=(), region_w=0x1000, lat_c=None, nbat=nb, null_block=False, null_list=False, count=None, **kw):
        f = dict(method=E.METHOD_MD, dtype=0, N=2, C=4, flags=0, tile_lo=0, tile_hi=0, row_lo=0, row_hi=0, d_weights=None, d_tile_w=None, d_rescale=None,
                 d_x_out=0x1000)
        f.update(kw)
        a = E._BlendArgs(**f)
        arr = (E._Region * max(1, len(regions)))(*regions)
        block = E._LatticeRegions(None if null_list else arr, len(regions) if count is None else count, region_w)
        rc = L.mdtile_blend_lattice_regions(ctypes.byref(lat_c) if lat_c is not None else lat.ref, ctypes.byref(a), _fake(max(nbat, 1)), nbat,
                                            None if null_block else ctypes.byref(block), None)
        assert rc == E.E_ARG, (text, rc)
        err = L.mdtile_last_error().decode()
        assert err.startswith("mdtile_blend_lattice_regions:") and re.search(text, err), err

    # everything mdtile_blend_lattice refuses
    blend(r"%d batches given, the lattice has %d" % (nb + 1, nb), nbat=nb + 1)
    blend("d_weights and d_rescale must be NULL", d_weights=0x1000)
    blend("d_weights and d_rescale must be NULL", d_rescale=0x1000, method=E.METHOD_MOD, d_tile_w=0x1000)
    blend("no MDTILE_BLEND_\\* flags", flags=E.BLEND_PARTIAL)
    blend("no MDTILE_BLEND_\\* flags", flags=E.BLEND_PACKED)
    blend("no row band", row_lo=0, row_hi=8)
    blend("Mixture of Diffusers needs d_tile_w", method=E.METHOD_MOD)
    blend("bad method", method=2)
    blend("bad dtype", dtype=3)
    blend("bad N=0", N=0)
    blend("null output", d_x_out=None)
    c = E._Lattice(*[getattr(lat._c, n) for n, _ in E._Lattice._fields_])
    c.sx = 0
    blend(r"sx = 0 outside \[1, 12\]", lat_c=c)
    many = E.Lattice(100, 100, 10, 10, 5, 1, 5, 5)
    blend("MDTILE_MAX_BATCHES", lat_c=many._c, nbat=many.num_batches)
    # the regions block
    blend("null regions block", null_block=True)
    blend("17 regions", regions=[region()] * 17)
    blend("-1 regions", count=-1)
    blend("null regions", null_list=True, count=1)
    for bad in (dict(w=0), dict(h=0), dict(x=-1), dict(y=-1), dict(x=W - 3), dict(y=H - 3), dict(w=W + 1, x=0), dict(x=2 ** 31 - 1, w=2 ** 31 - 1)):
        blend(r"region 1 \(.*\) does not lie on the %dx%d canvas" % (W, H), regions=[region(), region(**bad)])
    blend("region 0 bad mode 7", regions=[region(mode=7)])
    blend("region 0 has no output", regions=[region(out=None)])
    blend("region 0 \\(foreground\\) needs its feather mask", regions=[region(mode=E.REGION_FG, weight=None)])
    blend("region 0 \\(background, Mixture of Diffusers\\) needs its raw Gaussian", regions=[region(weight=None)], method=E.METHOD_MOD, d_tile_w=0x1000)
    blend("null d_region_w with 1 background region", regions=[region(mode=E.REGION_FG), region(weight=None)], region_w=None)


# ---- the option ------------------------------------------------------------------------------------------------------------------
OPTIONS = ("mdtile_grid_jitter", "mdtile_jitter_regions", "mdtile_grid_shift", "mdtile_inpaint_skip", "mdtile_wrap_x", "mdtile_wrap_y",
           "mdtile_wrap_regions")


def test_preload_option(host):
    pl, shared = host
    parser = argparse.ArgumentParser()
    load_preload().preload(parser)
    assert parser.parse_args([]).mdtile_jitter_regions is False
    ns = parser.parse_args(["--mdtile-jitter-regions"])
    assert ns.mdtile_jitter_regions is True and ns.mdtile_grid_jitter is False
    A = pl.abstractdiffusion.AbstractDiffusion
    assert not hasattr(shared.cmd_opts, "mdtile_jitter_regions") and A.jitter_regions_requested() is False      # a host that never heard of the option
    shared.cmd_opts.mdtile_jitter_regions = True
    try:
        assert A.jitter_regions_requested() is True
    finally:
        del shared.cmd_opts.mdtile_jitter_regions


# ---- wiring ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def jobs(wired, monkeypatch):
    """(plugin, shared, calls): wired, every option gone before and after, the step counter restored, and the engine calls of an evaluation with
    regions replaced by doubles that record what they were handed.  The maps are computed for real (numpy), so that raw and premultiplied
    weights can be told apart."""
    pl, shared = wired
    calls = []

    def gather_all_lattice(lat, x_in, out=None):
        calls.append(("gather", lat))
        g = gl.lattice(lat.w, lat.h, TILE, TILE, OV, BS, lat.sx, lat.sy)
        assert list(g.boxes) == lat.bboxes
        return [torch.from_numpy(gl.gather(g, x_in.numpy(), b)) for b in range(len(g.batches))]

    def blend_lattice(lat, method, batch_out, N_, C_, *, tile_w=None, **kw):
        assert not kw
        calls.append(("blend", lat))
        return torch.zeros(N_, C_, lat.h, lat.w)

    def blend_lattice_regions(lat, method, batch_out, N_, C_, *, regions=(), region_w=None, tile_w=None, **kw):
        assert not kw and len(batch_out) == lat.num_batches and (tile_w is not None) == (method == pl.engine.METHOD_MOD)
        calls.append(("blend regions", lat, list(regions), region_w))
        return torch.zeros(N_, C_, lat.h, lat.w)

    def gather_all(plan, x_in, out=None):
        calls.append(("plain gather",))
        return [torch.zeros(len(b) * x_in.shape[0], x_in.shape[1], plan.tile_h, plan.tile_w) for b in plan.batches]

    def blend(plan, method, batch_out, N_, C_, *, regions=(), weights=None, rescale=None, **kw):
        calls.append(("plain blend", list(regions), weights, rescale))
        return torch.zeros(N_, C_, plan.h, plan.w)

    def gather_rect(x_in, x, y, w, h):
        calls.append(("gather rect", x, y, w, h))
        return x_in[:, :, y:y + h, x:x + w].contiguous()

    def add_rect(weights, x, y, w, h, rect_w=None, scalar=1.0):
        weights[..., y:y + h, x:x + w] += scalar if rect_w is None else rect_w.reshape(h, w)

    def rect_mul_canvas(rect_w, canvas, x, y, w, h):
        rect_w *= canvas[..., y:y + h, x:x + w]

    for name, fn in (("gather_all_lattice", gather_all_lattice), ("blend_lattice", blend_lattice), ("blend_lattice_regions", blend_lattice_regions),
                     ("gather_all", gather_all), ("blend", blend), ("gather_rect", gather_rect), ("weight_map_add_rect", add_rect),
                     ("rect_mul_canvas", rect_mul_canvas), ("reciprocal", lambda t: 1.0 / t)):
        monkeypatch.setattr(pl.engine, name, fn)
    monkeypatch.setattr(pl.utils, "feather_mask", lambda w, h, ratio: torch.full((h, w), 0.25))
    monkeypatch.setattr(shared.state, "sampling_step", 0)
    for n in OPTIONS:
        if hasattr(shared.cmd_opts, n):
            monkeypatch.delattr(shared.cmd_opts, n)
    yield pl, shared, calls
    for n in OPTIONS:
        if hasattr(shared.cmd_opts, n):
            delattr(shared.cmd_opts, n)


REGIONS = ((0.1, 0.1, 0.5, 0.5, "Background"), (0.3, 0.25, 0.4, 0.5, "Foreground"))
BOXES = [(4, 2, 20, 12), (12, 6, 16, 12)]


def _job(pl, shared, method, regions=REGIONS, background=True, grid=True, **opts):
    """The delegate as the script sets it up: grid (unless no background is drawn), regions, init_done; the bar closed."""
    for k, v in opts.items():
        setattr(shared.cmd_opts, k, v)
    if grid:
        d, p = delegate(pl, W, H, TILE, TILE, OV, BS, method)
    else:
        from hostsim import stub_host as sh
        cls = pl.multidiffusion.MultiDiffusion if method == "md" else pl.mixtureofdiffusers.MixtureOfDiffusers
        p = sh.make_processing(W * 8, H * 8)
        d = cls(p, sh.kdiff_sampler())
    p.all_seeds = [SEED]
    if method == "mod":
        d.get_weight = lambda w, h: torch.full((h, w), 0.5)      # a region's Gaussian; the tile's was made (ones) when the grid was laid
    if regions:
        settings = {i: pl.utils.BBoxSettings(True, fx, fy, fw, fh, "", "", mode, 0.2, -1) for i, (fx, fy, fw, fh, mode) in enumerate(regions)}
        d.init_custom_bbox(settings, background, False)
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    d.update_pbar = lambda: None
    return d, p


def _evaluate(d, shared, method, x, own=False):
    if method == "md":
        return d.sample_one_step(x, None, lambda xt, bboxes: xt, lambda xt, bbox_id, bbox: xt, **(dict(own_evaluation=d.NOISE_INVERSION_FULL) if own else {}))
    shared.sd_model.apply_model_original_md = lambda x_, t_, c_: x_
    shared.sd_model.apply_model = lambda x_, t_, cond=None: x_
    d.custom_apply_model = lambda xt, t_in, c_in, bbox_id, bbox: xt
    cond = {"c_crossattn": [torch.zeros(2, 77, 8)], "c_concat": [torch.zeros(2, 5, 1, 1)]}
    return d.apply_model_hijack(x, torch.zeros(2), cond, **(dict(noise_inverse_step=0) if own else {}))


def _want(step):
    return gl.step_shift(W, H, TILE, TILE, OV, SEED, step)


def _names(calls):
    return [c[0] for c in calls]


PLAIN = ["plain gather", "gather rect", "gather rect", "plain blend"]


@pytest.mark.parametrize("method", ["md", "mod"])
def test_regions_ride_the_moving_grid(jobs, capsys, monkeypatch, method):
    """--mdtile-grid-jitter --mdtile-jitter-regions with one BG and one FG region: every evaluation gathers at the step's lattice, cuts the
    regions where they are, and ends in blend_lattice_regions with that lattice, the RAW weights and region_w; one lattice object per step
    value; the bar is sized from the largest lattice plus the regions; the infotext says so; no random generator is touched."""
    pl, shared, calls = jobs
    monkeypatch.setattr(pl.utils.Condition, "reconstruct_cond", staticmethod(lambda cond, step: torch.zeros(1, 77, 8)))
    d, p = _job(pl, shared, method, mdtile_grid_jitter=True, mdtile_jitter_regions=True)
    assert d.grid_jitter and d.jitter_regions and not d.wrap_regions
    assert [(b.x, b.y, b.w, b.h) for b in d.custom_bboxes] == BOXES
    assert d.num_batches == 2 and d.jitter_max_batches == 3 and d.total_bboxes == 3 + 2
    assert "Tiled Diffusion jitter regions" not in (getattr(p, "extra_generation_params", None) or {})
    # both forms of the maps: self.weights with the region added (the grid's own sum is a no-op double here), region_w the region alone
    bg = 1.0 if method == "md" else 0.5
    want_map = torch.zeros(H, W)
    want_map[2:14, 4:24] = bg
    assert torch.equal(d.region_w[0, 0], want_map) and torch.equal(d.weights[0, 0], want_map) and d.region_w is not d.weights
    x = torch.randn(2, 4, H, W)
    rng = torch.get_rng_state()
    per_step = []
    for step in (0, 0, 1, 2):
        shared.state.sampling_step = step
        del calls[:]
        out = _evaluate(d, shared, method, x)
        assert tuple(out.shape) == (2, 4, H, W)
        assert _names(calls) == ["gather", "gather rect", "gather rect", "blend regions"], calls
        lat = calls[0][1]
        assert (lat.sx, lat.sy) == _want(step) and calls[3][1] is lat
        assert [c[1:] for c in calls[1:3]] == BOXES, "the regions stay where the user put them"
        _, _, regions, region_w = calls[3]
        assert region_w is d.region_w
        assert [(r.x, r.y, r.w, r.h, r.mode) for r in regions] == [BOXES[0] + (pl.engine.REGION_BG,), BOXES[1] + (pl.engine.REGION_FG,)]
        assert torch.equal(regions[1].weight, torch.full((12, 16), 0.25))
        if method == "md":
            assert regions[0].weight is None
        else:      # the raw Gaussian, not the copy init_done multiplied by rescale_factor (0.5 * 1 / 0.5 = 1 inside the region)
            assert torch.equal(regions[0].weight.reshape(12, 20), torch.full((12, 20), 0.5))
            assert torch.equal(d.custom_weights[0].reshape(12, 20), torch.ones(12, 20))
        per_step.append(lat)
    assert per_step[0] is per_step[1] and len({(l.sx, l.sy) for l in per_step}) == 3, "one lattice per step value, another one every step"
    assert torch.equal(torch.get_rng_state(), rng)
    assert p.extra_generation_params["Tiled Diffusion jitter regions"] is True and p.extra_generation_params["Tiled Diffusion grid jitter"] is True
    assert "[Tiled Diffusion]" not in capsys.readouterr().out
    # Noise Inversion's own evaluations of the same job: the fixed grid, mdtile.blend, the forms of before
    for _ in range(2):
        del calls[:]
        _evaluate(d, shared, method, x, own=True)
        assert _names(calls) == PLAIN, calls
        _, regions, weights, rescale = calls[3]
        if method == "md":
            assert weights is d.weights and regions[0].weight is None
        else:
            assert rescale is d.rescale_factor and torch.equal(regions[0].weight.reshape(12, 20), torch.ones(12, 20)), "premultiplied weights"
    text = capsys.readouterr().out
    assert text.count("[Tiled Diffusion]") == 1 and text.count("--mdtile-grid-jitter not applied") == 1 and "Noise Inversion" in text
    del calls[:]
    _evaluate(d, shared, method, x)                      # and the sampler's own evaluations still move
    assert _names(calls)[-1] == "blend regions"


@pytest.mark.parametrize("method", ["md", "mod"])
def test_without_the_switch_nothing_changes(jobs, capsys, method):
    """--mdtile-grid-jitter and regions, no --mdtile-jitter-regions: the line of before, word for word and once, and the calls of before."""
    pl, shared, calls = jobs
    d, p = _job(pl, shared, method, mdtile_grid_jitter=True)
    assert d.grid_jitter and not d.jitter_regions and d.region_w is None and d.total_bboxes == 2 + 2
    for step in (0, 1):
        shared.state.sampling_step = step
        del calls[:]
        _evaluate(d, shared, method, torch.randn(2, 4, H, W))
        assert _names(calls) == PLAIN
    out = capsys.readouterr().out
    assert out.count("[Tiled Diffusion]") == 1 and OLD_REASON in out, out
    assert not any(k in (getattr(p, "extra_generation_params", None) or {}) for k in ("Tiled Diffusion jitter regions", "Tiled Diffusion grid jitter"))


@pytest.mark.parametrize("method", ["md", "mod"])
def test_the_switch_alone_is_ignored(jobs, capsys, method):
    """--mdtile-jitter-regions without --mdtile-grid-jitter: one line, and the calls of a job with neither."""
    pl, shared, calls = jobs
    runs = []
    for opts in ({}, dict(mdtile_jitter_regions=True)):
        d, p = _job(pl, shared, method, **opts)
        assert not d.grid_jitter and not d.jitter_regions and d.region_w is None and d.total_bboxes == 2 + 2
        del calls[:]
        for step in (0, 1):
            shared.state.sampling_step = step
            _evaluate(d, shared, method, torch.randn(2, 4, H, W))
        runs.append((_names(calls), capsys.readouterr().out))
    assert runs[0][0] == runs[1][0] == PLAIN * 2
    assert "[Tiled Diffusion]" not in runs[0][1]
    assert runs[1][1].count("[Tiled Diffusion]") == 1 and "--mdtile-jitter-regions ignored" in runs[1][1] and "--mdtile-grid-jitter" in runs[1][1]


@pytest.mark.parametrize("method", ["md", "mod"])
def test_both_switches_without_regions(jobs, capsys, method):
    """No regions: the jittered job of before, on mdtile.blend_lattice, with no line and no new infotext."""
    pl, shared, calls = jobs
    runs = []
    for opts in (dict(mdtile_grid_jitter=True), dict(mdtile_grid_jitter=True, mdtile_jitter_regions=True)):
        d, p = _job(pl, shared, method, regions=(), **opts)
        assert d.grid_jitter and not d.jitter_regions and d.total_bboxes == 3
        del calls[:]
        for step in (0, 1):
            shared.state.sampling_step = step
            _evaluate(d, shared, method, torch.randn(2, 4, H, W))
        runs.append([(c[0], c[1].sx, c[1].sy) for c in calls])
        assert "[Tiled Diffusion]" not in capsys.readouterr().out
        assert "Tiled Diffusion jitter regions" not in p.extra_generation_params and p.extra_generation_params["Tiled Diffusion grid jitter"] is True
    assert runs[0] == runs[1] == [(n,) + _want(step) for step in (0, 1) for n in ("gather", "blend")]


@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("grid", [False, True])
def test_no_background_means_no_grid_to_move(jobs, capsys, method, grid):
    """Both switches, regions, draw_background False: the regions are painted where they are on the fixed path, and one line gives the reason --
    whether the script never laid a grid (as it does without a background) or a grid was laid before the regions turned it off."""
    pl, shared, calls = jobs
    d, p = _job(pl, shared, method, background=False, grid=grid, mdtile_grid_jitter=True, mdtile_jitter_regions=True)
    assert not d.jitter_regions and not d.draw_background and d.region_w is None and d.total_bboxes == 2
    for step in (0, 1):
        shared.state.sampling_step = step
        del calls[:]
        _evaluate(d, shared, method, torch.randn(2, 4, H, W))
        assert _names(calls) == ["gather rect", "gather rect", "plain blend"]
    out = capsys.readouterr().out
    assert out.count("[Tiled Diffusion]") == 1 and "--mdtile-jitter-regions has no grid to move" in out, out
    assert "Tiled Diffusion jitter regions" not in (getattr(p, "extra_generation_params", None) or {})


def test_kept_apart_from_a_canvas_that_wraps(jobs, capsys):
    """On a wrap plan --mdtile-grid-jitter is not applied (its own line), so the new switch means nothing there; regions there are
    --mdtile-wrap-regions' business, and without that switch the refusal of before stands."""
    pl, shared, calls = jobs
    for k in ("mdtile_grid_jitter", "mdtile_jitter_regions", "mdtile_wrap_x"):
        setattr(shared.cmd_opts, k, True)
    d, _ = delegate(pl, W, H, TILE, TILE, OV, BS)
    assert not d.grid_jitter
    settings = {0: pl.utils.BBoxSettings(True, 0.1, 0.1, 0.5, 0.5, "", "", "Background", 0.2, -1)}
    with pytest.raises(RuntimeError, match="no region path"):
        d.init_custom_bbox(settings, True, False)
    out = capsys.readouterr().out
    assert out.count("[Tiled Diffusion]") == 1 and "use --mdtile-grid-shift there" in out
