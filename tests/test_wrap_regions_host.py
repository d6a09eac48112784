"""--mdtile-wrap-regions without a GPU: the header, the exports and the binding; the option; the one rectangle rule on both kinds
of axis; the refusal that stays without the option and the line when no axis wraps; the extended copies of a region that hangs over further
than any tile; the delegates' wiring on the CPU stub host with the engine's new calls replaced by doubles (the restatement
tests/wrap_region_ref.py); and the restatement against itself -- without regions it is tests/shift_ref.py's shifted blend, with regions it
commutes with rolling the whole canvas.  The kernels are tested in tests/test_gpu_wrap_regions.py."""
import argparse
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import shift_ref as sr
import wrap_ref as wr
import wrap_region_ref as rr
from wrap_common import host, wired, delegate, load_preload, take as _take      # noqa: F401  (host, wired: fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mdtile_gather_rect_wrap", "mdtile_weight_map_add_rect_wrap", "mdtile_region_noise_wrap", "mdtile_blend_wrap_regions"]
W, H, TILE, OV, BS = 40, 24, 24, 16, 2      # the cylinder of tests/test_gpu_wrap.py: columns 0, 8, 16, 24, 32; the last passes the edge by 16
N, C = 2, 4


# ---- symbols ---------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdtile.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mdtile_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(built_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/mdtile.h"
        assert hasattr(lib, name), f"libmdtile.so does not export {name}"
        assert name in built_lib.exported_symbols(), f"the binding has no signature for {name}"
        params = re.search(r"\b" + name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(built_lib._SIGNATURES[name][1]) == len(params.split(",")), f"{name}: the binding's argument count is not the header's"
    assert sorted(built_lib.exported_symbols()) == sorted(declared)
    fields = re.search(r"typedef struct mdtile_wrap_regions \{(.*?)\} mdtile_wrap_regions;", src, flags=re.S).group(1)
    names = [n.strip().lstrip("*") for decl in re.findall(r"(?:const\s+\w+\s*\*|int)\s*([^;]+);", fields) for n in decl.split(",")]
    assert names == [n for n, _ in built_lib._WrapRegions._fields_], "the binding's struct is not the header's"
    for fn in ("gather_rect_wrap", "weight_map_add_rect_wrap", "region_noise_wrap", "blend_wrap_regions"):
        assert callable(getattr(built_lib, fn))


def test_no_cpu_fallback(built_lib):
    """The new calls take device tensors only, as their neighbours."""
    with pytest.raises((AssertionError, built_lib.MdtileError, RuntimeError)):
        built_lib.gather_rect_wrap(torch.zeros(1, 1, 4, 4), 0, 0, 2, 2, wrap_x=True, wrap_y=False)
    with pytest.raises((AssertionError, built_lib.MdtileError, RuntimeError)):
        built_lib.weight_map_add_rect_wrap(torch.zeros(4, 4), 0, 0, 2, 2, wrap_x=True, wrap_y=False)


# ---- the option ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def option(host):
    """(plugin, shared) with --mdtile-wrap-regions and --mdtile-grid-shift gone before and after."""
    pl, shared = host

    def clear():
        for name in ("mdtile_wrap_regions", "mdtile_grid_shift"):
            if hasattr(shared.cmd_opts, name):
                delattr(shared.cmd_opts, name)

    clear()
    step = shared.state.sampling_step
    yield pl, shared
    clear()
    shared.state.sampling_step = step


def test_preload_option(option):
    pl, shared = option
    parser = argparse.ArgumentParser()
    load_preload().preload(parser)
    assert parser.parse_args([]).mdtile_wrap_regions is False
    ns = parser.parse_args(["--mdtile-wrap-regions"])
    assert ns.mdtile_wrap_regions is True and ns.mdtile_wrap_x is False and ns.mdtile_wrap_y is False
    A = pl.abstractdiffusion.AbstractDiffusion
    assert A.wrap_regions_requested() is False      # a host that never heard of the option
    shared.cmd_opts.mdtile_wrap_regions = True
    assert A.wrap_regions_requested() is True


# ---- the rectangle rule ----------------------------------------------------------------------------------------------------------
def test_rectangle_rule_on_literal_numbers(option):
    pl, _ = option
    rect = pl.utils.region_rect
    # an axis that does not wrap: today's rule, clipped at the edge; fx = 1.0 leaves an empty rectangle at the edge, as upstream
    assert rect(0.1, 0.1, 0.4, 0.4, 40, 24) == (4, 2, 16, 10)
    assert rect(0.9, 0.5, 0.6, 0.75, 40, 24) == (36, 12, 4, 12)
    assert rect(1.0, 1.0, 0.5, 0.5, 40, 24) == (40, 24, 0, 0)
    assert rect(0.0, 0.0, 1.0, 1.0, 40, 24) == (0, 0, 40, 24)
    assert rect(-0.2, 0.0, 0.3, 2.0, 40, 24) == (0, 0, 12, 24)
    # an axis that wraps: the origin mod the extent, the size no larger than the extent, x + w > W legal
    assert rect(0.9, 0.5, 0.6, 0.75, 40, 24, True, False) == (36, 12, 24, 12)
    assert rect(0.9, 0.5, 0.6, 0.75, 40, 24, False, True) == (36, 12, 4, 18)
    assert rect(0.9, 0.5, 0.6, 0.75, 40, 24, True, True) == (36, 12, 24, 18)
    assert rect(1.0, 1.0, 0.5, 0.5, 40, 24, True, True) == (0, 0, 20, 12)
    assert rect(0.5, 0.5, 1.0, 1.0, 40, 24, True, True) == (20, 12, 40, 24)
    assert rect(0.5, 0.5, 1.5, 3.0, 40, 24, True, True) == (20, 12, 40, 24)
    assert rect(0.975, 0.0, 0.001, 0.001, 40, 24, True, False) == (39, 0, 1, 1)


def test_rectangle_rule_is_the_restatement(option):
    pl, _ = option
    fr = [0.0, 0.01, 0.1, 0.25, 0.4999, 0.5, 0.75, 0.9, 0.975, 0.9999, 1.0]
    for (cw, ch) in ((40, 24), (37, 22), (38, 16)):
        for wx in (False, True):
            for wy in (False, True):
                for fx in fr:
                    for fw in fr[1:] + [1.3]:
                        got = pl.utils.region_rect(fx, fr[3], fw, fr[5], cw, ch, wx, wy)
                        assert got == rr.rect_rule(fx, fr[3], fw, fr[5], cw, ch, wx, wy), (cw, ch, wx, wy, fx, fw)
                        got = pl.utils.region_rect(fr[2], fx, fr[4], fw, cw, ch, wx, wy)
                        assert got == rr.rect_rule(fr[2], fx, fr[4], fw, cw, ch, wx, wy), (cw, ch, wx, wy, fx, fw)
                        x, y, w, h = got
                        if w > 0 and h > 0 and y < ch:
                            assert rr.rect_valid(cw, ch, x, y, w, h, wx, wy), got


# ---- the delegates on the CPU stub host, the engine's new calls replaced by doubles --------------------------------------------------
def _settings(pl, *regions):
    """regions: (fx, fy, fw, fh, "Background" | "Foreground")."""
    return {i: pl.utils.BBoxSettings(True, fx, fy, fw, fh, "", "", mode, 0.2, -1) for i, (fx, fy, fw, fh, mode) in enumerate(regions)}


@pytest.fixture
def regions_wired(wired, option, monkeypatch):
    """(plugin, shared, calls): the engine's rect and blend calls replaced by doubles that record their arguments and compute with the
    restatement; the feather mask of a foreground region is ones."""
    pl, shared = wired
    calls = []

    def add_rect_wrap(weights, x, y, w, h, rect_w=None, scalar=1.0, *, wrap_x, wrap_y):
        calls.append(("add_rect_wrap", x, y, w, h, wrap_x, wrap_y))
        assert rr.rect_valid(weights.shape[-1], weights.shape[-2], x, y, w, h, wrap_x, wrap_y)
        m = weights.view(weights.shape[-2], weights.shape[-1]).numpy()
        rr.weight_map_add_rect(m, x, y, w, h, None if rect_w is None else rect_w.numpy().reshape(h, w), scalar)

    def add_rect(weights, x, y, w, h, rect_w=None, scalar=1.0):
        calls.append(("add_rect", x, y, w, h))

    def gather_rect_wrap(x_in, x, y, w, h, *, wrap_x, wrap_y, out=None):
        calls.append(("gather_rect_wrap", x, y, w, h, wrap_x, wrap_y))
        return torch.from_numpy(rr.gather_rect(x_in.numpy(), x, y, w, h))

    def gather_all_shift(plan, x_in, sx, sy, out=None):
        g = wr.grid(plan.w, plan.h, plan.tile_w, plan.tile_h, plan.overlap, plan.tile_bs, plan.wrap_x, plan.wrap_y)
        return [torch.from_numpy(sr.gather(g, x_in.numpy(), b, sx, sy)) for b in range(len(g.batches))]

    def blend_wrap_regions(plan, method, batch_out, N_, C_, *, regions, grid_w, region_w, sx=0, sy=0, tile_w=None, **kw):
        calls.append(("blend", sx, sy, [(r.x, r.y, r.w, r.h, r.mode) for r in regions], grid_w, region_w, tile_w, len(batch_out)))
        return torch.zeros(N_, C_, plan.h, plan.w)

    def refused(*a, **k):
        raise AssertionError("a plain region call was made with --mdtile-wrap-regions active")

    monkeypatch.setattr(pl.engine, "weight_map_add_rect_wrap", add_rect_wrap)
    monkeypatch.setattr(pl.engine, "weight_map_add_rect", add_rect)
    monkeypatch.setattr(pl.engine, "gather_rect_wrap", gather_rect_wrap)
    monkeypatch.setattr(pl.engine, "gather_rect", refused)
    monkeypatch.setattr(pl.engine, "gather_all_shift", gather_all_shift)
    monkeypatch.setattr(pl.engine, "gather_all", lambda plan, x_in, out=None: gather_all_shift(plan, x_in, 0, 0))
    monkeypatch.setattr(pl.engine, "blend_wrap_regions", blend_wrap_regions)
    monkeypatch.setattr(pl.engine, "blend", refused)
    monkeypatch.setattr(pl.engine, "blend_shift", refused)
    monkeypatch.setattr(pl.engine, "reciprocal", lambda t: 1.0 / t)
    monkeypatch.setattr(pl.engine, "rect_mul_canvas", refused)
    monkeypatch.setattr(pl.utils, "feather_mask", lambda w, h, ratio: torch.ones(h, w))
    monkeypatch.setattr(shared.state, "sampling_step", 0)
    return pl, shared, calls


def test_refusal_is_unchanged_without_the_option(regions_wired):
    pl, shared, calls = regions_wired
    shared.cmd_opts.mdtile_wrap_x = True
    d, _ = delegate(pl, W, H, TILE, TILE, OV, BS)
    with pytest.raises(RuntimeError, match="mdtile-wrap-x.*custom regions.*no region path.*--mdtile-wrap-regions"):
        d.init_custom_bbox(_settings(pl, (0.9, 0.1, 0.6, 0.4, "Background")), True, False)
    assert not d.enable_custom_bbox and not d.custom_bboxes and not d.wrap_regions and not calls
    d.enable_custom_bbox = True
    with pytest.raises(RuntimeError, match="mdtile-wrap-x.*custom regions"):
        d.init_done()


def test_ignored_with_one_line_when_no_axis_wraps(regions_wired, capsys):
    pl, shared, calls = regions_wired
    shared.cmd_opts.mdtile_wrap_regions = True
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    capsys.readouterr()
    d.init_custom_bbox(_settings(pl, (0.9, 0.1, 0.6, 0.4, "Background")), True, False)
    out = capsys.readouterr().out
    assert out.count("[Tiled Diffusion]") == 1 and "--mdtile-wrap-regions ignored" in out and "wraps" in out
    assert d.enable_custom_bbox and not d.wrap_regions and d.region_w is None and (d.wrap_ext, d.wrap_ext_y) == (0, 0)
    b = d.custom_bboxes[0]
    assert (b.x, b.y, b.w, b.h) == (36, 2, 4, 10), "the plain rule clips at the edge"
    assert calls == [("add_rect", 36, 2, 4, 10)]
    assert "Tiled Diffusion wrap regions" not in (getattr(p, "extra_generation_params", None) or {})
    # a tile as wide as the canvas drops wrap-x, and the option with it
    shared.cmd_opts.mdtile_wrap_x = True
    d, p = delegate(pl, W, H, 48, 48, OV, BS)
    capsys.readouterr()
    d.init_custom_bbox(_settings(pl, (0.9, 0.1, 0.6, 0.4, "Background")), True, False)
    assert "--mdtile-wrap-regions ignored" in capsys.readouterr().out and not d.wrap_regions


@pytest.mark.parametrize("method", ["md", "mod"])
def test_regions_are_laid_on_the_circle(regions_wired, method):
    pl, shared, calls = regions_wired
    shared.cmd_opts.mdtile_wrap_x = shared.cmd_opts.mdtile_wrap_regions = True
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS, method)
    grid_map = d.weights.clone()
    d.init_custom_bbox(_settings(pl, (0.9, 0.5, 0.6, 0.75, "Background"), (0.95, 0.1, 0.2, 0.2, "Foreground"), (0.1, 0.1, 0.2, 0.2, "Background")), True, False)
    assert d.wrap_regions and p.extra_generation_params["Tiled Diffusion wrap regions"] is True
    assert [(b.x, b.y, b.w, b.h) for b in d.custom_bboxes] == [(36, 12, 24, 12), (38, 2, 8, 5), (4, 2, 8, 5)]      # wrap-x only: y stays clipped
    assert [c for c in calls if c[0].startswith("add_rect")] == [("add_rect_wrap", 36, 12, 24, 12, True, False), ("add_rect_wrap", 4, 2, 8, 5, True, False)]
    assert torch.equal(d.weights, grid_map), "self.weights stays the grid's map"
    want = np.zeros((H, W), np.float32)
    for (x, y, w, h) in ((36, 12, 24, 12), (4, 2, 8, 5)):
        rr.weight_map_add_rect(want, x, y, w, h, None if method == "md" else np.ones((h, w), np.float32))
    assert np.array_equal(d.region_w.numpy()[0, 0], want) and want[12, 0] == 1 and want[12, 19] == 1 and want[12, 20] == 0
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    d.update_pbar = lambda: None
    assert d.total_bboxes == d.num_batches + 3


def test_extended_copies_cover_the_largest_region_overhang(regions_wired):
    """The tile overhang of this plan is 16 columns; a region at x = 36 of width 24 hangs over by 20, and on the torus one at y = 30 of height 16
    by 6 < the tiles' 16: each axis takes its larger one, at every scale."""
    pl, shared, calls = regions_wired
    shared.cmd_opts.mdtile_wrap_x = shared.cmd_opts.mdtile_wrap_regions = True
    d, _ = delegate(pl, W, H, TILE, TILE, OV, BS)
    assert (d.wrap_ext, d.wrap_ext_y) == (16, 0)
    d.init_custom_bbox(_settings(pl, (0.9, 0.5, 0.6, 0.5, "Background"), (0.1, 0.1, 0.2, 0.2, "Background")), True, False)
    assert (d.wrap_ext, d.wrap_ext_y) == (20, 0)
    torch.manual_seed(0)
    icond = torch.randn(N, 5, H, W)
    assert tuple(d.extended_x(icond, "icond").shape) == (N, 5, H, W + 20)
    for b in d.custom_bboxes:
        assert np.array_equal(d.slice_icond(icond, b).numpy(), _take(icond, (b.x, b.y, b.w, b.h)))
    # ControlNet hints (8 x the latent grid) and the StableSR latent follow the region across the seam
    hint = torch.randn(1, 3, H * 8, W * 8)
    param = SimpleNamespace(hint_cond=hint)
    d.enable_controlnet, d.control_params, d.org_control_tensor_batch = True, [param], [hint]
    model = SimpleNamespace(latent_image=None)
    d.enable_stablesr, d.stablesr_script, d.stablesr_tensor = True, SimpleNamespace(stablesr_model=model), icond
    pl.engine.gather_rect = lambda t, x, y, w, h: t[:, :, y:y + h, x:x + w]
    b = d.custom_bboxes[0]
    d.set_custom_controlnet_tensors(0, 2)
    assert tuple(d.extended_x(hint, "hint0", 8).shape) == (1, 3, H * 8, (W + 20) * 8)
    assert np.array_equal(param.hint_cond.numpy(), np.concatenate([_take(hint, (b.x, b.y, b.w, b.h), 8)] * 2, axis=0))
    d.set_custom_stablesr_tensors(0)
    assert np.array_equal(model.latent_image.numpy(), _take(icond, (b.x, b.y, b.w, b.h)))
    # the torus: rows too
    shared.cmd_opts.mdtile_wrap_y = True
    d, _ = delegate(pl, 40, 40, 24, 24, 16, BS)
    assert (d.wrap_ext, d.wrap_ext_y) == (16, 16)
    d.init_custom_bbox(_settings(pl, (0.9, 0.75, 0.6, 0.4, "Background")), True, False)
    b = d.custom_bboxes[0]
    assert (b.x, b.y, b.w, b.h) == (36, 30, 24, 16) and (d.wrap_ext, d.wrap_ext_y) == (20, 16)
    icond = torch.randn(N, 5, 40, 40)
    assert np.array_equal(d.slice_icond(icond, b).numpy(), _take(icond, (36, 30, 24, 16)))


def _evaluate(d, shared, method, x):
    seen = []
    if method == "md":
        def custom(xt, bbox_id, bbox):
            seen.append((bbox_id, xt.clone()))
            return xt
        return d.sample_one_step(x, None, lambda xt, bboxes: xt, custom), seen

    def custom(xt, t_in, c_in, bbox_id, bbox):
        seen.append((bbox_id, xt.clone()))
        return xt
    d.custom_apply_model = custom
    shared.sd_model.apply_model_original_md = lambda x_, t_, c_: x_
    cond = {"c_crossattn": [torch.zeros(N, 77, 8)], "c_concat": [torch.zeros(N, 5, 1, 1)]}
    return d.apply_model_hijack(x, torch.zeros(N), cond), seen


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("method", ["md", "mod"])
def test_every_evaluation_ends_in_the_region_blend(regions_wired, method, shift):
    pl, shared, calls = regions_wired
    shared.cmd_opts.mdtile_wrap_x = shared.cmd_opts.mdtile_wrap_regions = True
    if shift:
        shared.cmd_opts.mdtile_grid_shift = True
    seed = 1234567
    d, p = delegate(pl, 37, 22, 16, 12, 6, 4, method)
    p.all_seeds = [seed]
    d.init_custom_bbox(_settings(pl, (0.9, 0.5, 0.4, 0.3, "Background"), (0.95, 0.1, 0.2, 0.2, "Foreground")), True, False)
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    d.update_pbar = lambda: None
    boxes = [(b.x, b.y, b.w, b.h) for b in d.custom_bboxes]
    assert boxes[0][0] + boxes[0][2] > 37 and boxes[1][0] + boxes[1][2] > 37, "both regions cross the seam"
    torch.manual_seed(1)
    x = torch.randn(N, C, 22, 37)
    for step in range(2):
        shared.state.sampling_step = step
        del calls[:]
        out, seen = _evaluate(d, shared, method, x)
        blends = [c for c in calls if c[0] == "blend"]
        assert len(blends) == 1 and out is d.x_buffer
        _, sx, sy, regions, grid_w, region_w, tile_w, nb = blends[0]
        assert (sx, sy) == ((sr.PINNED[(seed, step, 0, 37)], 0) if shift else (0, 0))
        assert regions == [boxes[0] + (pl.engine.REGION_BG,), boxes[1] + (pl.engine.REGION_FG,)]
        assert grid_w is d.weights and region_w is d.region_w and nb == d.num_batches
        assert (tile_w is None) == (method == "md")
        assert [i for i, _ in seen] == [0, 1]
        for (i, xt), box in zip(seen, boxes):
            assert np.array_equal(xt.numpy(), _take(x, box)), "the region's tile is the wrapped cut of x_in"
    if method == "mod":
        assert all(w is None or tuple(w.shape[-2:]) == (b[3], b[2]) for w, b in zip(d.custom_weights, boxes)), "raw region weights"


@pytest.mark.parametrize("method", ["md", "mod"])
def test_noise_inversion_evaluates_at_rest(regions_wired, method, capsys):
    pl, shared, calls = regions_wired
    shared.cmd_opts.mdtile_wrap_x = shared.cmd_opts.mdtile_wrap_regions = shared.cmd_opts.mdtile_grid_shift = True
    d, p = delegate(pl, 37, 22, 16, 12, 6, 4, method)
    p.all_seeds = [1234567]
    d.init_custom_bbox(_settings(pl, (0.9, 0.5, 0.4, 0.3, "Background")), True, False)
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    d.update_pbar = lambda: None
    d.custom_bboxes[0].cond = None
    shared.state.sampling_step = 1
    cond = {"c_crossattn": [torch.zeros(N, 77, 8)], "c_concat": [torch.zeros(N, 5, 1, 1)]}
    pl.utils.Condition.reconstruct_cond = staticmethod(lambda c, step: torch.zeros(N, 77, 8))
    shared.sd_model.apply_model = lambda x_, t_, cond: x_
    shared.sd_model.apply_model_original_md = lambda x_, t_, c_: x_
    d.get_noise(torch.zeros(N, C, 22, 37), torch.zeros(N), cond, 0)
    blends = [c for c in calls if c[0] == "blend"]
    assert len(blends) == 1 and blends[0][1:3] == (0, 0)
    assert "--mdtile-grid-shift not applied" in capsys.readouterr().out


def test_renoise_with_regions_only_is_refused_at_set_up(regions_wired):
    pl, shared, calls = regions_wired
    shared.cmd_opts.mdtile_wrap_x = shared.cmd_opts.mdtile_wrap_regions = True
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    d.noise_inverse_enabled, d.noise_inverse_renoise_strength = True, 1.0
    d.init_custom_bbox(_settings(pl, (0.9, 0.5, 0.6, 0.5, "Background")), False, False)      # no background: the grid is switched off
    assert d.wrap_regions and not d.enable_grid_bbox and float(d.weights.abs().sum()) == 0.0
    with pytest.raises(RuntimeError, match="--mdtile-wrap-regions.*Noise Inversion's renoise composite"):
        d.init_done()
    d.noise_inverse_renoise_strength = 0.0
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()


def test_region_noise_follows_the_delegate(regions_wired, monkeypatch):
    """create_random_tensors_hijack lays each region's noise with the same rule as the delegate, and calls the wrapped paste only then."""
    pl, shared, calls = regions_wired
    seen = []
    monkeypatch.setattr(pl.engine, "region_noise_wrap", lambda noise, regions, *, wrap_x, wrap_y: seen.append(("wrap", [r[:5] for r in regions], wrap_x, wrap_y)))
    monkeypatch.setattr(pl.engine, "region_noise", lambda noise, regions: seen.append(("plain", [r[:5] for r in regions])))
    S = pl.tilediffusion.Script
    monkeypatch.setattr(S, "create_random_tensors_original_md", staticmethod(lambda shape, *a, **k: torch.zeros((1,) + tuple(shape))), raising=False)
    s = S()
    settings = _settings(pl, (0.9, 0.5, 0.6, 0.75, "Background"))
    BG = pl.engine.REGION_BG
    s.delegate = SimpleNamespace(wrap_x=True, wrap_y=False, wrap_regions=True)
    s.create_random_tensors_hijack(settings, {}, (4, H, W), [1])
    s.delegate = SimpleNamespace(wrap_x=True, wrap_y=False, wrap_regions=False)
    s.create_random_tensors_hijack(settings, {}, (4, H, W), [1])
    s.delegate = None
    s.create_random_tensors_hijack(settings, {}, (4, H, W), [1])
    assert seen == [("wrap", [(36, 12, 24, 12, BG)], True, False), ("plain", [(36, 12, 4, 12, BG)]), ("plain", [(36, 12, 4, 12, BG)])]


# ---- the restatement against itself ------------------------------------------------------------------------------------------------
def _inputs(g, seed=5):
    rng = np.random.default_rng(seed)
    tiles = rng.standard_normal((len(g.boxes) * N, C, g.th, g.tw)).astype(np.float32)
    return rng, tiles


def _regions(rng, g, method, spec):
    out = []
    for (x, y, w, h, mode) in spec:
        weight = rng.random((h, w)).astype(np.float32) if mode == "fg" else (wr.gaussian(w, h) if method == "mod" else None)
        out.append(rr.Region(x, y, w, h, mode, rng.standard_normal((N, C, h, w)).astype(np.float32), weight))
    return out


@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("case", ["torus_odd", "ring_y", "order40"])
def test_without_regions_it_is_the_shifted_blend(case, method):
    g = wr.case_grid(case)
    _, _, _, _, _, wx, wy, _ = wr.CASES[case]
    _, tiles = _inputs(g)
    tw = wr.gaussian(g.tw, g.th) if method == "mod" else None
    gmap = wr.weight_map(g, tw)
    zeros = np.zeros((g.H, g.W), np.float32)
    with np.errstate(all="ignore"):
        rescale = (np.float32(1.0) / gmap).astype(np.float32)
    for (sx, sy) in ((0, 0), (5 if wx else 0, 3 if wy else 0), ((g.W - 1) if wx else 0, (g.H - 1) if wy else 0)):
        got = rr.blend(g, method, tiles, N, C, sx, sy, gmap, zeros, [], tw)
        want = sr.blend(g, method, tiles, N, sx, sy, gmap, tw, rescale)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (case, method, sx, sy)


@pytest.mark.parametrize("method", ["md", "mod"])
def test_with_regions_it_commutes_with_rolling_the_canvas(method):
    """The tiles' placement and the region origins rolled by (a, b), at shift (sx + a, sy + b): the rolled result, bit for bit -- tile and region
    list order do not change with the roll."""
    g = wr.case_grid("torus_odd")
    rng, tiles = _inputs(g)
    tw = wr.gaussian(g.tw, g.th) if method == "mod" else None
    gmap = wr.weight_map(g, tw)
    spec = [(30, 4, 12, 8, "bg"), (33, 18, 9, 9, "fg"), (2, 2, 10, 6, "bg"), (6, 4, 10, 6, "bg"), (35, 20, 6, 5, "fg"), (0, 10, 37, 3, "fg"), (36, 21, 1, 1, "bg")]
    regions = _regions(rng, g, method, spec)
    for (sx, sy) in ((0, 0), (5, 3)):
        base = rr.blend(g, method, tiles, N, C, sx, sy, gmap, rr.region_w_map(g.W, g.H, method, regions), regions, tw)
        assert np.isfinite(base).all()
        for (a, b) in ((1, 0), (7, 5), (36, 21)):
            moved = rr.rolled(regions, a, b, g.W, g.H)
            got = rr.blend(g, method, tiles, N, C, (sx + a) % g.W, (sy + b) % g.H, gmap, rr.region_w_map(g.W, g.H, method, moved), moved, tw)
            want = np.roll(base, (b, a), axis=(-2, -1))
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (method, sx, sy, a, b)


def test_regions_only_leave_uncovered_pixels_at_zero():
    g = wr.case_grid("torus_odd")
    rng = np.random.default_rng(2)
    for method in ("md", "mod"):
        regions = _regions(rng, g, method, [(30, 18, 12, 8, "bg"), (33, 20, 9, 9, "fg")])
        out = rr.blend(g, method, None, N, C, 0, 0, None, rr.region_w_map(g.W, g.H, method, regions), regions)
        assert np.isfinite(out).all() and (out[:, :, 10, 10] == 0).all() and (out[:, :, 0, 0] != 0).all()
