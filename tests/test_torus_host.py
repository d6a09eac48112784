"""Vertical wrap-around and the torus without a GPU: the plan of mdtile_plan_create_wrap against the numpy restatement
tests/wrap_ref.py, its refusals, the --mdtile-wrap-y option, the script wiring on the stub host (plan choice, per-axis fallback, the region
refusal, infotext, the extended copy's rows and corner) and the Tiled VAE hook's pad-and-crop in y on the torch doubles of the engine."""
import argparse
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUGIN = os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd")
for _p in (ROOT, PLUGIN, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from hostsim import stub_host as sh      # noqa: E402
import wrap_ref as tr                    # noqa: E402
from wrap_common import (host, wired, delegate as _delegate, load_preload, take as _take, cpu_vae_hook as _hook,      # noqa: E402,F401
                         pad_rows as _pad_rows, pad_cols as _pad_cols)


# ---- plan --------------------------------------------------------------------------------------------------------------------
def _raw(E, handle):
    """(info8, boxes, wrap_x, wrap_y) of a raw plan handle; the handle is destroyed."""
    L = E.lib()
    info = (ctypes.c_int * 8)()
    assert L.mdtile_plan_info(handle, info) == 0
    buf = (ctypes.c_int * (4 * info[2]))()
    assert L.mdtile_plan_bboxes(handle, buf) == 0
    flat = list(buf)
    out = (list(info), [tuple(flat[4 * i:4 * i + 4]) for i in range(info[2])], L.mdtile_plan_wrap_x(handle), L.mdtile_plan_wrap_y(handle))
    L.mdtile_plan_destroy(handle)
    return out


def _cover(origins, tile, extent):
    n = np.zeros(extent, int)
    for o in origins:
        n[(o + np.arange(tile)) % extent] += 1
    return n


@pytest.mark.parametrize("case", list(tr.CASES))
def test_plan_matches_the_restatement(built_lib, case):
    E = built_lib
    W, H, tw, th, ov, wx, wy, bs = tr.CASES[case]
    g = tr.case_grid(case)
    plan = E.Plan(W, H, tw, th, ov, bs, wrap_x=bool(wx), wrap_y=bool(wy))
    assert (plan.wrap_x, plan.wrap_y) == (bool(wx), bool(wy))
    assert (E.lib().mdtile_plan_wrap_x(plan.handle), E.lib().mdtile_plan_wrap_y(plan.handle)) == (wx, wy)
    assert (plan.cols, plan.rows, plan.num_tiles, plan.tile_w, plan.tile_h, plan.overlap) == (g.cols, g.rows, len(g.boxes), g.tw, g.th, g.ov)
    assert plan.bboxes == list(g.boxes)                      # row-major, y outer; a box reports y_r, so y_r + th may pass H
    assert (plan.tile_bs, plan.num_batches) == (g.tile_bs, len(g.batches))
    assert [len(b) for b in plan.batches] == [len(b) for b in g.batches]
    assert plan.num_batches <= E.MAX_BATCHES, "the case must stay under MDTILE_MAX_BATCHES: a wrap plan has no packed form"
    # every row is covered, no tile covers a row twice, cyclic neighbours overlap by at least ov, the seam (last -> first) included
    assert max(y + g.th for y in g.ys) > H, "no tile spans the seam in y"
    assert _cover(g.ys, g.th, H).min() >= 1 and g.th < H
    for r in range(g.rows):
        stride = (g.ys[(r + 1) % g.rows] - g.ys[r]) % H
        assert 0 < stride <= g.th - g.ov, (r, stride)
    if wx:
        assert max(x + g.tw for x in g.xs) > W and _cover(g.xs, g.tw, W).min() >= 1
    else:
        assert list(g.xs) == tr.plain_origins(W, g.tw, g.ov) and max(x + g.tw for x in g.xs) == W


def test_the_cases_are_what_the_issue_lists():
    """Origins and coverage counts of the GPU cases, as computed on the CPU for the issue."""
    g = tr.case_grid("torus_odd")
    assert g.xs == (0, 9, 18, 27) and g.ys == (0, 5, 11, 16)
    m = tr.weight_map(g)
    assert (m.min(), m.max()) == (2, 6) and g.W % 4 and g.H % 4
    g = tr.case_grid("ring_y")
    assert g.xs == (0, 10, 20) and g.ys == (0, 5, 10, 16, 21)
    g = tr.case_grid("order40")
    assert g.xs == g.ys == (0, 8, 16, 24, 32) and (tr.weight_map(g) == 9).all()
    assert [r for r in range(g.rows) if (0 - g.ys[r]) % g.H < g.th] == [0, 3, 4], "at the seam list order (0, 3, 4) is not circle order (3, 4, 0)"
    g = tr.case_grid("aligned64")
    assert all(v % 4 == 0 for v in g.xs + g.ys) and (tr.weight_map(g) == 4).all()
    g = tr.case_grid("dense50")
    m = tr.weight_map(g)
    assert (g.cols, g.rows) == (13, 13) and (m.min(), m.max()) == (144, 169)
    g = tr.case_grid("rect44")
    m = tr.weight_map(g)
    assert g.tw != g.th and (m.min(), m.max()) == (1, 4)


@pytest.mark.parametrize("geom", [(37, 20, 16, 12, 6, 4), (64, 16, 32, 32, 8, 2), (50, 12, 48, 48, 44, 4), (1024, 1024, 128, 128, 8, 8)],
                         ids=lambda g: "x".join(map(str, g)))
def test_wrap_x_alone_is_the_wrap_x_plan(built_lib, geom):
    """(wrap_x, wrap_y) = (1, 0): exactly what mdtile_plan_create_wrap_x produces, and what the restatements agree on."""
    E = built_lib
    L = E.lib()
    a = _raw(E, L.mdtile_plan_create_wrap(*geom, 1, 0))
    b = _raw(E, L.mdtile_plan_create_wrap_x(*geom))
    assert a == b and a[2:] == (1, 0)
    g = tr.grid(*geom, True, False)
    assert g == tr.grid(*geom) and a[1] == list(g.boxes)
    plan = E.Plan(*geom, wrap_x=True)
    assert plan.wrap_x and not plan.wrap_y and plan.bboxes == a[1]
    plain = E.Plan(*geom)
    assert not plain.wrap_x and not plain.wrap_y and L.mdtile_plan_wrap_y(plain.handle) == 0


def test_plan_refusals(built_lib):
    E = built_lib
    L = E.lib()
    # neither axis: the text points to the plain entry
    assert tr.grid(96, 64, 32, 32, 8, 4, False, False) is None
    assert L.mdtile_plan_create_wrap(96, 64, 32, 32, 8, 4, 0, 0) is None
    assert b"mdtile_plan_create" in L.mdtile_last_error() and b"neither" in L.mdtile_last_error()
    # a tile as large as the canvas on a wrapped axis: the text names the axis
    for tile_h in (64, 96):
        assert tr.grid(96, 64, 32, tile_h, 8, 4, False, True) is None
        assert L.mdtile_plan_create_wrap(96, 64, 32, tile_h, 8, 4, 0, 1) is None
        assert b"y axis" in L.mdtile_last_error() and b"meet itself" in L.mdtile_last_error()
        with pytest.raises(E.MdtileError, match="y axis"):
            E.Plan(96, 64, 32, tile_h, 8, 4, wrap_y=True)
        with pytest.raises(E.MdtileError, match="y axis"):
            E.Plan(96, 64, 32, tile_h, 8, 4, wrap_x=True, wrap_y=True)
    assert tr.grid(96, 64, 96, 32, 8, 4, True, True) is None
    assert L.mdtile_plan_create_wrap(96, 64, 96, 32, 8, 4, 1, 1) is None
    assert b"x axis" in L.mdtile_last_error() and b"meet itself" in L.mdtile_last_error()
    with pytest.raises(E.MdtileError, match="x axis"):
        E.Plan(96, 64, 128, 32, 8, 4, wrap_x=True, wrap_y=True)
    # ... but a tile as wide as the canvas is fine on an axis that does not wrap
    ring = E.Plan(96, 64, 96, 32, 8, 4, wrap_y=True)
    assert ring.cols == 1 and ring.bboxes == list(tr.grid(96, 64, 96, 32, 8, 4, False, True).boxes)
    # overlap equal to the tile (the overlap clamps to min(requested tiles) - 4 = 12 = the canvas-clamped tile width)
    assert L.mdtile_plan_create_wrap(12, 64, 16, 16, 12, 4, 0, 1) is None
    assert b"overlap" in L.mdtile_last_error()
    assert L.mdtile_plan_create_wrap(64, 64, 16, 0, 4, 4, 1, 1) is None and b"bad arguments" in L.mdtile_last_error()
    with pytest.raises(E.MdtileError, match="clamp"):
        E.Plan(200, 200, 96, 96, 48, 4, clamp=False, wrap_y=True)
    assert L.mdtile_plan_wrap_y(None) == 0


# ---- the option --------------------------------------------------------------------------------------------------------------
def test_preload_option(host):
    pl, shared = host
    parser = argparse.ArgumentParser()
    load_preload().preload(parser)
    assert parser.parse_args([]).mdtile_wrap_y is False
    ns = parser.parse_args(["--mdtile-wrap-y"])
    assert ns.mdtile_wrap_y is True and ns.mdtile_wrap_x is False
    ns = parser.parse_args(["--mdtile-wrap-x", "--mdtile-wrap-y"])
    assert ns.mdtile_wrap_y is True and ns.mdtile_wrap_x is True
    A = pl.abstractdiffusion.AbstractDiffusion
    assert not hasattr(shared.cmd_opts, "mdtile_wrap_y") and A.wrap_y_requested() is False      # a host that never heard of the option
    assert pl.tilevae._cmd_line_wrap_y() is False
    shared.cmd_opts.mdtile_wrap_y = True
    assert A.wrap_y_requested() is True and pl.tilevae._cmd_line_wrap_y() is True
    assert A.wrap_x_requested() is False and pl.tilevae._cmd_line_wrap_x() is False
    shared.cmd_opts.mdtile_wrap_y = False
    assert A.wrap_y_requested() is False and pl.tilevae._cmd_line_wrap_y() is False


# ---- script wiring -----------------------------------------------------------------------------------------------------------
def _info(p):
    return getattr(p, "extra_generation_params", None) or {}


def test_plan_choice_infotext_and_fallback(wired, capsys):
    pl, shared = wired
    # without the options: today's plan, no key
    d, p = _delegate(pl, 40, 40, 24, 24, 16)
    assert not d.plan.wrap_y and d.wrap_ext_y == 0 and "Tiled Diffusion wrap y" not in _info(p)
    assert d.plan.bboxes == pl.engine.Plan(40, 40, 24, 24, 16, 4).bboxes
    # wrap-y alone: plain columns, cyclic rows
    shared.cmd_opts.mdtile_wrap_y = True
    d, p = _delegate(pl, 40, 40, 24, 24, 16)
    g = tr.grid(40, 40, 24, 24, 16, 4, False, True)
    assert d.wrap_y and not d.wrap_x and d.plan.wrap_y and not d.plan.wrap_x and d.plan.bboxes == list(g.boxes)
    assert _info(p)["Tiled Diffusion wrap y"] is True and "Tiled Diffusion wrap x" not in _info(p)
    assert d.wrap_ext == 0 and d.wrap_ext_y == max(g.ys) + g.th - g.H == 16
    # both: the torus
    shared.cmd_opts.mdtile_wrap_x = True
    d, p = _delegate(pl, 40, 40, 24, 24, 16)
    g = tr.grid(40, 40, 24, 24, 16, 4, True, True)
    assert d.plan.wrap_x and d.plan.wrap_y and d.plan.bboxes == list(g.boxes)
    assert _info(p)["Tiled Diffusion wrap y"] is True and _info(p)["Tiled Diffusion wrap x"] is True
    assert (d.wrap_ext, d.wrap_ext_y) == (16, 16)
    assert [[(b.x, b.y, b.w, b.h) for b in batch] for batch in d.batched_bboxes] == [[g.boxes[t] for t in batch] for batch in g.batches]
    assert "[Tiled Diffusion]" not in capsys.readouterr().out
    # a tile as tall as the canvas: one line, wrap-y dropped, wrap-x stays
    d, p = _delegate(pl, 40, 24, 24, 24, 16)
    out = capsys.readouterr().out
    assert out.count("[Tiled Diffusion]") == 1 and "wrap-y" in out and "wrap-x" not in out
    assert d.wrap_x and not d.wrap_y and d.wrap_ext_y == 0 and d.plan.bboxes == list(tr.grid(40, 24, 24, 24, 16, 4).boxes)
    assert _info(p)["Tiled Diffusion wrap x"] is True and "Tiled Diffusion wrap y" not in _info(p)
    # ... and the other way round: a tile as wide as the canvas drops wrap-x only
    d, p = _delegate(pl, 24, 40, 24, 24, 16)
    out = capsys.readouterr().out
    assert out.count("[Tiled Diffusion]") == 1 and "wrap-x" in out and "wrap-y" not in out
    assert d.wrap_y and not d.wrap_x and d.plan.bboxes == list(tr.grid(24, 40, 24, 24, 16, 4, False, True).boxes)
    # both too large: two lines, the plain plan
    d, p = _delegate(pl, 24, 24, 24, 24, 16)
    assert capsys.readouterr().out.count("[Tiled Diffusion]") == 2
    assert not d.wrap_x and not d.wrap_y and d.plan.bboxes == pl.engine.Plan(24, 24, 24, 24, 16, 4).bboxes
    assert "Tiled Diffusion wrap y" not in _info(p) and "Tiled Diffusion wrap x" not in _info(p)


def test_torus_plan_through_the_script(wired):
    """Script.process + the sampler hijack build the delegate: with both options its plan is the torus plan and the infotext says so."""
    pl, shared = wired
    import modules.sd_samplers as sd_samplers
    shared.cmd_opts.mdtile_wrap_x = shared.cmd_opts.mdtile_wrap_y = True
    s = pl.tilediffusion.Script()
    p = sh.make_processing(2048, 1024)
    p.extra_generation_params = {}
    defaults = list(pl.utils.DEFAULT_BBOX_SETTINGS) * 8
    s.process(p, True, "MultiDiffusion", False, True, 1024, 1024, 96, 96, 48, 4, "None", 2.0, False, 10, 1, 1, 64, False, False, False, False, *defaults)
    try:
        sd_samplers.create_sampler("Euler", None)
        g = tr.grid(256, 128, 96, 96, 48, 4, True, True)
        assert s.delegate.plan.wrap_x and s.delegate.plan.wrap_y and s.delegate.plan.bboxes == list(g.boxes)
        assert p.extra_generation_params["Tiled Diffusion wrap y"] is True and p.extra_generation_params["Tiled Diffusion wrap x"] is True
    finally:
        if s.delegate is not None and s.delegate.pbar is not None:
            s.delegate.pbar.close()
        s.postprocess(p, None, True)


def test_regions_are_refused(wired):
    pl, shared = wired
    shared.cmd_opts.mdtile_wrap_y = True
    d, _ = _delegate(pl, 40, 40, 24, 24, 16)
    U = pl.utils
    settings = {0: U.BBoxSettings(True, 0.1, 0.1, 0.4, 0.4, "", "", "Background", 0.2, -1)}
    with pytest.raises(RuntimeError, match="mdtile-wrap-y.*custom regions"):
        d.init_custom_bbox(settings, True, False)
    assert not d.enable_custom_bbox and not d.custom_bboxes
    d.enable_custom_bbox = True                      # armed behind init_custom_bbox's back: init_done still refuses
    with pytest.raises(RuntimeError, match="mdtile-wrap-y.*custom regions"):
        d.init_done()
    shared.cmd_opts.mdtile_wrap_x = True             # the torus names both options
    d, _ = _delegate(pl, 40, 40, 24, 24, 16)
    with pytest.raises(RuntimeError, match="mdtile-wrap-x / --mdtile-wrap-y.*custom regions"):
        d.init_custom_bbox(settings, True, False)


def test_extended_copy_gains_rows_after_columns(wired):
    """cat(cat(t, t[..., :E]), that[..., :Ey, :]): the rows past the bottom edge are the first rows again, and the corner block -- past both
    edges -- is the source's top-left corner."""
    pl, shared = wired
    shared.cmd_opts.mdtile_wrap_x = shared.cmd_opts.mdtile_wrap_y = True
    d, _ = _delegate(pl, 40, 32, 24, 16, 8, bs=2)
    g = tr.grid(40, 32, 24, 16, 8, 2, True, True)
    E, Ey = d.wrap_ext, d.wrap_ext_y
    assert (E, Ey) == (max(g.xs) + g.tw - 40, max(g.ys) + g.th - 32) and E > 0 and Ey > 0 and E != Ey
    torch.manual_seed(0)
    t = torch.randn(2, 5, 32, 40)
    ext = d.extended_x(t, "icond")
    assert tuple(ext.shape) == (2, 5, 32 + Ey, 40 + E) and ext.is_contiguous()
    assert torch.equal(ext[..., :32, :40], t) and torch.equal(ext[..., :32, 40:], t[..., :, :E])
    assert torch.equal(ext[..., 32:, :40], t[..., :Ey, :]) and torch.equal(ext[..., 32:, 40:], t[..., :Ey, :E]), "the corner block"
    assert d.extended_x(t, "icond") is ext, "built once per source tensor"
    t.add_(1.0)
    assert d.extended_x(t, "icond") is not ext
    hint = torch.randn(1, 3, 32 * 8, 40 * 8)
    assert tuple(d.extended_x(hint, "hint0", 8).shape[-2:]) == ((32 + Ey) * 8, (40 + E) * 8)
    # wrap-y alone: rows only
    del shared.cmd_opts.mdtile_wrap_x
    d, _ = _delegate(pl, 40, 32, 24, 16, 8, bs=2)
    ext = d.extended_x(t, "icond")
    assert d.wrap_ext == 0 and tuple(ext.shape) == (2, 5, 32 + d.wrap_ext_y, 40) and torch.equal(ext[..., 32:, :], t[..., :d.wrap_ext_y, :])
    # neither: the tensor itself
    del shared.cmd_opts.mdtile_wrap_y
    d, _ = _delegate(pl, 40, 32, 24, 16, 8, bs=2)
    assert d.extended_x(t, "icond") is t


@pytest.mark.parametrize("method", ["md", "mod"])
def test_icond_slices_of_seam_tiles(wired, method):
    """img2img's image conditioning follows the tiles across both seams: equal to the source indexed mod its size."""
    pl, shared = wired
    shared.cmd_opts.mdtile_wrap_x = shared.cmd_opts.mdtile_wrap_y = True
    d, _ = _delegate(pl, 40, 32, 24, 16, 8, bs=2, method=method)
    g = tr.grid(40, 32, 24, 16, 8, 2, True, True)
    torch.manual_seed(0)
    icond = torch.randn(2, 5, 32, 40)
    cond = {"c_crossattn": [torch.zeros(2, 77, 8)], "c_concat": [icond]}
    both = [b for batch in d.batched_bboxes for b in batch if b.x + b.w > 40 and b.y + b.h > 32]
    assert len(both) == 1, "one tile spans both seams"
    for batch, idx in zip(d.batched_bboxes, g.batches):
        want = np.concatenate([_take(icond, g.boxes[t]) for t in idx], axis=0)
        if method == "md":
            got = d.get_icond(d.repeat_cond_dict(cond, batch))
        else:
            got = torch.cat([d.slice_icond(d.get_icond(cond), b) for b in batch], dim=0)
        assert got.shape == want.shape and np.array_equal(got.numpy(), want)


@pytest.mark.parametrize("kdiff", [True, False], ids=["kdiff", "ddim"])
def test_controlnet_and_stablesr_slices_of_seam_tiles(wired, kdiff):
    pl, shared = wired
    shared.cmd_opts.mdtile_wrap_x = shared.cmd_opts.mdtile_wrap_y = True
    d, _ = _delegate(pl, 40, 32, 24, 16, 8, bs=2)
    if not kdiff:
        d.sampler_raw = object()
    assert d.is_kdiff == kdiff
    g = tr.grid(40, 32, 24, 16, 8, 2, True, True)
    torch.manual_seed(1)
    hint = torch.randn(1, 3, 32 * 8, 40 * 8)
    param = SimpleNamespace(hint_cond=hint)
    d.enable_controlnet, d.control_params, d.org_control_tensor_batch = True, [param], [hint]
    sr = torch.randn(2, 4, 32, 40)
    model = SimpleNamespace(latent_image=None)
    d.enable_stablesr, d.stablesr_script, d.stablesr_tensor = True, SimpleNamespace(stablesr_model=model), sr
    for batch_id, idx in enumerate(g.batches):
        d.switch_controlnet_tensors(batch_id, 2, len(idx))
        tiles = np.concatenate([_take(hint, g.boxes[t], 8) for t in idx], axis=0)
        want = np.repeat(tiles, 2, axis=0) if kdiff else np.concatenate([tiles] * 4, axis=0)
        assert np.array_equal(param.hint_cond.numpy(), want), batch_id
        d.switch_stablesr_tensors(batch_id)
        want = np.concatenate([_take(sr, g.boxes[t]) for t in idx], axis=0)
        assert np.array_equal(model.latent_image.numpy(), want), batch_id
    d.reset_controlnet_tensors()
    assert param.hint_cond is hint


# ---- Tiled VAE ---------------------------------------------------------------------------------------------------------------
# (decoder?, tile size, input shape): tiled paths, H and W both above two pads
VAE_CASES = [(True, 16, (1, 4, 40, 24)), (False, 64, (1, 3, 200, 136))]


@pytest.mark.parametrize("is_decoder,ts,shape", VAE_CASES, ids=["decoder", "encoder"])
def test_vae_hook_pads_rows_by_its_tile_pad_and_crops(host, is_decoder, ts, shape):
    """wrap-y: the plain hook on the input padded by hand with the other edge's rows, cropped.  Both options: columns first, then rows, so the
    corners of the padded input come from the diagonal neighbour."""
    from hostsim import ldm_decoder as ld
    pl, shared = host
    net = ld.make_decoder(0, small=True) if is_decoder else ld.make_encoder(0, small=True)
    hook = _hook(pl, net, ts, is_decoder)
    P = 11 if is_decoder else 32
    assert hook.pad == P and shape[-2] > 2 * P and shape[-1] > 2 * P
    cut = 8 * P if is_decoder else P // 8
    torch.manual_seed(3)
    z = torch.randn(*shape)
    with torch.no_grad():
        plain = hook(z)
        padded_y = hook(_pad_rows(z, P))
        padded_xy = hook(_pad_rows(_pad_cols(z, P), P))
        shared.cmd_opts.mdtile_wrap_y = True
        got_y = hook(z)
        shared.cmd_opts.mdtile_wrap_x = True
        got_xy = hook(z)
    want_y = padded_y[..., cut:padded_y.shape[-2] - cut, :]
    want_xy = padded_xy[..., cut:padded_xy.shape[-2] - cut, cut:padded_xy.shape[-1] - cut]
    assert got_y.shape == got_xy.shape == plain.shape == want_y.shape == want_xy.shape
    assert torch.equal(got_y, want_y) and not torch.equal(got_y, plain)
    assert torch.equal(got_xy, want_xy) and not torch.equal(got_xy, got_y)
    assert got_y.is_contiguous() and got_xy.is_contiguous()


@pytest.mark.parametrize("is_decoder,ts,shape", [(True, 16, (1, 4, 40, 22)), (False, 64, (1, 3, 200, 64))], ids=["decoder", "encoder"])
def test_vae_hook_axes_decide_independently(host, is_decoder, ts, shape):
    """W = 2 P is too small to pad in x; y is still padded.  And H = 2 P with wrap-y alone acts as today."""
    from hostsim import ldm_decoder as ld
    pl, shared = host
    net = ld.make_decoder(0, small=True) if is_decoder else ld.make_encoder(0, small=True)
    hook = _hook(pl, net, ts, is_decoder)
    P = hook.pad
    assert shape[-1] == 2 * P
    cut = 8 * P if is_decoder else P // 8
    torch.manual_seed(3)
    z = torch.randn(*shape)
    zt = z.transpose(-1, -2).contiguous()            # H = 2 P
    with torch.no_grad():
        padded_y = hook(_pad_rows(z, P))
        plain_t = hook(zt)
        shared.cmd_opts.mdtile_wrap_x = shared.cmd_opts.mdtile_wrap_y = True
        got = hook(z)
        del shared.cmd_opts.mdtile_wrap_x
        got_t = hook(zt)
    assert torch.equal(got, padded_y[..., cut:padded_y.shape[-2] - cut, :])
    assert torch.equal(got_t, plain_t)
