"""Horizontal wrap-around without a GPU: the wrap-x plan of the library against the numpy restatement tests/wrap_ref.py, the
--mdtile-wrap-x option, the script wiring on the stub host (plan choice, fallback, refusals, infotext, the wrap-aware Python slices) and the
Tiled VAE hook's pad-and-crop on the torch doubles of the engine."""
import argparse
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
import wrap_ref as wr                    # noqa: E402
from wrap_common import host, wired, delegate, load_preload, take as _take, cpu_vae_hook as _hook, pad_cols      # noqa: E402,F401

# (W, H, requested tile_w, tile_h, overlap, tile_bs): the GPU cases of tests/test_gpu_wrap.py and a 1024-wide panorama
GEOMETRIES = [(37, 20, 16, 12, 6, 4), (64, 16, 32, 32, 8, 2), (50, 12, 48, 48, 44, 4), (40, 24, 24, 24, 16, 2), (64, 24, 32, 32, 16, 3),
              (1024, 1024, 128, 128, 8, 8)]
# The restatement pinned to literal numbers: geometry -> (xs, ys, min and max of the uniform weight map).  Computed once with the x-only
# restatement this module used before tests/wrap_ref.py took the per-axis form (which then agreed with it bit for bit on weight maps, gather
# and both blends for every geometry below).  The last three rows: the canvases of tests/test_gpu_wrap.py's 2- and 4-plane cases and of the
# script-wiring tests.
FROZEN = {
    (37, 20, 16, 12, 6, 4): ((0, 9, 18, 27), (0, 4, 8), 1, 6),
    (64, 16, 32, 32, 8, 2): ((0, 21, 42), (0,), 1, 2),
    (50, 12, 48, 48, 44, 4): ((0, 3, 7, 11, 15, 19, 23, 26, 30, 34, 38, 42, 46), (0,), 12, 13),
    (40, 24, 24, 24, 16, 2): ((0, 8, 16, 24, 32), (0,), 3, 3),
    (64, 24, 32, 32, 16, 3): ((0, 16, 32, 48), (0,), 2, 2),
    (1024, 1024, 128, 128, 8, 8): ((0, 113, 227, 341, 455, 568, 682, 796, 910), (0, 112, 224, 336, 448, 560, 672, 784, 896), 1, 4),
    (512, 256, 96, 96, 48, 8): ((0, 46, 93, 139, 186, 232, 279, 325, 372, 418, 465), (0, 40, 80, 120, 160), 2, 9),
    (1024, 256, 128, 128, 8, 8): ((0, 113, 227, 341, 455, 568, 682, 796, 910), (0, 64, 128), 1, 4),
    (256, 64, 96, 96, 48, 4): ((0, 42, 85, 128, 170, 213), (0,), 2, 3),
}


# ---- plan --------------------------------------------------------------------------------------------------------------------
def test_the_restatement_is_what_the_x_only_one_gave():
    """Origins and coverage counts of every wrap-x geometry against literal numbers, so that the per-axis restatement is not pinned to itself."""
    assert set(GEOMETRIES) <= set(FROZEN)
    for geom, (xs, ys, lo, hi) in FROZEN.items():
        g = wr.grid(*geom)
        assert g == wr.grid(*geom, True, False) and (g.xs, g.ys) == (xs, ys), geom
        m = wr.weight_map(g)
        assert (m.min(), m.max()) == (lo, hi), geom
        assert max(y + g.th for y in g.ys) == g.H, "plain rows: the last tile row is flush with the bottom edge"


@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_plan_matches_the_restatement(built_lib, geom):
    E = built_lib
    W, H, tw, th, ov, bs = geom
    g = wr.grid(*geom)
    plan = E.Plan(W, H, tw, th, ov, bs, wrap_x=True)
    assert plan.wrap_x and E.lib().mdtile_plan_wrap_x(plan.handle) == 1
    assert (plan.cols, plan.rows, plan.num_tiles, plan.tile_w, plan.tile_h, plan.overlap) == (g.cols, g.rows, len(g.boxes), g.tw, g.th, g.ov)
    assert plan.bboxes == list(g.boxes)
    assert (plan.tile_bs, plan.num_batches) == (g.tile_bs, len(g.batches))
    assert [len(b) for b in plan.batches] == [len(b) for b in g.batches]
    # every column is covered; no tile covers a column twice; cyclic neighbours overlap by at least ov, the seam (last -> first) included
    cover = np.zeros(W, int)
    for x in g.xs:
        cols = wr.columns(g, x)
        assert len(set(cols.tolist())) == g.tw
        cover[cols] += 1
    assert cover.min() >= 1
    for c in range(g.cols):
        stride = (g.xs[(c + 1) % g.cols] - g.xs[c]) % W
        assert 0 < stride <= g.tw - g.ov, (c, stride)
    assert max(x + g.tw for x in g.xs) > W, "no tile spans the seam"
    # the plain plan of the same arguments is what it was: last tile flush right, nothing past the edge
    plain = E.Plan(W, H, tw, th, ov, bs)
    assert not plain.wrap_x and E.lib().mdtile_plan_wrap_x(plain.handle) == 0
    xs = wr.plain_origins(W, g.tw, g.ov)
    assert plain.bboxes == [(x, y, g.tw, g.th) for y in g.ys for x in xs]
    assert max(b[0] + b[2] for b in plain.bboxes) == W


def test_plan_refuses_a_tile_as_wide_as_the_canvas(built_lib):
    E = built_lib
    assert wr.grid(96, 64, 96, 96, 48, 4) is None
    for tile in (96, 128):
        with pytest.raises(E.MdtileError, match="meet itself"):
            E.Plan(96, 64, tile, 96, 48, 4, wrap_x=True)
    assert E.lib().mdtile_plan_create_wrap_x(96, 64, 96, 96, 48, 4) is None
    assert b"meet itself" in E.lib().mdtile_last_error()
    with pytest.raises(E.MdtileError, match="clamp"):
        E.Plan(200, 64, 96, 96, 48, 4, clamp=False, wrap_x=True)
    assert E.lib().mdtile_plan_wrap_x(None) == 0


# ---- the option --------------------------------------------------------------------------------------------------------------
def test_preload_option(host):
    pl, shared = host
    parser = argparse.ArgumentParser()
    load_preload().preload(parser)
    assert parser.parse_args([]).mdtile_wrap_x is False
    assert parser.parse_args(["--mdtile-wrap-x"]).mdtile_wrap_x is True
    A = pl.abstractdiffusion.AbstractDiffusion
    assert not hasattr(shared.cmd_opts, "mdtile_wrap_x") and A.wrap_x_requested() is False      # a host that never heard of the option
    assert pl.tilevae._cmd_line_wrap_x() is False
    shared.cmd_opts.mdtile_wrap_x = True
    assert A.wrap_x_requested() is True and pl.tilevae._cmd_line_wrap_x() is True
    shared.cmd_opts.mdtile_wrap_x = False
    assert A.wrap_x_requested() is False and pl.tilevae._cmd_line_wrap_x() is False


# ---- script wiring -----------------------------------------------------------------------------------------------------------
def _delegate(pl, W, H, tile, ov, bs=4, method="md"):
    return delegate(pl, W, H, tile, tile, ov, bs, method)


def test_wrap_plan_only_with_the_option(wired, capsys):
    pl, shared = wired
    d, p = _delegate(pl, 40, 24, 24, 16)
    assert not d.plan.wrap_x and d.wrap_ext == 0 and "Tiled Diffusion wrap x" not in (getattr(p, "extra_generation_params", None) or {})
    assert d.plan.bboxes == pl.engine.Plan(40, 24, 24, 24, 16, 4).bboxes
    shared.cmd_opts.mdtile_wrap_x = True
    d, p = _delegate(pl, 40, 24, 24, 16)
    g = wr.grid(40, 24, 24, 24, 16, 4)
    assert d.plan.wrap_x and d.plan.bboxes == list(g.boxes)
    assert p.extra_generation_params["Tiled Diffusion wrap x"] is True
    assert d.wrap_ext == max(g.xs) + g.tw - g.W == 16
    assert [[(b.x, b.y, b.w, b.h) for b in batch] for batch in d.batched_bboxes] == [[g.boxes[t] for t in batch] for batch in g.batches]
    assert "[Tiled Diffusion]" not in capsys.readouterr().out
    # a tile as wide as the canvas: one line, today's plan
    d, p = _delegate(pl, 40, 24, 48, 16)
    out = capsys.readouterr().out
    assert out.count("[Tiled Diffusion]") == 1 and "wrap-x" in out
    assert not d.plan.wrap_x and d.wrap_ext == 0 and d.plan.bboxes == pl.engine.Plan(40, 24, 48, 48, 16, 4).bboxes
    assert "Tiled Diffusion wrap x" not in (getattr(p, "extra_generation_params", None) or {})


def test_wrap_plan_through_the_script(wired):
    """Script.process + the sampler hijack build the delegate: with the option its plan is the wrap-x plan and the infotext says so."""
    pl, shared = wired
    import modules.sd_samplers as sd_samplers
    shared.cmd_opts.mdtile_wrap_x = True
    s = pl.tilediffusion.Script()
    p = sh.make_processing(2048, 512)
    p.extra_generation_params = {}
    defaults = list(pl.utils.DEFAULT_BBOX_SETTINGS) * 8
    s.process(p, True, "MultiDiffusion", False, True, 1024, 1024, 96, 96, 48, 4, "None", 2.0, False, 10, 1, 1, 64, False, False, False, False, *defaults)
    try:
        sd_samplers.create_sampler("Euler", None)
        assert s.delegate.plan.wrap_x and s.delegate.plan.bboxes == list(wr.grid(256, 64, 96, 96, 48, 4).boxes)
        assert p.extra_generation_params["Tiled Diffusion wrap x"] is True
    finally:
        if s.delegate is not None and s.delegate.pbar is not None:
            s.delegate.pbar.close()
        s.postprocess(p, None, True)


def test_regions_are_refused(wired):
    pl, shared = wired
    shared.cmd_opts.mdtile_wrap_x = True
    d, _ = _delegate(pl, 40, 24, 24, 16)
    U = pl.utils
    settings = {0: U.BBoxSettings(True, 0.1, 0.1, 0.4, 0.4, "", "", "Background", 0.2, -1)}
    with pytest.raises(RuntimeError, match="mdtile-wrap-x.*custom regions"):
        d.init_custom_bbox(settings, True, False)
    assert not d.enable_custom_bbox and not d.custom_bboxes
    d.enable_custom_bbox = True                      # armed behind init_custom_bbox's back: init_done still refuses
    with pytest.raises(RuntimeError, match="mdtile-wrap-x.*custom regions"):
        d.init_done()
    del shared.cmd_opts.mdtile_wrap_x                # without the option the same regions are fine
    d, _ = _delegate(pl, 40, 24, 24, 16)
    monkey = pl.engine.weight_map_add_rect
    pl.engine.weight_map_add_rect = lambda *a, **k: None
    try:
        d.init_custom_bbox(settings, True, False)
    finally:
        pl.engine.weight_map_add_rect = monkey
    assert d.enable_custom_bbox and len(d.custom_bboxes) == 1


@pytest.mark.parametrize("method", ["md", "mod"])
def test_icond_slices_of_seam_tiles(wired, method):
    """img2img's image conditioning follows the tiles: repeat_cond_dict (MultiDiffusion) and the per-tile slice_icond (Mixture of Diffusers)
    cut a tile that spans the seam from the extended copy -- equal to the source indexed mod its size."""
    pl, shared = wired
    shared.cmd_opts.mdtile_wrap_x = True
    d, _ = _delegate(pl, 40, 24, 24, 16, bs=2, method=method)
    g = wr.grid(40, 24, 24, 24, 16, 2)
    torch.manual_seed(0)
    icond = torch.randn(2, 5, 24, 40)
    cond = {"c_crossattn": [torch.zeros(2, 77, 8)], "c_concat": [icond]}
    seam = [b for batch in d.batched_bboxes for b in batch if b.x + b.w > 40]
    assert len(seam) == 2
    for batch, idx in zip(d.batched_bboxes, g.batches):
        want = np.concatenate([_take(icond, g.boxes[t]) for t in idx], axis=0)
        if method == "md":
            got = d.get_icond(d.repeat_cond_dict(cond, batch))
        else:
            got = torch.cat([d.slice_icond(d.get_icond(cond), b) for b in batch], dim=0)
        assert got.shape == want.shape and np.array_equal(got.numpy(), want)
    ext = d.extended_x(icond, "icond")
    assert ext.shape[-1] == 40 + 16 and d.extended_x(icond, "icond") is ext, "the extended copy is built once per source tensor"
    icond.add_(1.0)                                   # written in place: a new copy
    assert d.extended_x(icond, "icond") is not ext
    other = torch.randn(2, 5, 1, 1)                   # txt2img's dummy conditioning is not tiled
    assert d.slice_icond(other, seam[0]) is other


@pytest.mark.parametrize("kdiff", [True, False], ids=["kdiff", "ddim"])
def test_controlnet_and_stablesr_slices_of_seam_tiles(wired, kdiff):
    pl, shared = wired
    shared.cmd_opts.mdtile_wrap_x = True
    d, _ = _delegate(pl, 40, 24, 24, 16, bs=2)
    if not kdiff:
        d.sampler_raw = object()
    assert d.is_kdiff == kdiff
    g = wr.grid(40, 24, 24, 24, 16, 2)
    torch.manual_seed(1)
    hint = torch.randn(1, 3, 24 * 8, 40 * 8)
    param = SimpleNamespace(hint_cond=hint)
    d.enable_controlnet, d.control_params, d.org_control_tensor_batch = True, [param], [hint]
    sr = torch.randn(2, 4, 24, 40)
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
    assert d.extended_x(hint, "hint0", 8).shape[-1] == (40 + 16) * 8
    d.reset_controlnet_tensors()
    assert param.hint_cond is hint


# ---- Tiled VAE ---------------------------------------------------------------------------------------------------------------
# (decoder?, tile size, input shape, tiled?): padded inputs above and below the "tiny" threshold of the unchanged path
VAE_CASES = [(True, 16, (1, 4, 24, 56), True), (True, 64, (1, 4, 24, 40), False), (False, 64, (1, 3, 136, 200), True), (False, 256, (1, 3, 96, 128), False)]


@pytest.mark.parametrize("is_decoder,ts,shape,tiled", VAE_CASES, ids=["dec-tiled", "dec-untiled", "enc-tiled", "enc-untiled"])
def test_vae_hook_pads_by_its_tile_pad_and_crops(host, capsys, is_decoder, ts, shape, tiled):
    from hostsim import ldm_decoder as ld
    pl, shared = host
    net = ld.make_decoder(0, small=True) if is_decoder else ld.make_encoder(0, small=True)
    hook = _hook(pl, net, ts, is_decoder)
    P = 11 if is_decoder else 32
    assert hook.pad == P and shape[-1] > 2 * P
    torch.manual_seed(3)
    z = torch.randn(*shape)
    with torch.no_grad():
        capsys.readouterr()
        padded = hook(pad_cols(z, P))
        assert ("tiny" in capsys.readouterr().out) == (not tiled)
        plain = hook(z)
        shared.cmd_opts.mdtile_wrap_x = True
        got = hook(z)
    cut = 8 * P if is_decoder else P // 8
    want = padded[..., cut:padded.shape[-1] - cut]
    assert got.shape == plain.shape == want.shape
    assert torch.equal(got, want)
    assert not torch.equal(got, plain)


@pytest.mark.parametrize("is_decoder,ts,shape", [(True, 16, (1, 4, 60, 22)), (False, 64, (1, 3, 200, 64))], ids=["decoder", "encoder"])
def test_vae_hook_acts_as_today_on_a_canvas_no_wider_than_two_pads(host, is_decoder, ts, shape):
    from hostsim import ldm_decoder as ld
    pl, shared = host
    net = ld.make_decoder(0, small=True) if is_decoder else ld.make_encoder(0, small=True)
    hook = _hook(pl, net, ts, is_decoder)
    assert shape[-1] == 2 * hook.pad
    torch.manual_seed(3)
    z = torch.randn(*shape)
    with torch.no_grad():
        plain = hook(z)
        shared.cmd_opts.mdtile_wrap_x = True
        got = hook(z)
    assert torch.equal(got, plain)
