"""--mdtile-grid-shift without a GPU: the option, the shift function against a table written out from its formula, and the
delegates' wiring on the CPU stub host -- when the option counts, the job's boxes and extended copies, one shift per sampler step, Noise
Inversion's unshifted evaluations, and that no random generator is touched.  The engine's two shifted calls are replaced by doubles that record
their shift (the gather's double is the restatement tests/shift_ref.py); the kernels themselves are tested in tests/test_gpu_shift.py."""
import argparse
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import shift_ref as sr
import wrap_ref as wr
from wrap_common import host, wired, delegate, load_preload, take as _take      # noqa: F401  (host, wired: fixtures)

W, H, TILE, OV, BS = 40, 24, 16, 4, 4


@pytest.fixture
def shifting(wired, monkeypatch):
    """(plugin, shared, calls): wired, the grid-shift option gone before and after, the step counter restored, and the two shifted engine calls
    replaced by doubles that append ("gather" | "blend", sx, sy) to calls."""
    pl, shared = wired
    calls = []

    def gather_all_shift(plan, x_in, sx, sy, out=None):
        calls.append(("gather", sx, sy))
        g = wr.grid(plan.w, plan.h, plan.tile_w, plan.tile_h, plan.overlap, plan.tile_bs, plan.wrap_x, plan.wrap_y)
        assert list(g.boxes) == plan.bboxes
        return [torch.from_numpy(sr.gather(g, x_in.numpy(), b, sx, sy)) for b in range(len(g.batches))]

    def blend_shift(plan, method, batch_out, N, C, *, sx, sy, **kw):
        calls.append(("blend", sx, sy))
        return torch.zeros(N, C, plan.h, plan.w)

    def unshifted(*a, **k):
        raise AssertionError("the unshifted engine call was made with --mdtile-grid-shift active")

    monkeypatch.setattr(pl.engine, "gather_all_shift", gather_all_shift)
    monkeypatch.setattr(pl.engine, "blend_shift", blend_shift)
    monkeypatch.setattr(pl.engine, "gather_all", unshifted)
    monkeypatch.setattr(pl.engine, "blend", unshifted)
    monkeypatch.setattr(shared.state, "sampling_step", 0)
    if hasattr(shared.cmd_opts, "mdtile_grid_shift"):
        monkeypatch.delattr(shared.cmd_opts, "mdtile_grid_shift")
    yield pl, shared, calls
    if hasattr(shared.cmd_opts, "mdtile_grid_shift"):
        del shared.cmd_opts.mdtile_grid_shift


def _torus(pl, shared, method="md", seed=1234567):
    shared.cmd_opts.mdtile_wrap_x = shared.cmd_opts.mdtile_wrap_y = shared.cmd_opts.mdtile_grid_shift = True
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS, method)
    p.all_seeds = [seed]
    if method == "mod":
        d.rescale_factor = torch.ones(1, 1, H, W)
    return d, p


def _evaluate(d, shared, method, x, cond=None):
    if method == "md":
        return d.sample_one_step(x, None, lambda xt, bboxes: xt, None)
    shared.sd_model.apply_model_original_md = lambda x_, t_, c_: x_
    cond = cond or {"c_crossattn": [torch.zeros(2, 77, 8)], "c_concat": [torch.zeros(2, 5, 1, 1)]}
    return d.apply_model_hijack(x, torch.zeros(2), cond)


# ---- the option and the function -------------------------------------------------------------------------------------------------
def test_preload_option(host):
    pl, shared = host
    parser = argparse.ArgumentParser()
    load_preload().preload(parser)
    assert parser.parse_args([]).mdtile_grid_shift is False
    assert parser.parse_args(["--mdtile-grid-shift"]).mdtile_grid_shift is True
    A = pl.abstractdiffusion.AbstractDiffusion
    assert not hasattr(shared.cmd_opts, "mdtile_grid_shift") and A.grid_shift_requested() is False      # a host that never heard of the option
    shared.cmd_opts.mdtile_grid_shift = True
    try:
        assert A.grid_shift_requested() is True
    finally:
        del shared.cmd_opts.mdtile_grid_shift


def test_shift_function_is_pinned(host):
    pl, _ = host
    for (seed, step, axis, extent), want in sr.PINNED.items():
        assert pl.utils.grid_shift(seed, step, axis, extent) == want == sr.shift(seed, step, axis, extent), (seed, step, axis, extent)
    assert sr.PINNED[(0, 0, 0, 128)] == 0xE220A8397B1DCDAF % 128, "splitmix64's first output for state 0"


@pytest.mark.parametrize("extent", [1, 2, 37, 65535])
def test_shift_is_in_range(host, extent):
    pl, _ = host
    got = [pl.utils.grid_shift(seed, step, axis, extent) for seed in (0, 1, 1234567, 2 ** 32 - 1, 2 ** 64 - 1, -1) for step in range(40) for axis in (0, 1)]
    assert all(isinstance(v, int) and 0 <= v < extent for v in got)
    if extent > 2:
        assert len(set(got)) > 2, "the shift does not move"


# ---- when the option counts ------------------------------------------------------------------------------------------------------
def test_ignored_on_a_plain_grid_with_one_line(shifting, capsys):
    pl, shared, calls = shifting
    shared.cmd_opts.mdtile_grid_shift = True
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    out = capsys.readouterr().out
    assert out.count("[Tiled Diffusion]") == 1 and "--mdtile-grid-shift ignored" in out and "does not wrap" in out
    assert not d.grid_shift and (d.wrap_ext, d.wrap_ext_y) == (0, 0)
    assert "Tiled Diffusion grid shift" not in (getattr(p, "extra_generation_params", None) or {})
    assert d.plan.bboxes == pl.engine.Plan(W, H, TILE, TILE, OV, BS).bboxes
    assert d.step_shift() == ((0, 0), d.batched_bboxes)


def test_off_by_default_on_a_wrap_plan(shifting, capsys):
    pl, shared, calls = shifting
    shared.cmd_opts.mdtile_wrap_x = True
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    g = wr.grid(W, H, TILE, TILE, OV, BS)
    assert not d.grid_shift and d.wrap_ext == max(g.xs) + g.tw - g.W and "Tiled Diffusion grid shift" not in p.extra_generation_params
    assert "[Tiled Diffusion]" not in capsys.readouterr().out


@pytest.mark.parametrize("wrap", [(True, False), (False, True), (True, True)], ids=["wrap_x", "wrap_y", "torus"])
def test_infotext_extent_and_axes(shifting, capsys, wrap):
    """Active on a plan that wraps: the infotext says so, wrap_ext is the whole tile on a wrapped axis, and only the axes that wrap move."""
    pl, shared, calls = shifting
    shared.cmd_opts.mdtile_wrap_x, shared.cmd_opts.mdtile_wrap_y = wrap
    shared.cmd_opts.mdtile_grid_shift = True
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    p.all_seeds = [77]
    assert "[Tiled Diffusion]" not in capsys.readouterr().out
    assert d.grid_shift and p.extra_generation_params["Tiled Diffusion grid shift"] is True
    assert (d.wrap_ext, d.wrap_ext_y) == (TILE if wrap[0] else 0, TILE if wrap[1] else 0)
    g = wr.grid(W, H, TILE, TILE, OV, BS, *wrap)
    moved = set()
    for step in range(6):
        shared.state.sampling_step = step
        (sx, sy), boxes = d.step_shift()
        assert (sx, sy) == sr.step_shift(g, wrap[0], wrap[1], 77, step)
        assert [(b.x, b.y, b.w, b.h) for batch in boxes for b in batch] == sr.boxes(g, sx, sy)
        assert [len(batch) for batch in boxes] == [len(b) for b in g.batches]
        moved.add((sx, sy))
    assert len(moved) > 1 and all((sx == 0 or wrap[0]) and (sy == 0 or wrap[1]) for sx, sy in moved)


def test_job_seed(shifting):
    pl, shared, _ = shifting
    d, p = _torus(pl, shared)
    assert d.job_seed() == 1234567
    p.all_seeds, p.seed = [], 42
    assert d.job_seed() == 42
    del p.all_seeds, p.seed
    assert d.job_seed() == 0


# ---- the slices of a step's boxes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["md", "mod"])
def test_slices_of_shifted_boxes(shifting, method):
    """Image conditioning, ControlNet hints and the StableSR latent cut at a step's boxes from the extended copies == the source indexed mod
    its size; the copies are built once for the job although the shift changes."""
    pl, shared, _ = shifting
    d, _ = _torus(pl, shared, method)
    g = wr.grid(W, H, TILE, TILE, OV, BS, True, True)
    torch.manual_seed(0)
    icond = torch.randn(2, 5, H, W)
    cond = {"c_crossattn": [torch.zeros(2, 77, 8)], "c_concat": [icond]}
    hint = torch.randn(1, 3, H * 8, W * 8)
    param = SimpleNamespace(hint_cond=hint)
    d.enable_controlnet, d.control_params, d.org_control_tensor_batch = True, [param], [hint]
    latent = torch.randn(2, 4, H, W)
    model = SimpleNamespace(latent_image=None)
    d.enable_stablesr, d.stablesr_script, d.stablesr_tensor = True, SimpleNamespace(stablesr_model=model), latent
    ext = None
    for step in range(4):
        shared.state.sampling_step = step
        (sx, sy), batched = d.step_shift()
        boxes = sr.boxes(g, sx, sy)
        assert any(x + w > W for (x, y, w, h) in boxes) or any(y + h > H for (x, y, w, h) in boxes)
        for batch_id, (batch, idx) in enumerate(zip(batched, g.batches)):
            want = np.concatenate([_take(icond, boxes[t]) for t in idx], axis=0)
            if method == "md":
                got = d.get_icond(d.repeat_cond_dict(cond, batch))
            else:
                got = torch.cat([d.slice_icond(d.get_icond(cond), b) for b in batch], dim=0)
            assert got.shape == want.shape and np.array_equal(got.numpy(), want), (step, batch_id)
            d.switch_controlnet_tensors(batch_id, 2, len(idx), batched_bboxes=batched)
            tiles = np.concatenate([_take(hint, boxes[t], 8) for t in idx], axis=0)
            assert np.array_equal(param.hint_cond.numpy(), np.repeat(tiles, 2, axis=0)), (step, batch_id)
            d.switch_stablesr_tensors(batch_id, batched)
            assert np.array_equal(model.latent_image.numpy(), np.concatenate([_take(latent, boxes[t]) for t in idx], axis=0)), (step, batch_id)
        if ext is None:
            ext = d.extended_x(icond, "icond")
            assert tuple(ext.shape[-2:]) == (H + TILE, W + TILE)
        assert d.extended_x(icond, "icond") is ext, "the extended copy is rebuilt although its source did not change"


# ---- one shift per sampler step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["md", "mod"])
def test_one_shift_per_step(shifting, method):
    """Two evaluations at one value of the step counter (cond and uncond calls) run the same tiling; the next step has its own.  Gather and
    blend of one evaluation always get the same shift, and the tiles the model sees are the restatement's at that shift."""
    pl, shared, calls = shifting
    d, _ = _torus(pl, shared, method)
    g = wr.grid(W, H, TILE, TILE, OV, BS, True, True)
    x = torch.randn(2, 4, H, W)
    per_step = []
    for step in (0, 0, 1, 2, 2):
        shared.state.sampling_step = step
        del calls[:]
        _evaluate(d, shared, method, x)
        want = (sr.shift(1234567, step, 0, W), sr.shift(1234567, step, 1, H))
        assert calls == [("gather",) + want, ("blend",) + want], (step, calls)
        per_step.append(want)
    assert per_step[0] == per_step[1] and per_step[3] == per_step[4] and len({per_step[0], per_step[2], per_step[3]}) == 3


# ---- Noise Inversion -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["md", "mod"])
def test_get_noise_passes_shift_zero(shifting, capsys, method):
    pl, shared, calls = shifting
    d, _ = _torus(pl, shared, method)
    shared.state.sampling_step = 1
    assert d.step_shift()[0] != (0, 0)
    x = torch.randn(1, 4, H, W)
    cond = {"c_crossattn": [torch.zeros(1, 77, 8)], "c_concat": [torch.zeros(1, 5, 1, 1)]}
    model = lambda x_, t_, cond=None: x_
    shared.sd_model.apply_model = model
    shared.sd_model.apply_model_original_md = lambda x_, t_, c_: x_
    capsys.readouterr()
    for _ in range(2):
        d.get_noise(x, torch.zeros(1), cond, 0)
    assert calls == [("gather", 0, 0), ("blend", 0, 0)] * 2
    out = capsys.readouterr().out
    assert out.count("--mdtile-grid-shift not applied") == 1 and "Noise Inversion" in out
    del calls[:]
    _evaluate(d, shared, method, torch.randn(2, 4, H, W))        # the sampler's own evaluations still move
    assert calls[0][1:] == (sr.shift(1234567, 1, 0, W), sr.shift(1234567, 1, 1, H)) != (0, 0)


# ---- no generator is touched -------------------------------------------------------------------------------------------------------
def test_the_random_generators_are_left_alone(shifting):
    pl, shared, calls = shifting
    d, _ = _torus(pl, shared)
    x = torch.randn(2, 4, H, W)
    torch_state, numpy_state = torch.get_rng_state(), np.random.get_state()
    for step in range(5):
        shared.state.sampling_step = step
        _evaluate(d, shared, "md", x)
    assert len({c[1:] for c in calls}) > 1
    assert torch.equal(torch.get_rng_state(), torch_state)
    after = np.random.get_state()
    assert after[0] == numpy_state[0] and np.array_equal(after[1], numpy_state[1]) and after[2:] == numpy_state[2:]
