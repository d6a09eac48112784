"""--mdtile-grid-jitter without a GPU: the host integers of mdtile_lattice_make / mdtile_lattice_bboxes against the numpy
restatement tests/grid_lattice_ref.py, what the calls refuse (argument checks happen before any device is touched), header = library = binding, the
option, the shift function against a literal table, and the delegates' wiring on the CPU stub host with engine doubles, in the manner of
tests/test_shift_host.py: one lattice per sampler step, slices at the pushed-in boxes, every not-applied case with its single line and the
unjittered calls, no random generator touched, the infotext.  The kernels themselves are tested in tests/test_gpu_lattice.py."""
import argparse
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import grid_lattice_ref as lr
from wrap_common import host, wired, delegate, load_preload      # noqa: F401  (host, wired: fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mdtile_lattice_make", "mdtile_lattice_bboxes", "mdtile_lattice_weight_map", "mdtile_gather_all_lattice", "mdtile_blend_lattice"]
W, H, TILE, OV, BS = 40, 24, 16, 4, 4      # stride 12: 3 columns at rest, 4 at any other shift; 2 rows at shifts 4 .. 12, 3 below
SEED = 1234567


# ---- symbols ---------------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdtile.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mdtile_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(built_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/mdtile.h"
        assert hasattr(lib, name), f"libmdtile.so does not export {name}"
        assert name in built_lib.exported_symbols(), f"the binding has no signature for {name}"
    assert sorted(built_lib.exported_symbols()) == sorted(declared)
    assert built_lib.lib().mdtile_version() == 100
    fields = re.search(r"typedef struct mdtile_lattice \{(.*?)\} mdtile_lattice;", src, flags=re.S).group(1)
    names = [n.strip() for decl in re.findall(r"int ([^;]+);", fields) for n in decl.split(",")]
    assert names == [n for n, _ in built_lib._Lattice._fields_], "the binding's struct is not the header's"


# ---- the host integers -----------------------------------------------------------------------------------------------------------
def test_the_restatement_is_pinned_on_literal_numbers():
    g = lr.lattice(40, 24, 16, 16, 4, 4, 12, 12)          # at rest: the plain grid
    assert (g.us, g.xs, g.vs, g.ys) == ((0, 12, 24), (0, 12, 24), (0, 12), (0, 8)) and g.tile_bs == 3 and len(g.batches) == 2
    g = lr.lattice(40, 24, 16, 16, 4, 4, 1, 5)
    assert (g.us, g.xs) == ((-11, 1, 13, 25), (0, 1, 13, 24)) and (g.vs, g.ys) == ((-7, 5, 17), (0, 5, 8))
    g = lr.lattice(16, 40, 16, 16, 0, 4, 7, 16)           # the tile spans x: one column, sx ignored
    assert (g.us, g.xs, g.sx, g.cols) == ((0,), (0,), 0, 1) and g.vs == (0, 16, 32) and g.ys == (0, 16, 24)


def _same(E, g, lat):
    assert (lat.w, lat.h, lat.tile_w, lat.tile_h, lat.overlap) == (g.W, g.H, g.tw, g.th, g.ov)
    assert (lat.stride_x, lat.stride_y, lat.sx, lat.sy) == (g.stride_x, g.stride_y, g.sx, g.sy)
    assert (lat.cols, lat.rows, lat.num_tiles, lat.num_batches, lat.tile_bs) == (g.cols, g.rows, len(g.boxes), len(g.batches), g.tile_bs)
    assert lat.bboxes == list(g.boxes)
    assert [len(b) for b in lat.batches] == [len(b) for b in g.batches]


@pytest.mark.parametrize("tile_w,tile_h,ov", [(16, 16, 0), (16, 16, 4), (16, 16, 12), (16, 12, 4), (8, 24, 3), (5, 7, 1), (40, 9, 2), (64, 64, 8)])
def test_make_and_bboxes_equal_the_restatement(built_lib, tile_w, tile_h, ov):
    """W, H in 5 .. 48, every shift of both axes (x swept at sy = rest and y at sx = rest, plus the diagonal): the library's integers are the
    explicit loop's, and the properties the kernels rely on hold."""
    E = built_lib
    checked = 0
    for Wc in range(5, 49):
        for Hc in (5, 22, 48) if Wc % 4 else range(5, 49):
            if lr.lattice(Wc, Hc, tile_w, tile_h, ov, 4, 1, 1) is None:
                with pytest.raises(E.MdtileError, match="overlap"):
                    E.Lattice(Wc, Hc, tile_w, tile_h, ov, 4, 1, 1)
                continue
            stx, sty = lr.rest(Wc, Hc, tile_w, tile_h, ov)
            stx, sty = max(stx, 1), max(sty, 1)            # an axis that does not move ignores its shift (its stride may be <= 0)
            shifts = {(sx, sty) for sx in range(1, stx + 1)} | {(stx, sy) for sy in range(1, sty + 1)} | {(s, s) for s in range(1, min(stx, sty) + 1)}
            for (sx, sy) in sorted(shifts):
                g = lr.lattice(Wc, Hc, tile_w, tile_h, ov, 4, sx, sy)
                _same(E, g, E.Lattice(Wc, Hc, tile_w, tile_h, ov, 4, sx, sy))
                checked += 1
                for org, psh, tile, extent in ((g.us, g.xs, g.tw, g.W), (g.vs, g.ys, g.th, g.H)):
                    assert all(a < b for a, b in zip(psh, psh[1:])), "pushed-in origins not strictly increasing"
                    for p in range(extent):
                        cover = [k for k, u in enumerate(org) if u <= p < u + tile]
                        assert cover and cover == list(range(cover[0], cover[-1] + 1)) and all(0 <= p - psh[k] < tile for k in cover)
    assert checked > 100


def test_batching_follows_the_plan_rule(built_lib):
    for bs in (1, 3, 4, 5, 100):
        _same(built_lib, lr.lattice(37, 22, 16, 12, 4, bs, 2, 1), built_lib.Lattice(37, 22, 16, 12, 4, bs, 2, 1))


def test_at_rest_the_lattice_is_the_plain_plan(built_lib):
    E = built_lib
    for (Wc, Hc, tw, th, ov) in [(40, 28, 16, 16, 4), (64, 64, 32, 32, 0), (1024, 1024, 128, 128, 0), (16, 40, 16, 16, 4)]:
        plan = E.Plan(Wc, Hc, tw, th, ov, 4)
        stx, sty = lr.rest(Wc, Hc, tw, th, ov)
        assert (Wc - plan.tile_w) % stx == 0 and (Hc - plan.tile_h) % sty == 0
        lat = E.Lattice(Wc, Hc, tw, th, ov, 4, stx, sty)
        assert lat.bboxes == plan.bboxes and (lat.cols, lat.rows, lat.num_batches, lat.tile_bs) == (plan.cols, plan.rows, plan.num_batches, plan.tile_bs)
    assert E.Lattice(1024, 1024, 128, 128, 0, 8, 128, 128).num_tiles == 64 and E.Lattice(1024, 1024, 128, 128, 0, 8, 1, 1).num_tiles == 81


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_make_refuses_and_writes_nothing(built_lib):
    E, L = built_lib, built_lib.lib()
    lat = E._Lattice(*([-7] * 14))
    for args, text in [((40, 24, 16, 16, 4, 4, 0, 12), r"sx = 0 outside \[1, 12\]"), ((40, 24, 16, 16, 4, 4, 13, 12), r"sx = 13 outside \[1, 12\]"),
                       ((40, 24, 16, 16, 4, 4, 12, 0), r"sy = 0 outside \[1, 12\]"), ((40, 24, 16, 16, 4, 4, 12, -3), r"sy = -3 outside"),
                       ((0, 24, 16, 16, 4, 4, 1, 1), "bad arguments"), ((40, 24, 16, 16, 4, 0, 1, 1), "bad arguments"),
                       ((70000, 24, 16, 16, 4, 4, 1, 1), "bad arguments"), ((40, 8, 16, 16, 8, 4, 1, 1), "overlap 8 equals")]:
        assert L.mdtile_lattice_make(*args, ctypes.byref(lat)) == E.E_ARG
        assert re.search(text, L.mdtile_last_error().decode()), (args, L.mdtile_last_error())
        assert all(getattr(lat, n) == -7 for n, _ in E._Lattice._fields_), "a refused mdtile_lattice_make wrote to the struct"
    assert L.mdtile_lattice_make(16, 40, 16, 16, 4, 4, 99, 3, ctypes.byref(lat)) == 0 and (lat.sx, lat.sy, lat.cols) == (0, 3, 1)      # sx ignored


def _fake(n):
    """n pointers that are not null and are never followed: a refused call reads no device memory."""
    return (ctypes.c_void_p * n)(*([0x1000] * n))


def test_calls_refuse_before_any_device_is_touched(built_lib):
    E, L = built_lib, built_lib.lib()
    lat = E.Lattice(W, H, TILE, TILE, OV, BS, 5, 5)
    nb = lat.num_batches

    def blend(text, lat_c=None, nbat=nb, **kw):
        f = dict(method=E.METHOD_MD, dtype=0, N=2, C=4, flags=0, tile_lo=0, tile_hi=0, row_lo=0, row_hi=0, d_weights=None, d_tile_w=None, d_rescale=None,
                 d_x_out=0x1000)
        f.update(kw)
        a = E._BlendArgs(**f)
        assert L.mdtile_blend_lattice(ctypes.byref(lat_c) if lat_c is not None else lat.ref, ctypes.byref(a), _fake(max(nbat, 1)), nbat, None) == E.E_ARG
        assert re.search(text, L.mdtile_last_error().decode()), L.mdtile_last_error()

    def gather(text, lat_c=None, nbat=nb, dtype=0, N=2, C=4):
        assert L.mdtile_gather_all_lattice(ctypes.byref(lat_c) if lat_c is not None else lat.ref, dtype, N, C, 0x1000, _fake(max(nbat, 1)), nbat, None) == E.E_ARG
        assert re.search(text, L.mdtile_last_error().decode()), L.mdtile_last_error()

    blend(r"%d batches given, the lattice has %d" % (nb + 1, nb), nbat=nb + 1)
    gather(r"%d batches given, the lattice has %d" % (nb - 1, nb), nbat=nb - 1)
    blend("d_weights and d_rescale must be NULL", d_weights=0x1000)
    blend("d_weights and d_rescale must be NULL", d_rescale=0x1000, method=E.METHOD_MOD, d_tile_w=0x1000)
    blend("no MDTILE_BLEND_\\* flags", flags=E.BLEND_PARTIAL)
    blend("no row band", row_lo=0, row_hi=8)
    blend("Mixture of Diffusers needs d_tile_w", method=E.METHOD_MOD)
    blend("bad method", method=2)
    blend("bad dtype", dtype=3)
    blend("bad N=0", N=0)
    blend("null output", d_x_out=None)
    gather("bad dtype", dtype=-1)
    gather("bad N=2 C=40000", C=40000)
    # a struct that mdtile_lattice_make did not write
    def broken(**kw):
        c = E._Lattice(*[getattr(lat._c, n) for n, _ in E._Lattice._fields_])
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    for kw, text in [(dict(sx=0), r"sx = 0 outside \[1, 12\]"), (dict(sy=13), r"sy = 13 outside \[1, 12\]"), (dict(cols=lat.cols + 1), "tiles along x"),
                     (dict(rows=1), "tiles along y"), (dict(stride_x=8), "stride_x"), (dict(num_tiles=lat.num_tiles + 1), "bad lattice"),
                     (dict(tile_bs=1), "bad lattice"), (dict(tile_w=W + 1), "bad lattice"), (dict(h=0), "bad lattice")]:
        blend(text, lat_c=broken(**kw))
        gather(text, lat_c=broken(**kw))
        buf = (ctypes.c_int * (4 * 64))()
        assert L.mdtile_lattice_bboxes(ctypes.byref(broken(**kw)), buf) == E.E_ARG
        assert L.mdtile_lattice_weight_map(ctypes.byref(broken(**kw)), None, 0x1000, None) == E.E_ARG
    # more batches than the argument block carries: 19 x 19 tiles at batch size 1
    many = E.Lattice(100, 100, 10, 10, 5, 1, 5, 5)
    assert many.num_batches == 361 > E.MAX_BATCHES
    gather("MDTILE_MAX_BATCHES", lat_c=many._c, nbat=many.num_batches)
    blend("MDTILE_MAX_BATCHES", lat_c=many._c, nbat=many.num_batches)


# ---- the option and the function -------------------------------------------------------------------------------------------------
def test_preload_option(host):
    pl, shared = host
    parser = argparse.ArgumentParser()
    load_preload().preload(parser)
    assert parser.parse_args([]).mdtile_grid_jitter is False
    assert parser.parse_args(["--mdtile-grid-jitter"]).mdtile_grid_jitter is True
    A = pl.abstractdiffusion.AbstractDiffusion
    assert not hasattr(shared.cmd_opts, "mdtile_grid_jitter") and A.grid_jitter_requested() is False      # a host that never heard of the option
    shared.cmd_opts.mdtile_grid_jitter = True
    try:
        assert A.grid_jitter_requested() is True
    finally:
        del shared.cmd_opts.mdtile_grid_jitter


def test_shift_function_is_pinned(host):
    pl, _ = host
    for (seed, step, axis, stride), want in lr.PINNED.items():
        assert pl.utils.lattice_shift(seed, step, axis, stride) == want == lr.shift(seed, step, axis, stride), (seed, step, axis, stride)
        assert want == 1 + pl.utils.grid_shift(seed, step, axis, stride)
    assert lr.PINNED[(0, 0, 0, 128)] == 1 + 0xE220A8397B1DCDAF % 128, "splitmix64's first output for state 0"


@pytest.mark.parametrize("stride", [1, 2, 12, 128])
def test_shift_is_in_range(host, stride):
    pl, _ = host
    got = [pl.utils.lattice_shift(seed, step, axis, stride) for seed in (0, 1, SEED, 2 ** 32 - 1, 2 ** 64 - 1, -1) for step in range(40) for axis in (0, 1)]
    assert all(isinstance(v, int) and 1 <= v <= stride for v in got)
    if stride > 2:
        assert len(set(got)) > 2, "the shift does not move"


# ---- wiring ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def jittering(wired, monkeypatch):
    """(plugin, shared, calls): wired, the option gone before and after, the step counter restored, the two lattice calls replaced by doubles
    that append ("gather" | "blend", sx, sy, the lattice) and the fixed grid's calls by doubles that append ("plain gather" | "plain blend")."""
    pl, shared = wired
    calls = []

    def gather_all_lattice(lat, x_in, out=None):
        calls.append(("gather", lat.sx, lat.sy, lat))
        g = lr.lattice(lat.w, lat.h, TILE, TILE, OV, BS, lat.sx, lat.sy)
        assert list(g.boxes) == lat.bboxes
        return [torch.from_numpy(lr.gather(g, x_in.numpy(), b)) for b in range(len(g.batches))]

    def blend_lattice(lat, method, batch_out, N, C, *, tile_w=None, **kw):
        assert not kw and len(batch_out) == lat.num_batches and (tile_w is not None) == (method == pl.engine.METHOD_MOD)
        calls.append(("blend", lat.sx, lat.sy, lat))
        return torch.zeros(N, C, lat.h, lat.w)

    def gather_all(plan, x_in, out=None):
        calls.append(("plain gather",))
        return [torch.zeros(len(b) * x_in.shape[0], x_in.shape[1], plan.tile_h, plan.tile_w) for b in plan.batches]

    def blend(plan, method, batch_out, N, C, **kw):
        calls.append(("plain blend",))
        return torch.zeros(N, C, plan.h, plan.w)

    monkeypatch.setattr(pl.engine, "gather_all_lattice", gather_all_lattice)
    monkeypatch.setattr(pl.engine, "blend_lattice", blend_lattice)
    monkeypatch.setattr(pl.engine, "gather_all", gather_all)
    monkeypatch.setattr(pl.engine, "blend", blend)
    monkeypatch.setattr(pl.engine, "blend_sparse", lambda plan, method, batch_out, N, C, **kw: calls.append(("sparse blend",)) or torch.zeros(N, C, plan.h, plan.w))
    monkeypatch.setattr(shared.state, "sampling_step", 0)
    names = ("mdtile_grid_jitter", "mdtile_grid_shift", "mdtile_inpaint_skip", "mdtile_wrap_x", "mdtile_wrap_y")
    for n in names:
        if hasattr(shared.cmd_opts, n):
            monkeypatch.delattr(shared.cmd_opts, n)
    yield pl, shared, calls
    for n in names:
        if hasattr(shared.cmd_opts, n):
            delattr(shared.cmd_opts, n)


def _job(pl, shared, method="md", w=W, h=H, tile=TILE, bs=BS, **opts):
    shared.cmd_opts.mdtile_grid_jitter = True
    for k, v in opts.items():
        setattr(shared.cmd_opts, k, v)
    d, p = delegate(pl, w, h, tile, tile, OV, bs, method)
    p.all_seeds = [SEED]
    return d, p


def _evaluate(d, shared, method, x, cond=None):
    if method == "md":
        return d.sample_one_step(x, None, lambda xt, bboxes: xt, None)
    shared.sd_model.apply_model_original_md = lambda x_, t_, c_: x_
    cond = cond or {"c_crossattn": [torch.zeros(2, 77, 8)], "c_concat": [torch.zeros(2, 5, 1, 1)]}
    return d.apply_model_hijack(x, torch.zeros(2), cond)


def _want(step):
    return lr.step_shift(W, H, TILE, TILE, OV, SEED, step)


@pytest.mark.parametrize("method", ["md", "mod"])
def test_one_lattice_per_step(jittering, capsys, method):
    """Two evaluations at one value of the step counter (cond and uncond calls) run the same lattice object; the next step has its own, with
    other shifts.  Gather and blend of one evaluation get the same lattice, and the infotext says that the grid moved."""
    pl, shared, calls = jittering
    d, p = _job(pl, shared, method)
    assert d.grid_jitter and "Tiled Diffusion grid jitter" not in (getattr(p, "extra_generation_params", None) or {})
    x = torch.randn(2, 4, H, W)
    per_step = []
    for step in (0, 0, 1, 2, 2):
        shared.state.sampling_step = step
        del calls[:]
        out = _evaluate(d, shared, method, x)
        assert tuple(out.shape) == (2, 4, H, W)
        assert [c[:3] for c in calls] == [("gather",) + _want(step), ("blend",) + _want(step)], (step, calls)
        assert calls[0][3] is calls[1][3]
        per_step.append(calls[0][3])
    assert per_step[0] is per_step[1] and per_step[3] is per_step[4]
    assert len({(l.sx, l.sy) for l in per_step}) == 3, "the lattice does not move"
    assert all(1 <= l.sx <= TILE - OV and 1 <= l.sy <= TILE - OV for l in per_step)
    assert p.extra_generation_params["Tiled Diffusion grid jitter"] is True
    assert "[Tiled Diffusion]" not in capsys.readouterr().out


@pytest.mark.parametrize("method", ["md", "mod"])
def test_slices_at_the_pushed_in_boxes(jittering, method):
    """Image conditioning, ControlNet hints and the StableSR latent are cut at the step's pushed-in boxes: ordinary slices inside the canvas."""
    pl, shared, _ = jittering
    d, _ = _job(pl, shared, method)
    torch.manual_seed(0)
    icond = torch.randn(2, 5, H, W)
    cond = {"c_crossattn": [torch.zeros(2, 77, 8)], "c_concat": [icond]}
    hint = torch.randn(1, 3, H * 8, W * 8)
    param = SimpleNamespace(hint_cond=hint)
    d.enable_controlnet, d.control_params, d.org_control_tensor_batch = True, [param], [hint]
    latent = torch.randn(2, 4, H, W)
    model = SimpleNamespace(latent_image=None)
    d.enable_stablesr, d.stablesr_script, d.stablesr_tensor = True, SimpleNamespace(stablesr_model=model), latent
    counts = set()
    for step in range(4):
        shared.state.sampling_step = step
        lat, batched = d.step_lattice()
        g = lr.lattice(W, H, TILE, TILE, OV, BS, *_want(step))
        counts.add(len(g.boxes))
        assert [(b.x, b.y, b.w, b.h) for batch in batched for b in batch] == list(g.boxes)
        assert all(0 <= x and x + w <= W and 0 <= y and y + h <= H for (x, y, w, h) in g.boxes)
        cut = lambda src, box, s=1: src[:, :, box[1] * s:(box[1] + box[3]) * s, box[0] * s:(box[0] + box[2]) * s]
        for batch_id, (batch, idx) in enumerate(zip(batched, g.batches)):
            want = torch.cat([cut(icond, g.boxes[t]) for t in idx], dim=0)
            if method == "md":
                got = d.get_icond(d.repeat_cond_dict(cond, batch))
            else:
                got = torch.cat([d.slice_icond(d.get_icond(cond), b) for b in batch], dim=0)
            assert torch.equal(got, want), (step, batch_id)
            d.switch_controlnet_tensors(batch_id, 2, len(idx), batched_bboxes=batched)
            tiles = torch.cat([cut(hint, g.boxes[t], 8) for t in idx], dim=0)
            assert torch.equal(param.hint_cond, tiles.repeat_interleave(2, dim=0)), (step, batch_id)
            d.switch_stablesr_tensors(batch_id, batched)
            assert torch.equal(model.latent_image, torch.cat([cut(latent, g.boxes[t]) for t in idx], dim=0)), (step, batch_id)
    assert len(counts) > 1, "the steps of this test never change the tile count"


def test_the_tiles_the_model_sees(jittering):
    """The batches handed to the model are the restatement's gather at the step's lattice, the short last batch included."""
    pl, shared, calls = jittering
    d, _ = _job(pl, shared)
    x = torch.randn(2, 4, H, W)
    shared.state.sampling_step = 3
    seen = []
    d.sample_one_step(x, None, lambda xt, bboxes: seen.append((xt, len(bboxes))) or xt, None)
    g = lr.lattice(W, H, TILE, TILE, OV, BS, *_want(3))
    assert [n for _, n in seen] == [len(b) for b in g.batches]
    for b, (xt, _) in enumerate(seen):
        assert np.array_equal(xt.numpy(), lr.gather(g, x.numpy(), b))


def _fixed_grid_ran(d, shared, calls, method, capsys, reason, x=None):
    """Two evaluations: only the unjittered calls, and one line per job that names `reason`."""
    del calls[:]
    for step in (0, 1):
        shared.state.sampling_step = step
        _evaluate(d, shared, method, torch.randn(2, 4, d.h, d.w) if x is None else x)
    assert calls and not any(c[0] in ("gather", "blend") for c in calls), calls
    out = capsys.readouterr().out
    assert out.count("--mdtile-grid-jitter not applied") == 1 and out.count("[Tiled Diffusion]") == 1 and reason in out, out
    assert "Tiled Diffusion grid jitter" not in (getattr(d.p, "extra_generation_params", None) or {})


@pytest.mark.parametrize("method", ["md", "mod"])
def test_not_applied_on_a_canvas_that_wraps(jittering, capsys, monkeypatch, method):
    pl, shared, calls = jittering
    d, _ = _job(pl, shared, method, mdtile_wrap_x=True)
    assert not d.grid_jitter and d.wrap_x
    if method == "mod":
        d.rescale_factor = torch.ones(1, 1, H, W)
    _fixed_grid_ran(d, shared, calls, method, capsys, "--mdtile-grid-shift")
    assert [c[0] for c in calls] == ["plain gather", "plain blend"] * 2


@pytest.mark.parametrize("method", ["md", "mod"])
def test_not_applied_with_region_control(jittering, capsys, monkeypatch, method):
    pl, shared, calls = jittering
    d, _ = _job(pl, shared, method)
    assert d.grid_jitter
    d.enable_custom_bbox = True            # region prompt control armed, as init_custom_bbox leaves it (the region list itself is not the point)
    if method == "mod":
        d.rescale_factor = torch.ones(1, 1, H, W)
    monkeypatch.setattr(d, "region_specs", lambda outs: [])
    _fixed_grid_ran(d, shared, calls, method, capsys, "region prompt control")
    d2, _ = _job(pl, shared, method)
    d2.draw_background = False
    if method == "mod":
        d2.rescale_factor = torch.ones(1, 1, H, W)
    _fixed_grid_ran(d2, shared, calls, method, capsys, "no background")
    assert [c[0] for c in calls] == ["plain blend"] * 2


@pytest.mark.parametrize("decided", ["sparse", "empty"])
def test_not_applied_when_inpaint_skip_skips_tiles(jittering, capsys, decided):
    pl, shared, calls = jittering
    d, _ = _job(pl, shared, "md", mdtile_inpaint_skip=True)
    d.skip_mode = decided
    if decided == "sparse":
        d.sparse_plan = d.plan.subset([1] + [0] * (d.plan.num_tiles - 1), BS)
        d.sparse_batched_bboxes = [[pl.utils.BBox(*b) for b in batch] for batch in d.sparse_plan.batches]
    x = torch.randn(2, 4, H, W)
    for step in (0, 1):                   # "empty" makes no engine call at all
        shared.state.sampling_step = step
        out = d.sample_one_step(x, None, lambda xt, bboxes: xt, None)
    assert not any(c[0] in ("gather", "blend") for c in calls)
    assert [c[0] for c in calls] == (["plain gather", "sparse blend"] * 2 if decided == "sparse" else [])
    if decided == "empty":
        assert torch.equal(out, x) and out is not x
    text = capsys.readouterr().out
    assert text.count("--mdtile-grid-jitter not applied") == 1 and f'decided "{decided}"' in text


@pytest.mark.parametrize("method", ["md", "mod"])
def test_noise_inversion_runs_the_fixed_grid(jittering, capsys, method):
    pl, shared, calls = jittering
    d, _ = _job(pl, shared, method)
    if method == "mod":
        d.rescale_factor = torch.ones(1, 1, H, W)
    x = torch.randn(1, 4, H, W)
    cond = {"c_crossattn": [torch.zeros(1, 77, 8)], "c_concat": [torch.zeros(1, 5, 1, 1)]}
    shared.sd_model.apply_model = lambda x_, t_, cond=None: x_
    shared.sd_model.apply_model_original_md = lambda x_, t_, c_: x_
    shared.state.sampling_step = 1
    capsys.readouterr()
    for _ in range(2):
        d.get_noise(x, torch.zeros(1), cond, 0)
    assert [c[0] for c in calls] == ["plain gather", "plain blend"] * 2
    out = capsys.readouterr().out
    assert out.count("--mdtile-grid-jitter not applied") == 1 and "Noise Inversion" in out
    del calls[:]
    _evaluate(d, shared, method, torch.randn(2, 4, H, W))        # the sampler's own evaluations still move
    assert [c[:3] for c in calls] == [("gather",) + _want(1), ("blend",) + _want(1)]


def test_not_applied_when_no_axis_can_move(jittering, capsys):
    pl, shared, calls = jittering
    d, _ = _job(pl, shared, "md", tile=64)
    assert not d.grid_jitter and d.plan.num_tiles == 1
    _fixed_grid_ran(d, shared, calls, "md", capsys, "no axis can move")


def test_not_applied_beyond_the_batch_limit(jittering, capsys):
    """104 x 104 at tile 8 / overlap 4: 25 x 25 = 625 tiles at rest, 26 x 26 at shift 1, batch size 2 -> 338 batches > 320.  (The fixed grid packs
    any number of batches into one buffer.)"""
    pl, shared, calls = jittering
    d, _ = _job(pl, shared, "md", w=104, h=104, tile=8, bs=2)
    assert pl.engine.Lattice(104, 104, 8, 8, OV, 2, 1, 1).num_batches == 338 > pl.engine.MAX_BATCHES >= d.plan.num_batches == 313
    assert not d.grid_jitter
    _fixed_grid_ran(d, shared, calls, "md", capsys, "338 batches")


def test_one_axis_moves_when_the_tile_spans_the_other(jittering, capsys):
    pl, shared, calls = jittering
    d, _ = _job(pl, shared, "md", w=16, h=40)
    assert d.grid_jitter
    shifts = set()
    for step in range(4):
        shared.state.sampling_step = step
        _evaluate(d, shared, "md", torch.randn(2, 4, 40, 16))
        shifts.add(calls[-1][1:3])
    assert all(sx == 0 and 1 <= sy <= TILE - OV for sx, sy in shifts) and len(shifts) > 1
    assert "[Tiled Diffusion]" not in capsys.readouterr().out


def test_off_by_default_and_grid_shift_keeps_its_message(jittering, capsys):
    pl, shared, calls = jittering
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    assert not d.grid_jitter and d.step_lattice() is None and "[Tiled Diffusion]" not in capsys.readouterr().out
    _evaluate(d, shared, "md", torch.randn(2, 4, H, W))
    assert [c[0] for c in calls] == ["plain gather", "plain blend"]
    shared.cmd_opts.mdtile_grid_shift = True
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    out = capsys.readouterr().out
    assert out.count("[Tiled Diffusion]") == 1 and "--mdtile-grid-shift ignored" in out and "does not wrap" in out and not d.grid_shift


def test_the_progress_bar_is_sized_from_the_largest_tile_count(jittering):
    pl, shared, _ = jittering
    d, _ = _job(pl, shared)
    most = pl.engine.Lattice(W, H, TILE, TILE, OV, BS, 1, 1)
    assert most.num_tiles == 12 and d.plan.num_tiles == 6 and most.num_batches == 3 > d.num_batches == 2
    assert all(pl.engine.Lattice(W, H, TILE, TILE, OV, BS, sx, sy).num_batches <= most.num_batches for sx in range(1, 13) for sy in range(1, 13))
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    assert d.total_bboxes == most.num_batches
    del shared.cmd_opts.mdtile_grid_jitter
    d, _ = delegate(pl, W, H, TILE, TILE, OV, BS)
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    assert d.total_bboxes == d.num_batches == 2


def test_the_random_generators_are_left_alone(jittering):
    pl, shared, calls = jittering
    d, _ = _job(pl, shared)
    x = torch.randn(2, 4, H, W)
    torch_state, numpy_state = torch.get_rng_state(), np.random.get_state()
    for step in range(5):
        shared.state.sampling_step = step
        _evaluate(d, shared, "md", x)
    assert len({c[1:3] for c in calls}) > 1
    assert torch.equal(torch.get_rng_state(), torch_state)
    after = np.random.get_state()
    assert after[0] == numpy_state[0] and np.array_equal(after[1], numpy_state[1]) and after[2:] == numpy_state[2:]
