"""Tile skipping without a GPU: the new symbols in header, library and binding, the sparse plan of the library against the
numpy restatement tests/sparse_ref.py, what mdtile_plan_create_subset refuses, the calls a sparse plan refuses by name (argument checks happen
before any device is touched), and the --mdtile-inpaint-skip option."""
import argparse
import ctypes
import os
import re
import sys
from ctypes import c_int

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUGIN = os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd")
for _p in (ROOT, PLUGIN, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import sparse_ref as sr                  # noqa: E402
from hostsim import stub_host as sh      # noqa: E402
from wrap_common import host, wired, delegate, load_preload      # noqa: E402,F401

NEW_SYMBOLS = ["mdtile_tile_activity", "mdtile_plan_create_subset", "mdtile_plan_active", "mdtile_blend_sparse"]
# (W, H, requested tile_w, tile_h, overlap, tile_bs): the GPU cases of tests/test_gpu_sparse.py and an 8K canvas's latent at tile 128 / overlap 8
GEOMETRIES = [(37, 20, 16, 12, 6, 4), (64, 24, 32, 32, 16, 3), (40, 24, 24, 24, 16, 2), (34, 20, 32, 12, 8, 4), (1024, 1024, 128, 128, 8, 8)]


def _flags(T, ids):
    return [1 if t in ids else 0 for t in range(T)]


# ---- symbols -----------------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_agree_on_the_new_symbols(built_lib):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdtile.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(mdtile_[a-z0-9_]+)\s*\(", src))
    lib = ctypes.CDLL(built_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared, f"{name} is not declared in include/mdtile.h"
        assert hasattr(lib, name), f"libmdtile.so does not export {name}"
        assert name in built_lib.exported_symbols(), f"the binding has no signature for {name}"
    assert sorted(built_lib.exported_symbols()) == sorted(declared)


# ---- the sparse plan ---------------------------------------------------------------------------------------------------------
def test_the_restatement_grid_is_the_plain_plan(built_lib):
    for geom in GEOMETRIES:
        g, plan = sr.grid(*geom), built_lib.Plan(*geom)
        assert plan.bboxes == list(g.boxes) and (plan.cols, plan.rows, plan.tile_bs, plan.num_batches) == (g.cols, g.rows, g.tile_bs, len(g.batches))
        assert not plan.sparse and plan.active_ids == () and built_lib.lib().mdtile_plan_active(plan.handle, None) == 0
    g = sr.grid(37, 20, 16, 12, 6, 4)
    assert (g.xs, g.ys) == ((0, 7, 14, 21), (0, 4, 8))      # literal numbers, so that the restatement is not pinned to itself alone
    g = sr.grid(34, 20, 32, 12, 8, 4)                       # the second tile column starts 2 px into the first quad, the last quad has 2 px
    assert (g.xs, g.ys, g.tw, g.th) == ((0, 2), (0, 4, 8), 32, 12)


@pytest.mark.parametrize("geom,ids,tile_bs", [
    ((37, 20, 16, 12, 6, 4), (0, 4, 8, 9, 10), 4),                  # ragged: 5 active tiles at tile_bs 4 -> 2 batches of 3 (3 + 2)
    ((37, 20, 16, 12, 6, 4), (11,), 4),
    ((37, 20, 16, 12, 6, 4), tuple(range(12)), 5),                  # Ta == T is allowed
    ((64, 24, 32, 32, 16, 3), (0, 2), 3),
    ((40, 24, 24, 24, 16, 2), (0, 1, 2), 2),
    ((34, 20, 32, 12, 8, 4), (1, 2, 5), 4),
    ((1024, 1024, 128, 128, 8, 8), (0, 1, 9, 10, 40, 41, 49, 50, 80), 8),
], ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_subset_matches_the_restatement(built_lib, geom, ids, tile_bs):
    E = built_lib
    g = sr.grid(*geom)
    T = len(g.boxes)
    parent = E.Plan(*geom)
    want = sr.subset(g, _flags(T, ids), tile_bs)
    sub = parent.subset(_flags(T, ids), tile_bs)
    assert sub.sparse and not parent.sparse
    assert sub.active_ids == want.active_ids == ids
    assert sub.bboxes == list(want.boxes)
    assert (sub.num_batches, sub.tile_bs) == (len(want.batches), want.tile_bs)
    assert sub.batches == [[g.boxes[t] for t in b] for b in want.batches]
    assert (sub.num_tiles, sub.parent_tiles, sub.w, sub.h) == (len(ids), T, parent.w, parent.h)
    info = (c_int * 8)()
    assert E.lib().mdtile_plan_info(sub.handle, info) == 0
    assert list(info) == [g.cols, g.rows, len(ids), len(want.batches), want.tile_bs, g.tw, g.th, g.ov]
    buf = (c_int * len(ids))()
    assert E.lib().mdtile_plan_active(sub.handle, buf) == len(ids) and tuple(buf) == ids
    # the parent is what it was, and the sparse plan does not need it
    assert parent.num_tiles == T and parent.bboxes == list(g.boxes)
    del parent
    assert E.lib().mdtile_plan_info(sub.handle, info) == 0 and info[2] == len(ids)
    boxes = (c_int * (4 * len(ids)))()
    assert E.lib().mdtile_plan_bboxes(sub.handle, boxes) == 0
    assert [tuple(boxes[4 * i:4 * i + 4]) for i in range(len(ids))] == list(want.boxes)


def test_the_ragged_case_is_ragged():
    want = sr.subset(sr.grid(37, 20, 16, 12, 6, 4), _flags(12, (0, 4, 8, 9, 10)), 4)
    assert want.tile_bs == 3 and [len(b) for b in want.batches] == [3, 2]


def test_subset_refusals_name_the_reason(built_lib):
    E = built_lib
    L = E.lib()
    parent = E.Plan(37, 20, 16, 12, 6, 4)
    none = (c_int * 12)()
    assert L.mdtile_plan_create_subset(parent.handle, none, 4) is None
    assert b"Ta == 0" in L.mdtile_last_error()
    with pytest.raises(E.MdtileError, match="no active tile"):
        parent.subset([0] * 12, 4)
    wrap = E.Plan(37, 20, 16, 12, 6, 4, wrap_x=True)
    flags = (c_int * wrap.num_tiles)(*([1] * wrap.num_tiles))
    assert L.mdtile_plan_create_subset(wrap.handle, flags, 4) is None
    assert b"wrap-x" in L.mdtile_last_error()
    torus = E.Plan(37, 22, 16, 12, 6, 4, wrap_x=True, wrap_y=True)
    with pytest.raises(E.MdtileError, match="torus"):
        torus.subset([1] * torus.num_tiles, 4)
    sub = parent.subset(_flags(12, (1, 2)), 4)
    assert L.mdtile_plan_create_subset(sub.handle, (c_int * 12)(*([1] * 12)), 4) is None
    assert b"sparse plan" in L.mdtile_last_error()
    with pytest.raises(E.MdtileError, match="sparse plan"):
        sub.subset([1] * 12, 4)
    with pytest.raises(E.MdtileError, match="flags for 12 tiles"):
        parent.subset([1] * 5, 4)
    # more batches than the kernel arguments carry: 81 active tiles at tile_bs 1 fit (81 <= 320), 400 of a finer grid do not
    big = E.Plan(1024, 1024, 64, 64, 8, 1)
    assert big.num_tiles > E.MAX_BATCHES
    with pytest.raises(E.MdtileError, match="MDTILE_MAX_BATCHES"):
        big.subset([1] * big.num_tiles, 1)
    assert big.subset([1] * big.num_tiles, 2).num_batches == (big.num_tiles + 1) // 2


# ---- what a sparse plan refuses ----------------------------------------------------------------------------------------------
def test_a_sparse_plan_refuses_the_full_grid_calls_by_name(built_lib):
    """Every refusal is an argument check in front of the first device call: it needs no GPU and the (fake) pointers are never followed."""
    E = built_lib
    L = E.lib()
    sub = E.Plan(37, 20, 16, 12, 6, 4).subset(_flags(12, (0, 4, 8, 9, 10)), 4)
    from mdtile import _BlendArgs, _Region
    a = _BlendArgs(E.METHOD_MD, E.DT_F32, 2, 4, 0, 0, 0, 0, 0, 64, 0, 0, 64)
    ptrs = (ctypes.c_void_p * 2)(64, 64)
    regions = (_Region * 1)()

    def refused(rc, *words):
        text = L.mdtile_last_error().decode()
        assert rc == E.E_ARG, (rc, text)
        for w in words:
            assert w in text, text

    refused(L.mdtile_blend(sub.handle, ctypes.byref(a), ptrs, 2, regions, 0, None), "mdtile_blend:", "sparse plan", "mdtile_blend_sparse")
    refused(L.mdtile_blend_finalize(sub.handle, ctypes.byref(a), 64, regions, 0, None), "mdtile_blend_finalize", "sparse plan")
    refused(L.mdtile_gather_range(sub.handle, E.DT_F32, 2, 4, 64, 64, 0, 5, None), "mdtile_gather_range", "sparse plan")
    info = (c_int * 8)()
    refused(L.mdtile_blend_dispatch(sub.handle, E.DT_F32, 2, 4, 0, 2, 1, 0, 0, info), "mdtile_blend_dispatch", "sparse plan")
    refused(L.mdtile_weight_map_add_grid(sub.handle, None, 64, None), "mdtile_weight_map_add_grid", "sparse plan", "parent")
    refused(L.mdtile_tile_activity(sub.handle, 64, 1, 64, None), "mdtile_tile_activity", "sparse plan")
    with pytest.raises(E.MdtileError, match="sparse plan"):
        E.blend_dispatch(sub, torch.float32, 2, 4)
    # mdtile_blend_sparse itself: a full plan, flags, a row band, a missing fill, the wrong number of batches
    full = E.Plan(37, 20, 16, 12, 6, 4)
    refused(L.mdtile_blend_sparse(full.handle, ctypes.byref(a), ptrs, 2, 64, None), "not a sparse plan")
    flagged = _BlendArgs(E.METHOD_MD, E.DT_F32, 2, 4, E.BLEND_PARTIAL, 0, 0, 0, 0, 64, 0, 0, 64)
    refused(L.mdtile_blend_sparse(sub.handle, ctypes.byref(flagged), ptrs, 2, 64, None), "flags")
    band = _BlendArgs(E.METHOD_MD, E.DT_F32, 2, 4, 0, 0, 0, 0, 8, 64, 0, 0, 64)
    refused(L.mdtile_blend_sparse(sub.handle, ctypes.byref(band), ptrs, 2, 64, None), "row band")
    refused(L.mdtile_blend_sparse(sub.handle, ctypes.byref(a), ptrs, 2, None, None), "fill")
    refused(L.mdtile_blend_sparse(sub.handle, ctypes.byref(a), ptrs, 1, 64, None), "1 batches given, the sparse plan has 2")
    mod = _BlendArgs(E.METHOD_MOD, E.DT_F32, 2, 4, 0, 0, 0, 0, 0, 64, 0, 0, 64)
    refused(L.mdtile_blend_sparse(sub.handle, ctypes.byref(mod), ptrs, 2, 64, None), "d_tile_w and d_rescale")
    wrap = E.Plan(37, 20, 16, 12, 6, 4, wrap_x=True)
    refused(L.mdtile_tile_activity(wrap.handle, 64, 1, 64, None), "wrap-x")
    # the full plan is untouched by all this
    assert E.blend_dispatch(full, torch.float32, 2, 4).kernel in (E.BLEND_KERNEL_PLAIN, E.BLEND_KERNEL_LDS)


def test_the_binding_checks_before_the_device(built_lib):
    E = built_lib
    full = E.Plan(37, 20, 16, 12, 6, 4)
    with pytest.raises(E.MdtileError, match="no CPU fallback"):
        E.tile_activity(full, torch.zeros(1, 20, 37))
    with pytest.raises(E.MdtileError, match="needs a sparse plan"):
        E.blend_sparse(full, E.METHOD_MD, [], 2, 4, fill=torch.zeros(2, 4, 20, 37), dtype=torch.float32, device="cpu")


# ---- restatement: activity and liveness ---------------------------------------------------------------------------------------
def test_activity_and_liveness_of_the_restatement():
    g = sr.grid(37, 20, 16, 12, 6, 4)
    m = np.zeros((2, 20, 37), np.float32)
    assert sr.activity(g, m) == [0] * 12
    m[0, 3, 5] = -0.0
    assert sr.activity(g, m) == [0] * 12, "-0.0 is equal to zero"
    m[1, 0, 0] = np.nan
    assert sr.activity(g, m) == _flags(12, (0,)), "NaN is not equal to zero"
    m[1, 0, 0], m[0, 19, 36] = 0, np.float32(1.4e-45)
    assert sr.activity(g, m) == _flags(12, (11,)), "a denormal is not equal to zero"
    live = sr.live_map(g, _flags(12, (11,)))
    # tile 11 = (21, 8, 16, 12); tile 10 reaches x = 29 and tile 7 reaches y = 15: tile 11 alone covers x >= 30, y >= 16
    assert live[16:, 30:].all() and int(live.sum()) == 4 * 7
    # a pixel with a non-zero mask is live: every tile that covers it holds that pixel, so every one of them is active
    rng = np.random.default_rng(0)
    for _ in range(20):
        m = (rng.random((1, 20, 37)) < 0.01).astype(np.float32)
        act = sr.activity(g, m)
        assert sr.live_map(g, act)[m[0] != 0].all()


# ---- the option --------------------------------------------------------------------------------------------------------------
def test_preload_option(host):
    pl, shared = host
    parser = argparse.ArgumentParser()
    load_preload().preload(parser)
    assert parser.parse_args([]).mdtile_inpaint_skip is False
    assert parser.parse_args(["--mdtile-inpaint-skip"]).mdtile_inpaint_skip is True
    A = pl.abstractdiffusion.AbstractDiffusion
    if hasattr(shared.cmd_opts, "mdtile_inpaint_skip"):
        del shared.cmd_opts.mdtile_inpaint_skip
    assert A.inpaint_skip_requested() is False          # a host that never heard of the option
    try:
        shared.cmd_opts.mdtile_inpaint_skip = True
        assert A.inpaint_skip_requested() is True
        shared.cmd_opts.mdtile_inpaint_skip = False
        assert A.inpaint_skip_requested() is False
    finally:
        del shared.cmd_opts.mdtile_inpaint_skip


# ---- the delegate's decision, on the torch doubles of the engine ----------------------------------------------------------------------
@pytest.fixture
def skip_option(wired):
    pl, shared = wired
    shared.cmd_opts.mdtile_inpaint_skip = True
    try:
        yield pl, shared
    finally:
        if hasattr(shared.cmd_opts, "mdtile_inpaint_skip"):
            del shared.cmd_opts.mdtile_inpaint_skip


@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_decision_and_the_batch_limit(skip_option, monkeypatch, capsys, method):
    """The delegate's choice of plan with mdtile.tile_activity replaced by the restatement's slice test (Plan.subset needs no device): a partial
    mask gives the sparse plan; more active batches than a sparse plan carries keep the full plan with one line that names the limit -- the
    library's refusal never becomes a failed job."""
    pl, shared = skip_option
    geom = (168, 168, 16, 16, 8)
    g = sr.grid(*geom, 1)
    monkeypatch.setattr(pl.engine, "tile_activity", lambda plan, mask: sr.activity(g, mask.numpy()))
    nmask = np.ones((4, g.H, g.W), np.float32)
    nmask[:, :24, :24] = 0.0
    assert sum(sr.activity(g, nmask)) == 396 > pl.engine.MAX_BATCHES
    d, p = delegate(pl, *geom, 1, method)
    p.nmask = torch.from_numpy(nmask)
    capsys.readouterr()
    assert d.inpaint_skip() == "full" and d.inpaint_skip() == "full" and d.sparse_plan is None
    out = capsys.readouterr().out
    assert "inpaint mask touches 396 of 400 tiles" in out
    assert out.count("--mdtile-inpaint-skip not applied") == 1 and "396 batches" in out and str(pl.engine.MAX_BATCHES) in out
    d, p = delegate(pl, *geom, 2, method)
    p.nmask = torch.from_numpy(nmask)
    assert d.inpaint_skip() == "sparse" and d.sparse_plan.num_batches == 198 and d.total_bboxes == 198
    assert [len(b) for b in d.sparse_batched_bboxes] == [2] * 198
    assert "not applied" not in capsys.readouterr().out
    shared.cmd_opts.mdtile_inpaint_skip = False          # option off: nothing is read, nothing is printed
    d, p = delegate(pl, *geom, 2, method)
    p.nmask = torch.from_numpy(nmask)
    assert d.inpaint_skip() == "full" and d.skip_mode is None and capsys.readouterr().out == ""


def test_demofusion_says_once_that_it_runs_every_window(skip_option, capsys):
    pl, shared = skip_option
    capsys.readouterr()
    d = pl.demofusion.DemoFusion(sh.make_processing(320, 192), sh.kdiff_sampler())
    out = capsys.readouterr().out
    assert out.count("--mdtile-inpaint-skip not applied") == 1 and "DemoFusion" in out
    d._skip_note("DemoFusion runs its own window schedule")
    assert capsys.readouterr().out == ""
    del shared.cmd_opts.mdtile_inpaint_skip
    pl.demofusion.DemoFusion(sh.make_processing(320, 192), sh.kdiff_sampler())
    assert "inpaint" not in capsys.readouterr().out
