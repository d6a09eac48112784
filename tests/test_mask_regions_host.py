"""Free-form mask regions without a GPU: the restatement tests/mask_region_ref.py against the existing oracle and upstream's
feather_mask; the cover rule at its threshold, the box and the count; the header, the exports and the binding; the option, the `p` attribute and
every refusal by name on the CPU stub host with the engine's calls replaced by doubles.  The kernels are tested in tests/test_gpu_mask_regions.py."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

from oracle import blend_oracle as bo

import mask_region_cases as cases
import mask_region_ref as rr
from wrap_common import host, wired, delegate, load_preload, assert_bitwise      # noqa: F401  (host, wired: fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mdtile_mask_cover_u8", "mdtile_mask_region", "mdtile_blend_mask_regions", "mdtile_region_noise_masked"]
W, H, TILE, OV, BS = 40, 24, 16, 8, 4
N, C = 2, 4


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draw_background", [True, False])
@pytest.mark.parametrize("method", ["md", "mod"])
def test_with_whole_rectangles_it_is_the_oracle(method, draw_background):
    """All-ones covers (and None): the restatement is oracle/blend_oracle.py's region blend bit for bit, BG and FG regions, with and without the grid."""
    regions = [bo.Region(2, 1, 13, 9, bo.BG), bo.Region(10, 6, 12, 8, bo.BG), bo.Region(18, 1, 10, 10, bo.FG, 0.3), bo.Region(20, 3, 10, 10, bo.FG, 0.5),
               bo.Region(31, 17, 9, 7, bo.FG, 0.2), bo.Region(33, 0, 1, 1, bo.BG)]
    o = bo.BlendOracle(method, W, H, TILE, TILE, OV, BS, regions, draw_background)
    torch.manual_seed(1)
    x = torch.randn(N, C, H, W)
    want = o.evaluate(x, bo.synthetic_denoiser, bo.synthetic_region_denoiser)
    tiles = torch.cat([bo.synthetic_denoiser(o.gather(x, b)) for b in o.batches], dim=0).numpy() if draw_background else None
    boxes = [b for batch in o.batches for b in batch]
    for ones in (False, True):
        ref = []
        for i, r in enumerate(regions):
            wgt = o.feather[i] if r.blend_mode == bo.FG else (o.custom_weights[i][0, 0] if method == "mod" else None)
            ref.append(rr.Region(r.x, r.y, r.w, r.h, "fg" if r.blend_mode == bo.FG else "bg", bo.synthetic_region_denoiser(x[r.sl], i).numpy(),
                                 None if wgt is None else wgt.numpy(), np.ones((r.h, r.w), np.uint8) if ones else None))
        got = rr.blend(W, H, boxes, method, tiles, N, C, ref, o.weights[0, 0].numpy(), o.tile_weights.numpy() if method == "mod" else None,
                       o.rescale[0, 0].numpy() if method == "mod" else None)
        assert_bitwise(torch.from_numpy(got), want, f"{method} background={draw_background} ones={ones}")
        # and the maps, built the way the delegates build them
        grid_w = bo.grid_weight_map(W, H, boxes, o.tile_weights)[0, 0].numpy() if draw_background else np.zeros((H, W), np.float32)
        gauss = [bo.gaussian_weights(r.w, r.h).numpy() for r in regions]
        weights = rr.weight_sum(grid_w, method, ref, gauss)
        assert_bitwise(torch.from_numpy(weights), o.weights[0, 0], "the weight sum")
        if method == "mod":
            for i, R in enumerate(ref):
                if R.mode == "bg":
                    assert_bitwise(torch.from_numpy(rr.premultiplied(gauss[i], R, o.rescale[0, 0].numpy())), o.custom_weights[i][0, 0], f"region {i}")


def test_noise_with_whole_rectangles_is_the_plain_noise():
    import wrap_region_ref as plain
    torch.manual_seed(2)
    noise = torch.randn(N, C, H, W).numpy()
    regions = [(x, y, w, h, mode, torch.randn(1, C, h, w).numpy()) for (_, x, y, w, h, mode, _) in cases.spec(W, H)]
    got = rr.region_noise(noise, [r + (None,) for r in regions])
    assert np.array_equal(got.view(np.int32), plain.region_noise(noise, regions).view(np.int32))
    masked = rr.region_noise(noise, [r + (c[6],) for r, c in zip(regions, cases.spec(W, H))])
    assert not np.array_equal(masked, got)
    # under a pixel no region covers, the job's noise stays
    painted = np.zeros((H, W), bool)
    for (_, x, y, w, h, _, cover) in cases.spec(W, H):
        painted[y:y + h, x:x + w] |= np.ones((h, w), bool) if cover is None else cover != 0
    assert np.array_equal(masked[:, :, ~painted], noise[:, :, ~painted]) and (masked[:, :, painted] != noise[:, :, painted]).all()


@pytest.mark.parametrize("w,h", [(8, 6), (14, 10), (12, 12), (2, 2), (30, 4)])
@pytest.mark.parametrize("ratio", [0.0, 0.2, 0.5, 1.0])
def test_feather_of_a_full_even_rectangle_is_upstreams(w, h, ratio):
    assert_bitwise(torch.from_numpy(rr.feather(np.ones((h, w), np.uint8), ratio)), bo.feather_mask(w, h, ratio), f"{w}x{h}@{ratio}")


def test_feather_against_the_golden_maps(golden_maps):
    seen = 0
    for key in golden_maps.files:
        m = re.fullmatch(r"feather_(\d+)x(\d+)_([0-9.]+)", key)
        if m and int(m.group(1)) % 2 == 0 and int(m.group(2)) % 2 == 0:
            w, h, r = int(m.group(1)), int(m.group(2)), float(m.group(3))
            assert np.array_equal(rr.feather(np.ones((h, w), np.uint8), r).view(np.int32), golden_maps[key].astype(np.float32).view(np.int32)), key
            seen += 1
    assert seen > 0


def test_odd_sizes_differ_on_the_middle_column_only():
    """9 x 8 at ratio 0.5 (R = 2): upstream's quadrant loop leaves the middle column at 1.0, the distance form feathers it like its neighbours."""
    mine, up = rr.feather(np.ones((8, 9), np.uint8), 0.5), bo.feather_mask(9, 8, 0.5).numpy()
    diff = mine.view(np.int32) != up.view(np.int32)
    assert sorted(set(np.nonzero(diff)[1])) == [4] and sorted(np.nonzero(diff)[0]) == [0, 1, 6, 7]
    assert (up[:, 4] == 1.0).all() and list(mine[:, 4]) == [0.0, 0.25, 1.0, 1.0, 1.0, 1.0, 0.25, 0.0]


def test_cover_rule_at_the_threshold():
    cover, box = rr.cover_u8(np.array([[255, 255, 255, 254], [0, 0, 0, 0]], np.uint8), 2, 1)
    assert cover.tolist() == [[1, 0]] and box == [0, 0, 1, 1, 1]
    assert rr.cover_u8(np.array([[255, 0], [255, 0]], np.uint8), 1, 1)[0].tolist() == [[1]]       # 2 * 510 >= 255 * 4
    assert rr.cover_u8(np.array([[255, 0], [254, 0]], np.uint8), 1, 1)[0].tolist() == [[0]]
    assert rr.cover_u8(np.array([[128]], np.uint8), 1, 1)[0].tolist() == [[1]] and rr.cover_u8(np.array([[127]], np.uint8), 1, 1)[0].tolist() == [[0]]


def test_boxes_and_counts():
    cover, box = rr.cover_u8(np.zeros((16, 24), np.uint8), 6, 4)
    assert not cover.any() and box == [0, 0, 0, 0, 0]
    cover, box = rr.cover_u8(np.full((16, 24), 255, np.uint8), 6, 4)
    assert cover.all() and box == [0, 0, 6, 4, 24]
    m = np.zeros((16, 24), np.uint8)
    m[12:, 20:] = 255
    assert rr.cover_u8(m, 6, 4)[1] == [5, 3, 6, 4, 1]
    m[0:4, 4:12] = 255
    assert rr.cover_u8(m, 6, 4)[1] == [1, 0, 6, 4, 3]
    # ragged boxes: 7 rows over 3 cells own 2, 2 and 3 rows (integer division)
    m = np.zeros((7, 3), np.uint8)
    m[4:] = 255
    assert rr.cover_u8(m, 3, 3)[0].tolist() == [[0, 0, 0], [0, 0, 0], [1, 1, 1]]
    m[2:4] = 255
    assert rr.cover_u8(m, 3, 3)[0].tolist() == [[0, 0, 0], [1, 1, 1], [1, 1, 1]]
    c = cases.canvas_cover(W, H)
    assert rr.box_of(c)[4] == int(c.sum()) and rr.box_of(c)[2] == W
    k = rr.chessboard(np.ones((5, 7), np.uint8))
    assert k.tolist() == [[1] * 7, [1, 2, 2, 2, 2, 2, 1], [1, 2, 3, 3, 3, 2, 1], [1, 2, 2, 2, 2, 2, 1], [1] * 7]
    hole = np.ones((5, 7), np.uint8)
    hole[2, 3] = 0
    assert rr.chessboard(hole)[2].tolist() == [1, 2, 1, 0, 1, 2, 1]


# ---- symbols --------------------------------------------------------------------------------------------------------------------------
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
    fields = re.search(r"struct mdtile_mask_region \{(.*?)\};", src, flags=re.S).group(1)
    assert [f.split()[-1].lstrip("*") for f in fields.split(";") if f.strip()] == [n for n, _ in built_lib._MaskRegion._fields_]
    assert ctypes.sizeof(built_lib._MaskRegion) == ctypes.sizeof(built_lib._Region) + 8
    assert lib.mdtile_version() == 100
    for fn in ("mask_cover_u8", "mask_region", "blend_mask_regions", "region_noise_masked"):
        assert callable(getattr(built_lib, fn))
    assert built_lib.RegionSpec(0, 0, 1, 1, 0, None).cover is None
    assert not re.search(r"getenv\(\"MDTILE_", open(os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd", "csrc", "mask_regions.hip")).read())


def test_no_cpu_fallback(built_lib):
    """The new calls take device tensors only, as their neighbours."""
    with pytest.raises((AssertionError, built_lib.MdtileError, RuntimeError)):
        built_lib.mask_cover_u8(torch.zeros(8, 8, dtype=torch.uint8), 4, 4)
    with pytest.raises((AssertionError, built_lib.MdtileError, RuntimeError)):
        built_lib.mask_region(torch.zeros(8, 8, dtype=torch.uint8), 0, 0, 4, 4, 0.2)
    with pytest.raises((AssertionError, built_lib.MdtileError, RuntimeError)):
        built_lib.region_noise_masked(torch.zeros(1, 4, 8, 8), [])


def test_sharded_blend_refuses_a_cover(built_lib):
    from mdtile import sharding
    with pytest.raises(built_lib.MdtileError, match="ShardedBlend: region 1 has a cover"):
        sharding.ShardedBlend(None, W, H, TILE, TILE, OV, BS, built_lib.METHOD_MD,
                              regions=[(0, 0, 4, 4, built_lib.REGION_BG, 0.2, None), (0, 0, 4, 4, built_lib.REGION_BG, 0.2, torch.ones(4, 4, dtype=torch.uint8))])


# ---- the option and the plumbing on the stub host -----------------------------------------------------------------------------------------
@pytest.fixture
def masks(wired, monkeypatch, tmp_path):
    """(plugin, shared, calls, folder): the engine's mask, rect and blend calls replaced by doubles that compute with the restatement and record
    themselves; every option this file sets is gone before and after."""
    pl, shared = wired
    names = ("mdtile_region_masks", "mdtile_grid_jitter", "mdtile_jitter_regions", "mdtile_wrap_regions", "mdtile_wrap_x", "mdtile_wrap_y")

    def clear():
        for name in names:
            if hasattr(shared.cmd_opts, name):
                delattr(shared.cmd_opts, name)
    clear()
    calls = []

    def mask_cover_u8(mask, w, h):
        calls.append(("mask_cover_u8", tuple(mask.shape), w, h))
        assert mask.dtype == torch.uint8
        if mask.shape[0] < h or mask.shape[1] < w:
            raise pl.engine.MdtileError("smaller")
        cover, box = rr.cover_u8(mask.numpy(), w, h)
        return torch.from_numpy(cover), torch.tensor(box, dtype=torch.int32)

    def mask_region(cover, x, y, w, h, ratio=None):
        calls.append(("mask_region", x, y, w, h, ratio))
        rc, f = rr.region_tensors(cover.numpy(), x, y, w, h, ratio)
        return torch.from_numpy(rc), None if f is None else torch.from_numpy(f)

    def add_rect(weights, x, y, w, h, rect_w=None, scalar=1.0):
        calls.append(("add_rect", x, y, w, h, None if rect_w is None else rect_w.clone()))
        weights.view(weights.shape[-2], weights.shape[-1])[y:y + h, x:x + w] += scalar if rect_w is None else rect_w.view(h, w)

    def blend_mask_regions(plan, method, batch_out, N_, C_, *, regions, **kw):
        calls.append(("blend_mask_regions", [(r.x, r.y, r.w, r.h, r.mode, r.cover) for r in regions], len(batch_out)))
        return torch.zeros(N_, C_, plan.h, plan.w)

    def blend(plan, method, batch_out, N_, C_, *, regions=(), **kw):
        calls.append(("blend", [(r.x, r.y, r.w, r.h, r.mode, r.cover) for r in regions], len(batch_out)))
        return torch.zeros(N_, C_, plan.h, plan.w)

    E = pl.engine
    monkeypatch.setattr(E, "mask_cover_u8", mask_cover_u8)
    monkeypatch.setattr(E, "mask_region", mask_region)
    monkeypatch.setattr(E, "weight_map_add_rect", add_rect)
    monkeypatch.setattr(E, "blend_mask_regions", blend_mask_regions)
    monkeypatch.setattr(E, "blend", blend)
    monkeypatch.setattr(E, "gather_all", lambda plan, x_in, out=None: [torch.cat([x_in[:, :, y:y + h, x:x + w] for (x, y, w, h) in b]) for b in plan.batches])
    monkeypatch.setattr(E, "gather_rect", lambda x_in, x, y, w, h: x_in[:, :, y:y + h, x:x + w].contiguous())
    monkeypatch.setattr(E, "reciprocal", lambda t: 1.0 / t)
    monkeypatch.setattr(E, "rect_mul_canvas", lambda rect_w, canvas, x, y, w, h: rect_w.mul_(canvas.view(canvas.shape[-2], canvas.shape[-1])[y:y + h, x:x + w]))
    monkeypatch.setattr(E, "gaussian_weights", lambda w, h, dev=None: bo.gaussian_weights(w, h))
    monkeypatch.setattr(pl.utils, "feather_mask", lambda w, h, ratio: bo.feather_mask(w, h, ratio))
    monkeypatch.setattr(shared.state, "sampling_step", 0)
    yield pl, shared, calls, tmp_path
    clear()


def _settings(pl, *regions):
    return {i: pl.utils.BBoxSettings(True, fx, fy, fw, fh, "", "", mode, 0.3, 11 + i) for i, (fx, fy, fw, fh, mode) in enumerate(regions)}


THREE = ((0.9, 0.9, 0.05, 0.05, "Background"), (0.2, 0.1, 0.6, 0.5, "Background"), (0.0, 0.0, 0.1, 0.1, "Foreground"))


def _save(folder, k, cover, value=255, scale=8):
    Image.fromarray((np.kron(cover, np.ones((scale, scale), np.uint8)) * value).astype(np.uint8), "L").save(os.path.join(folder, f"region{k}.png"))


def test_preload_option(masks):
    pl, shared, _, folder = masks
    parser = argparse.ArgumentParser()
    load_preload().preload(parser)
    assert parser.parse_args([]).mdtile_region_masks is None
    assert parser.parse_args(["--mdtile-region-masks", str(folder)]).mdtile_region_masks == str(folder)
    text = parser.format_help()
    for word in ("--mdtile-region-masks", "region<k>.png", "p.mdtile_region_masks", "--mdtile-wrap-x", "Noise Inversion", "--mdtile-jitter-regions",
                 "--mdtile-inpaint-skip", "ShardedBlend", "smaller than the latent canvas"):
        assert word in re.sub(r"\s+", " ", text), word


@pytest.mark.parametrize("method", ["md", "mod"])
def test_directory_masks_reach_the_delegate(masks, method):
    pl, shared, calls, folder = masks
    cov = cases.canvas_cover(W, H)
    _save(folder, 1, cov)
    _save(folder, 3, np.flipud(cov), value=200)
    shared.cmd_opts.mdtile_region_masks = str(folder)
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS, method)
    if method == "mod":
        d.get_weight = lambda w, h: bo.gaussian_weights(w, h)
    d.init_custom_bbox(_settings(pl, *THREE), True, False)
    assert d.mask_regions and not d.jitter_regions and not d.wrap_regions
    b1, b3 = rr.box_of(cov), rr.box_of(np.flipud(cov))
    want = [(b1[0], b1[1], b1[2] - b1[0], b1[3] - b1[1]), (8, 2, 24, 12), (b3[0], b3[1], b3[2] - b3[0], b3[3] - b3[1])]
    assert [(b.x, b.y, b.w, b.h) for b in d.custom_bboxes] == want and [b.index for b in d.custom_bboxes] == [0, 1, 2]
    rc1, _ = rr.region_tensors(cov, *want[0], None)
    rc3, f3 = rr.region_tensors(np.flipud(cov), *want[2], 0.3)
    assert np.array_equal(d.custom_bboxes[0].cover.numpy(), rc1) and d.custom_bboxes[1].cover is None and np.array_equal(d.custom_bboxes[2].cover.numpy(), rc3)
    assert d.custom_bboxes[0].feather_mask is None and np.array_equal(d.custom_bboxes[2].feather_mask.numpy().view(np.int32), f3.view(np.int32))
    assert [c[:1] + c[1:5] for c in calls if c[0] == "mask_region"] == [("mask_region", *want[0]), ("mask_region", *want[2])]
    assert [c[5] for c in calls if c[0] == "mask_region"] == [None, 0.3], "a feather is made for the FG region only, with its own ratio"
    assert [c[1:4] for c in calls if c[0] == "mask_cover_u8"] == [((8 * H, 8 * W), W, H)] * 2
    # the weight sums: the cover as 0.0 / 1.0 (md), gaussian * cover (mod); the rectangle as before
    adds = [c for c in calls if c[0] == "add_rect"]
    assert [a[1:5] for a in adds] == [want[0], want[1]]
    if method == "md":
        assert torch.equal(adds[0][5], torch.from_numpy(rc1).float()) and adds[1][5] is None
    else:
        assert torch.equal(adds[0][5], bo.gaussian_weights(want[0][2], want[0][3]) * torch.from_numpy(rc1).float())
        assert torch.equal(adds[1][5], bo.gaussian_weights(24, 12))
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    d.update_pbar = lambda: None
    specs = d.region_specs([torch.zeros(N, C, b.h, b.w) for b in d.custom_bboxes])
    assert [s.cover is None for s in specs] == [False, True, False]
    x = torch.randn(N, C, H, W)
    if method == "md":
        d.sample_one_step(x, None, lambda xt, b: xt, lambda xt, i, b: xt)
    else:
        shared.sd_model.apply_model_original_md = lambda x_, t_, c_: x_
        d.custom_apply_model = lambda xt, t_in, c_in, i, b: xt
        d.apply_model_hijack(x, torch.zeros(N), {"c_crossattn": [torch.zeros(N, 77, 768)], "c_concat": [torch.zeros(N, 5, 1, 1)]})
    blends = [c for c in calls if c[0] in ("blend", "blend_mask_regions")]
    assert [c[0] for c in blends] == ["blend_mask_regions"] and blends[0][2] == d.plan.num_batches
    assert [r[:4] for r in blends[0][1]] == want


def test_a_job_without_masks_makes_the_calls_of_before(masks):
    pl, shared, calls, folder = masks
    shared.cmd_opts.mdtile_region_masks = str(folder)      # an empty directory
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    d.init_custom_bbox(_settings(pl, *THREE), True, False)
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    d.update_pbar = lambda: None
    assert not d.mask_regions and [(b.x, b.y, b.w, b.h) for b in d.custom_bboxes] == [(36, 21, 2, 2), (8, 2, 24, 12), (0, 0, 4, 3)]
    d.sample_one_step(torch.randn(N, C, H, W), None, lambda xt, b: xt, lambda xt, i, b: xt)
    assert [c[0] for c in calls if c[0].startswith(("mask", "blend"))] == ["blend"]
    assert all(r[5] is None for c in calls if c[0] == "blend" for r in c[1])


def test_the_attribute_wins_and_an_empty_mask_drops_the_region(masks, capsys):
    pl, shared, calls, folder = masks
    cov = cases.canvas_cover(W, H)
    _save(folder, 1, cov)
    shared.cmd_opts.mdtile_region_masks = str(folder)
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    island = np.zeros((H, W), np.uint8)
    island[5:9, 30:37] = 1
    other = os.path.join(folder, "painted.png")
    Image.fromarray((np.kron(island, np.ones((8, 8), np.uint8)) * 255).astype(np.uint8), "L").save(other)
    p.mdtile_region_masks = {1: other, 3: Image.fromarray(np.zeros((8 * H, 8 * W), np.uint8), "L")}
    assert {i: n for i, (_, n) in pl.utils.region_mask_sources(p, [0, 1, 2]).items()} == {0: "painted.png", 2: "<image>"}
    capsys.readouterr()
    d.init_custom_bbox(_settings(pl, *THREE), True, False)
    out = capsys.readouterr().out
    assert out.count("[Tiled Diffusion]") == 1 and "region 3 dropped" in out and "covers no pixel" in out
    assert [(b.x, b.y, b.w, b.h, b.index) for b in d.custom_bboxes] == [(30, 5, 7, 4, 0), (8, 2, 24, 12, 1)]
    assert d.mask_region_indices == {0, 2}


def test_generation_parameters_record_the_masks_that_take_part(masks):
    """extra_generation_params names the mask of a region that is laid -- the file name, or "<image>" -- and nothing for a rectangle or for a
    region whose mask covered no pixel and was dropped."""
    pl, shared, calls, folder = masks
    _save(folder, 1, cases.canvas_cover(W, H))
    shared.cmd_opts.mdtile_region_masks = str(folder)
    settings = _settings(pl, *THREE, (0.5, 0.5, 0.2, 0.2, "Background"))
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    p.mdtile_region_masks = {3: Image.fromarray(np.zeros((8 * H, 8 * W), np.uint8), "L"),
                             4: Image.fromarray((np.kron(cases.canvas_cover(W, H), np.ones((8, 8), np.uint8)) * 255).astype(np.uint8), "L")}
    p.extra_generation_params = {"Tiled Diffusion": {"Region control": {f"Region {i + 1}": s._asdict() for i, s in settings.items()}}}
    d.init_custom_bbox(settings, True, False)
    rc = p.extra_generation_params["Tiled Diffusion"]["Region control"]
    assert rc["Region 1"]["mask"] == "region1.png" and rc["Region 4"]["mask"] == "<image>"
    assert "mask" not in rc["Region 2"] and "mask" not in rc["Region 3"]
    assert [b.index for b in d.custom_bboxes] == [0, 1, 3]


def test_generation_parameters_and_the_noise(masks, monkeypatch):
    """The script records the mask's name per region, and the noise hijack draws each masked region's noise for its bounding box and pastes it through
    region_noise_masked with the delegate's rectangle and cover."""
    pl, shared, calls, folder = masks
    from hostsim import stub_host as sh
    cov = cases.canvas_cover(W, H)
    _save(folder, 1, cov)
    shared.cmd_opts.mdtile_region_masks = str(folder)
    settings = _settings(pl, *THREE)
    p = sh.make_processing(W * 8, H * 8)
    p.mdtile_region_masks = {3: Image.fromarray(np.zeros((8 * H, 8 * W), np.uint8), "L")}
    names = pl.utils.region_mask_sources(p, list(settings))
    assert {i: n for i, (_, n) in names.items()} == {0: "region1.png", 2: "<image>"}
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    p.mdtile_region_masks = {3: Image.fromarray(np.zeros((8 * H, 8 * W), np.uint8), "L")}
    d.init_custom_bbox(settings, True, False)
    script = pl.tilediffusion.Script()
    script.delegate = d
    seen = []
    monkeypatch.setattr(pl.engine, "region_noise_masked", lambda noise, regions: seen.append(("masked", [(r[:5], tuple(r[5].shape), r[6]) for r in regions])))
    monkeypatch.setattr(pl.engine, "region_noise", lambda noise, regions: seen.append(("plain",)))
    monkeypatch.setattr(pl.tilediffusion.Script, "create_random_tensors_original_md", staticmethod(lambda shape, *a, **k: torch.zeros((1,) + tuple(shape))),
                        raising=False)
    info = {f"Region {i + 1}": {} for i in settings}
    script.create_random_tensors_hijack(settings, info, (C, H, W), [1])
    b1 = rr.box_of(cov)
    box = (b1[0], b1[1], b1[2] - b1[0], b1[3] - b1[1])
    assert len(seen) == 1 and seen[0][0] == "masked"
    (r0, s0, c0), (r1, s1, c1) = seen[0][1]
    assert r0 == box + (pl.engine.REGION_BG,) and s0 == (1, C, box[3], box[2]) and np.array_equal(c0.numpy(), rr.region_tensors(cov, *box, None)[0])
    assert r1 == (8, 2, 24, 12, pl.engine.REGION_BG) and s1 == (1, C, 12, 24) and c1 is None
    assert info["Region 1"]["seed"] == 11 and info["Region 2"]["seed"] == 12 and "seed" not in info["Region 3"], "the dropped region draws no noise"
    # noise of another size (a hires pass): a mask region has no rectangle there and draws none; the rectangle is laid by the rule, as before
    seen.clear()
    info = {f"Region {i + 1}": {} for i in settings}
    script.create_random_tensors_hijack(settings, info, (C, 2 * H, 2 * W), [1])
    assert seen == [("plain",)] and list(k for k, v in info.items() if "seed" in v) == ["Region 2"]


# ---- refused or set aside ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [("mdtile_wrap_x",), ("mdtile_wrap_y",), ("mdtile_wrap_x", "mdtile_wrap_regions"), ("mdtile_wrap_x", "mdtile_wrap_y", "mdtile_wrap_regions")])
def test_refused_on_a_canvas_that_wraps(masks, opts):
    pl, shared, calls, folder = masks
    _save(folder, 1, cases.canvas_cover(W, H))
    shared.cmd_opts.mdtile_region_masks = str(folder)
    for o in opts:
        setattr(shared.cmd_opts, o, True)
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    assert d.wrap_x or d.wrap_y
    with pytest.raises(RuntimeError, match=r"mask regions \(--mdtile-region-masks / p.mdtile_region_masks\) cannot be combined with --mdtile-wrap-[xy].*with or without --mdtile-wrap-regions"):
        d.init_custom_bbox(_settings(pl, *THREE), True, False)
    assert not d.custom_bboxes and not calls


def test_refused_with_noise_inversion(masks):
    pl, shared, calls, folder = masks
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    p.mdtile_region_masks = {2: Image.fromarray(np.full((8 * H, 8 * W), 255, np.uint8), "L")}
    d.noise_inverse_enabled = True
    with pytest.raises(RuntimeError, match="mask regions .* cannot be combined with Noise Inversion"):
        d.init_custom_bbox(_settings(pl, *THREE), True, False)
    assert not d.custom_bboxes and not calls


def test_refused_when_the_mask_is_smaller_than_the_latent_canvas(masks):
    pl, shared, calls, folder = masks
    for (mw, mh) in ((W - 1, 8 * H), (8 * W, H - 1)):
        d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
        p.mdtile_region_masks = {2: Image.fromarray(np.full((mh, mw), 255, np.uint8), "L")}
        with pytest.raises(RuntimeError, match=rf"the mask of region 2 \({mw} x {mh} px\) is smaller than the latent canvas \({W} x {H}\)"):
            d.init_custom_bbox(_settings(pl, *THREE), True, False)
    assert not [c for c in calls if c[0] == "mask_cover_u8"]


def test_the_fixed_grid_runs_under_jitter_regions(masks, capsys):
    pl, shared, calls, folder = masks
    shared.cmd_opts.mdtile_grid_jitter = shared.cmd_opts.mdtile_jitter_regions = True
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    assert d.grid_jitter
    p.mdtile_region_masks = {2: Image.fromarray((np.kron(cases.canvas_cover(W, H), np.ones((8, 8), np.uint8)) * 255).astype(np.uint8), "L")}
    capsys.readouterr()
    d.init_custom_bbox(_settings(pl, *THREE), True, False)
    assert d.mask_regions and not d.jitter_regions and d.region_w is None
    assert d.step_lattice(None, "full") is None and d.step_lattice(None, "full") is None
    out = capsys.readouterr().out
    assert out.count("--mdtile-grid-jitter not applied") == 1 and "a region is a painted mask" in out and "--mdtile-jitter-regions" in out
    # without a mask the same options keep the moving grid
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    d.init_custom_bbox(_settings(pl, *THREE), True, False)
    assert not d.mask_regions and d.jitter_regions


def test_inpaint_skip_stands_down_as_with_every_region_job(masks):
    pl, shared, calls, folder = masks
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS)
    p.mdtile_region_masks = {2: Image.fromarray(np.full((8 * H, 8 * W), 255, np.uint8), "L")}
    d.init_custom_bbox(_settings(pl, *THREE), True, False)
    assert d.mask_regions and d._decide_inpaint_skip() == "full"
