"""Tile skipping on the GPU (csrc/sparse.hip), BITWISE against the numpy restatement tests/sparse_ref.py and against the full
blend of the parent plan on the GPU: tile activity, the gather of the active tiles, mdtile_blend_sparse for MultiDiffusion / Mixture of Diffusers
in fp32, fp16 and bf16, poisoned tile outputs, special values in `fill`, and one model evaluation through both delegates with
--mdtile-inpaint-skip.  No tolerance appears in this file; half types follow tests/test_gpu_blend_matrix.py (inputs and tile outputs rounded to
the dtype, the fp32 restatement evaluated on those values, rounded once).  Every case runs N = 2, C = 4."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from hostsim import stub_host as sh

import sparse_ref as sr
from wrap_common import (DT, NAN, N, C, SPECIALS, bits, assert_bitwise as _assert_bitwise, tile_fn as _tile_fn, on_device as _on_device, maps as _maps,
                         make_delegate, set_options, take as _take)

pytestmark = pytest.mark.gpu

# id -> (W, H, requested tile_w, tile_h, overlap, tile_bs, misaligned batches)
CASES = {
    # odd origins (0, 7, 14, 21), W not a multiple of 4, a ragged last quad, three tile rows
    "odd37": (37, 20, 16, 12, 6, 4, False),
    # every origin a multiple of 4 (0, 16, 32; the tile is clamped to 32 x 24): every quad of an active tile on the vector path
    "aligned64": (64, 24, 32, 32, 16, 3, False),
    # three tile columns (0, 8, 16) of width 24 on 40 columns: up to three tiles on a pixel, liveness depends on all of them
    "order40": (40, 24, 24, 24, 16, 2, False),
    # the same columns under three tile rows (origins 0, 8, 16 on both axes): up to nine tiles on a pixel, so partial masks leave live, dead and
    # mixed quads next to each other
    "order40sq": (40, 40, 24, 24, 16, 2, False),
    # the vector path must be skipped: every batch tensor starts one element into its storage
    "aligned64_misaligned": (64, 24, 32, 32, 16, 3, True),
    # 2 x 3 tiles of 32 x 12 whose second tile column starts 1, 2, 3 px into the first quad (origins {0, 1}, {0, 2}, {0, 3}) and whose last quad
    # has 1, 2, 3 valid pixels: the second column's offset from quad 0 is negative, which the blend takes on the circle of W columns
    "shift1_33": (33, 20, 32, 12, 8, 4, False),
    "shift2_34": (34, 20, 32, 12, 8, 4, False),
    "shift3_35": (35, 20, 32, 12, 8, 4, False),
}
# the launcher's other forms.  It gives a thread 4 (2) planes while that leaves >= 131072 threads: H * ceil(W / 4) * 8 / 4 = 131072 at 1024 x 256,
# and 65536 (so 2 planes: 131072) at 512 x 256.  Upstream's default 96 / 48 grid, odd origins; 128 / 8, origins 0, 112, 224, ...
PLANES_CASES = {
    "planes2_512": (512, 256, 96, 96, 48, 8, False),
    "planes4_1024": (1024, 256, 128, 128, 8, 8, False),
}
MASKS = ["corner", "edges", "ell", "all", "specials"]      # and "zeros": every tile inactive, the subset is refused


def _geom(case):
    return CASES[case] if case in CASES else PLANES_CASES[case]


@functools.lru_cache(maxsize=None)
def _grid(case):
    return sr.grid(*_geom(case)[:6])


def _plan(E, case):
    plan = E.Plan(*_geom(case)[:6])
    g = _grid(case)
    assert plan.bboxes == list(g.boxes) and plan.tile_bs == g.tile_bs and plan.num_batches == len(g.batches)
    return plan


@functools.lru_cache(maxsize=None)
def _mask(case, kind):
    """[4, H, W] fp32, as the host's latent mask."""
    g = _grid(case)
    m = np.zeros((4, g.H, g.W), np.float32)
    if kind == "corner":
        m[2, g.H - 1, g.W - 1] = 1.0
    elif kind == "edges":                  # first column / row and last column / row of an interior tile (the middle tile column, middle row)
        x, y, tw, th = g.boxes[(g.rows // 2) * g.cols + g.cols // 2]
        m[0, y, x] = 1.0
        m[3, y + th - 1, x + tw - 1] = 1.0
    elif kind == "ell":                    # a stroke down the left edge and one along the bottom edge, half the canvas long
        m[:, :, 0] = 1.0
        m[:, g.H - 1, :g.W // 2] = 1.0
    elif kind == "all":
        m[:] = 1.0
    elif kind == "zeros":
        m[:] = 0.0
        m[:, ::2, 1::2] = -0.0
    elif kind == "specials":               # one pixel each, one per plane
        m[0, 0, g.W - 1] = NAN
        m[1, g.H - 1, 0] = np.float32(1.4e-45)
        m[2, g.H // 2, g.W // 2] = -3.0
        m[3, 1, 1] = 0.25
    else:
        raise KeyError(kind)
    return m


@functools.lru_cache(maxsize=None)
def _tiles(case, dt):
    """(canvas, the model output of EVERY tile [T * N, C, th, tw]) on the CPU, in the dtype -- computed once per (case, dtype)."""
    g, dtype = _grid(case), DT[dt]
    torch.manual_seed(len(case) + 11)
    x = torch.randn(N, C, g.H, g.W).to(dtype)
    outs = _tile_fn(torch.from_numpy(sr.gather(g, x.float().numpy(), range(len(g.boxes)))).to(dtype))
    return x, outs


@functools.lru_cache(maxsize=None)
def _fill(case, dt, special=False):
    g, dtype = _grid(case), DT[dt]
    torch.manual_seed(len(case) + 23)
    f = torch.randn(N, C, g.H, g.W).to(dtype)
    if special:
        flat = f.view(-1)
        vals = torch.tensor(SPECIALS).to(dtype)
        flat[:] = vals[(torch.arange(flat.numel()) * 5) % len(vals)]
        # NaNs with a payload, quiet and signalling, both signs: bit patterns a float conversion would not keep
        pats = {"f32": [0x7fc12345, -0x3fffff, 0x7f800001], "f16": [0x7e01, -0x1ff, 0x7c01], "bf16": [0x7fc1, -0x3f, 0x7f81]}[dt]
        b = bits(f).view(-1)
        for i, pat in enumerate(pats):
            b[i::17] = pat
        assert torch.isnan(f.view(-1)[0::17]).all() and (f == 0).any() and torch.isinf(f).any()
    return f


def _compact(outs, sub_batches):
    """The model outputs of the compact batches: the rows of every active tile, in slot order."""
    return [torch.cat([outs[t * N:(t + 1) * N] for t in b], dim=0).contiguous() for b in sub_batches]


# ---- activity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["odd37", "aligned64", "order40"])
def test_tile_activity_is_the_slice_test(plugin, cuda, case):
    E, g = plugin.engine, _grid(case)
    plan = _plan(E, case)
    for kind in MASKS + ["zeros"]:
        m = _mask(case, kind)
        want = sr.activity(g, m)
        assert E.tile_activity(plan, torch.from_numpy(m).to(cuda)) == want, (case, kind)
        assert (sum(want) == 0) == (kind == "zeros") and (kind != "all" or sum(want) == len(want)), (kind, want)
    one = _mask(case, "corner")[2]          # [H, W] is accepted as one plane
    assert E.tile_activity(plan, torch.from_numpy(one).to(cuda)) == sr.activity(g, one[None])
    with pytest.raises(E.MdtileError, match="no active tile"):
        plan.subset(E.tile_activity(plan, torch.from_numpy(_mask(case, "zeros")).to(cuda)), CASES[case][5])


def test_the_ell_mask_leaves_a_ragged_last_batch():
    g = _grid("odd37")
    want = sr.subset(g, sr.activity(g, _mask("odd37", "ell")), 4)
    assert want.active_ids == (0, 4, 8, 9, 10) and [len(b) for b in want.batches] == [3, 2]


# ---- gather ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dt", list(DT))
def test_sparse_gather_in_slot_order(plugin, cuda, case, dt):
    """Every mask that leaves a tile active: mdtile_gather per compact batch and mdtile_gather_all give the active tiles' values in slot order;
    on the misaligned variant mdtile_gather_all writes into batch tensors that start one element into their storage."""
    E, g = plugin.engine, _grid(case)
    plan = _plan(E, case)
    x, _ = _tiles(case, dt)
    xd = x.to(cuda)
    for kind in MASKS:
        want = sr.subset(g, sr.activity(g, _mask(case, kind)), CASES[case][5])
        sub = plan.subset(sr.activity(g, _mask(case, kind)), CASES[case][5])
        assert sub.active_ids == want.active_ids and sub.tile_bs == want.tile_bs
        refs = [torch.from_numpy(sr.gather(g, x.float().numpy(), ids)).to(x.dtype) for ids in want.batches]
        into = [_on_device(torch.full_like(r, NAN), cuda, True) for r in refs] if CASES[case][6] else None
        got_all = E.gather_all(sub, xd, out=into)
        assert len(got_all) == len(want.batches)
        for b, ref in enumerate(refs):
            _assert_bitwise(E.gather(sub, xd, b), ref, f"{case} {kind} gather batch {b}")
            _assert_bitwise(got_all[b], ref, f"{case} {kind} gather_all batch {b}")


# ---- blend -----------------------------------------------------------------------------------------------------------------------
def _map_args(m, method):
    if method == "md":
        return (m.weights.cpu().numpy(),), dict(weights=m.weights)
    return (None, m.tile_w.cpu().numpy(), m.rescale.cpu().numpy()), dict(tile_w=m.tile_w, rescale=m.rescale)


def _sparse_blend(E, cuda, case, method, sub, m, outs, fill, dtype):
    slots = [sub.active_ids[i * sub.tile_bs:(i + 1) * sub.tile_bs] for i in range(sub.num_batches)]
    batch = [_on_device(t, cuda, _geom(case)[6]) for t in _compact(outs, slots)]
    out = torch.full(fill.shape, NAN, dtype=dtype, device=cuda)
    got = E.blend_sparse(sub, E.METHOD_MD if method == "md" else E.METHOD_MOD, batch, N, C, fill=fill.to(cuda), out=out, **_map_args(m, method)[1])
    assert got.dtype == dtype
    return got


def _check_blend(plugin, cuda, case, method, dt, kinds):
    E, g, dtype = plugin.engine, _grid(case), DT[dt]
    plan = _plan(E, case)
    m = _maps(E, plan, cuda)
    x, outs = _tiles(case, dt)
    fill = _fill(case, dt)
    ref_args, kw = _map_args(m, method)
    full_ref = torch.from_numpy(sr.full_blend(g, method, outs.float().numpy(), N, *ref_args)).to(dtype)
    full_batches = [_on_device(outs[b[0] * N:(b[-1] + 1) * N].contiguous(), cuda, _geom(case)[6]) for b in g.batches]
    full_gpu = E.blend(plan, E.METHOD_MD if method == "md" else E.METHOD_MOD, full_batches, N, C, **kw).cpu()
    _assert_bitwise(full_gpu, full_ref, f"{case} {method} {dt} parent blend")
    for kind in kinds:
        active = sr.activity(g, _mask(case, kind))
        live = sr.live_map(g, active)
        sub = plan.subset(active, _geom(case)[5])
        want = sr.select(live, full_ref, fill)
        got = _sparse_blend(E, cuda, case, method, sub, m, outs, fill, dtype)
        _assert_bitwise(got, want, f"{case} {kind} {method} {dt} vs the restatement")
        _assert_bitwise(got, sr.select(live, full_gpu, fill), f"{case} {kind} {method} {dt} vs where(live, blend(parent), fill)")
        # poison: NaN in the active tiles' outputs at every element that lies on a pixel that is not live
        poisoned = outs.clone()
        for t, (bx, by, tw, th) in enumerate(g.boxes):
            poisoned[t * N:(t + 1) * N][:, :, torch.from_numpy(~live[by:by + th, bx:bx + tw])] = NAN
        assert live.all() or torch.isnan(poisoned).any()
        _assert_bitwise(_sparse_blend(E, cuda, case, method, sub, m, poisoned, fill, dtype), want, f"{case} {kind} {method} {dt} poisoned outputs")


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_blend_sparse_bitwise(plugin, cuda, case, method, dt):
    """mdtile_blend_sparse == where(live, full blend, fill), with the full blend both the sequential loop of the restatement and mdtile_blend on
    the parent plan; the tile outputs carry NaN wherever they lie on a pixel that is not live (no such element may be read)."""
    _check_blend(plugin, cuda, case, method, dt, MASKS)


@pytest.mark.parametrize("case", list(PLANES_CASES))
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_blend_sparse_two_and_four_planes_per_thread(plugin, cuda, case, method, dt):
    """The same on the two canvases at which the launcher gives a thread two and four planes."""
    _check_blend(plugin, cuda, case, method, dt, ["edges", "ell"])


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_all_active_reads_no_fill(plugin, cuda, case, method, dt):
    """Ta == T: every pixel is live, the result is the parent's blend and a NaN-filled `fill` leaves no NaN."""
    E, g, dtype = plugin.engine, _grid(case), DT[dt]
    plan = _plan(E, case)
    m = _maps(E, plan, cuda)
    _, outs = _tiles(case, dt)
    sub = plan.subset([1] * len(g.boxes), CASES[case][5])
    assert sub.active_ids == tuple(range(len(g.boxes)))
    fill = torch.full((N, C, g.H, g.W), NAN, dtype=dtype)
    got = _sparse_blend(E, cuda, case, method, sub, m, outs, fill, dtype)
    assert not torch.isnan(got).any()
    full_ref = torch.from_numpy(sr.full_blend(g, method, outs.float().numpy(), N, *_map_args(m, method)[0])).to(dtype)
    _assert_bitwise(got, full_ref, f"{case} all active {method} {dt}")


@pytest.mark.parametrize("case", ["odd37", "aligned64", "shift1_33", "shift2_34", "shift3_35"])
@pytest.mark.parametrize("dt", list(DT))
def test_fill_passes_through_bit_for_bit(plugin, cuda, case, dt):
    """+-0, +-inf, denormals and NaNs with payloads in `fill` come back with every bit at the pixels that are not live (integer comparison:
    the NaN patterns too), in every dtype."""
    E, g, dtype = plugin.engine, _grid(case), DT[dt]
    plan = _plan(E, case)
    m = _maps(E, plan, cuda)
    _, outs = _tiles(case, dt)
    fill = _fill(case, dt, special=True)
    for kind in ("corner", "ell"):
        active = sr.activity(g, _mask(case, kind))
        live = torch.from_numpy(sr.live_map(g, active))
        assert (~live).any() and live.any()
        sub = plan.subset(active, CASES[case][5])
        for method in ("md", "mod"):
            got = _sparse_blend(E, cuda, case, method, sub, m, outs, fill, dtype).cpu()
            assert torch.equal(bits(got)[:, :, ~live], bits(fill)[:, :, ~live]), f"{case} {kind} {method} {dt}: fill bits changed"
            assert not torch.isnan(got[:, :, live]).any()


# ---- the plugin with the option set --------------------------------------------------------------------------------------------
@pytest.fixture
def skip_option():
    _, shared = sh.host()
    shared.cmd_opts.mdtile_inpaint_skip = True
    try:
        yield shared
    finally:
        if hasattr(shared.cmd_opts, "mdtile_inpaint_skip"):
            del shared.cmd_opts.mdtile_inpaint_skip
        set_options(shared, False, False)


E2E = (37, 20, 16, 12, 6, 4)


def _evaluate(d, method, x, shared, cuda, monkeypatch, calls, noise_inversion=False):
    """One model evaluation of tile_fn through the delegate; `calls` collects (rows, the ControlNet hint at the call) per model call."""
    def model(xt):
        hint = d.control_params[0].hint_cond if d.control_params else None
        calls.append((xt.shape[0], None if hint is None else hint.detach().cpu().clone()))
        return _tile_fn(xt)
    cond = {"c_crossattn": [torch.zeros(N, 77, 768, device=cuda)], "c_concat": [torch.zeros(N, 5, 1, 1, device=cuda)]}
    monkeypatch.setattr(shared.sd_model, "apply_model_original_md", lambda x_, t_, c_: model(x_), raising=False)
    monkeypatch.setattr(shared.sd_model, "apply_model", lambda x_, t_, cond=None: model(x_), raising=False)
    xd = x.to(cuda)
    if noise_inversion:
        return d.get_noise(xd, torch.zeros(N, device=cuda), cond, 3)
    if method == "md":
        return d.sample_one_step(xd, None, lambda xt, b: model(xt), None)
    return d.apply_model_hijack(xd, torch.zeros(N, device=cuda), cond)


def _delegate(plugin, method, nmask, cuda, geom=E2E):
    d, p = make_delegate(plugin, method, *geom)
    if nmask is not None:
        p.nmask = torch.from_numpy(nmask).to(cuda)
    return d, p


@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_runs_only_the_touched_tiles(plugin, cuda, skip_option, monkeypatch, capsys, method):
    """Option off against option on, both through the host's `init * (1 - nmask) + nmask * out`: bitwise equal, with Ta * N model-call rows
    instead of T * N; a ControlNet stand-in receives the hints of the ACTIVE batch's boxes."""
    g = sr.grid(*E2E)
    nmask = _mask("odd37", "ell")
    active = sr.activity(g, nmask)
    want = sr.subset(g, active, 4)
    T, Ta = len(g.boxes), len(want.active_ids)
    assert 0 < Ta < T
    x, _ = _tiles("odd37", "f32")
    torch.manual_seed(3)
    init = torch.randn(N, C, g.H, g.W)
    nm = torch.from_numpy(nmask)[None]
    hint = torch.randn(1, 3, g.H * 8, g.W * 8, device=cuda)

    def host_mix(out):
        return init * (1 - nm) + nm * out.cpu()

    def arm(d):
        d.enable_controlnet, d.control_params, d.org_control_tensor_batch = True, [SimpleNamespace(hint_cond=hint)], [hint]

    del skip_option.cmd_opts.mdtile_inpaint_skip
    d, _ = _delegate(plugin, method, nmask, cuda)
    arm(d)
    calls_off = []
    out_off = _evaluate(d, method, x, skip_option, cuda, monkeypatch, calls_off)
    assert sum(r for r, _ in calls_off) == T * N and d.skip_mode is None and d.sparse_plan is None
    assert "inpaint" not in capsys.readouterr().out

    skip_option.cmd_opts.mdtile_inpaint_skip = True
    d, _ = _delegate(plugin, method, nmask, cuda)
    arm(d)
    calls_on = []
    out_on = _evaluate(d, method, x, skip_option, cuda, monkeypatch, calls_on)
    assert sum(r for r, _ in calls_on) == Ta * N, "the option did not reduce the model calls to the touched tiles"
    assert [r for r, _ in calls_on] == [len(b) * N for b in want.batches]
    assert d.skip_mode == "sparse" and d.sparse_plan.active_ids == want.active_ids and d.total_bboxes == len(want.batches)
    assert f"inpaint mask touches {Ta} of {T} tiles" in capsys.readouterr().out
    _assert_bitwise(host_mix(out_on), host_mix(out_off), f"{method}: the host's composite with and without the option")
    live = torch.from_numpy(sr.live_map(g, active))
    assert torch.equal(bits(out_on.cpu())[:, :, ~live], bits(x)[:, :, ~live]), "x_in where no active tile decides"
    for (_, got), ids in zip(calls_on, want.batches):
        tiles = np.concatenate([_take(hint.cpu(), g.boxes[t], 8) for t in ids], axis=0)
        assert np.array_equal(got.numpy(), np.repeat(tiles, N, axis=0)), ids
    # a second evaluation decides nothing again
    _evaluate(d, method, x, skip_option, cuda, monkeypatch, [])
    assert "inpaint mask" not in capsys.readouterr().out


@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_keeps_the_full_plan_and_says_why(plugin, cuda, skip_option, monkeypatch, capsys, method):
    g = sr.grid(*E2E)
    nmask = _mask("odd37", "ell")
    x, _ = _tiles("odd37", "f32")
    T = len(g.boxes)

    def rows_and_lines(d, **kw):
        capsys.readouterr()
        calls = []
        for _ in range(2):
            _evaluate(d, method, x, skip_option, cuda, monkeypatch, calls, **kw)
        lines = [l for l in capsys.readouterr().out.splitlines() if "--mdtile-inpaint-skip not applied" in l]
        return [sum(r for r, _ in calls) // 2, lines]

    d, _ = _delegate(plugin, method, nmask, cuda)           # custom regions
    d.enable_custom_bbox = True
    rows, lines = rows_and_lines(d)
    assert rows == T * N and len(lines) == 1 and "custom regions" in lines[0]
    d, _ = _delegate(plugin, method, nmask, cuda)           # Noise Inversion's own evaluations; the sampler's then skip
    rows, lines = rows_and_lines(d, noise_inversion=True)
    assert rows == T * N and len(lines) == 1 and "Noise Inversion" in lines[0] and d.skip_mode is None
    rows, lines = rows_and_lines(d)
    assert rows == 5 * N and not lines and d.skip_mode == "sparse"
    d, _ = _delegate(plugin, method, None, cuda)            # no mask
    rows, lines = rows_and_lines(d)
    assert rows == T * N and len(lines) == 1 and "no inpaint mask" in lines[0]
    d, _ = _delegate(plugin, method, nmask[:, :10], cuda)   # a mask of another size
    rows, lines = rows_and_lines(d)
    assert rows == T * N and len(lines) == 1 and "size" in lines[0]
    d, _ = _delegate(plugin, method, _mask("odd37", "all"), cuda)      # Ta == T: the full path, nothing to explain
    rows, lines = rows_and_lines(d)
    assert rows == T * N and not lines and d.skip_mode == "full" and d.sparse_plan is None
    for shape in ((g.H, g.W), (1, 4, g.H, g.W)):            # [H, W] and [1, P, H, W] are accepted
        d, p = _delegate(plugin, method, None, cuda)
        p.nmask = torch.from_numpy(nmask if len(shape) == 4 else nmask[0]).to(cuda).reshape(shape)
        rows, lines = rows_and_lines(d)
        assert rows == 5 * N and not lines, shape
    set_options(skip_option, True, False)                   # wrap-around
    d, _ = _delegate(plugin, method, nmask, cuda)
    assert d.plan.wrap_x
    rows, lines = rows_and_lines(d)
    assert rows == d.plan.num_tiles * N and len(lines) == 1 and "wrap" in lines[0]


@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_with_an_untouched_canvas_calls_no_model(plugin, cuda, skip_option, monkeypatch, capsys, method):
    x, _ = _tiles("odd37", "f32")
    d, _ = _delegate(plugin, method, _mask("odd37", "zeros"), cuda)
    calls = []
    out = _evaluate(d, method, x, skip_option, cuda, monkeypatch, calls)
    assert not calls and d.skip_mode == "empty"
    assert torch.equal(bits(out.cpu()), bits(x))
    again = _evaluate(d, method, x, skip_option, cuda, monkeypatch, calls)
    assert not calls and again.data_ptr() != out.data_ptr(), "every evaluation hands back a tensor of its own"
    assert "inpaint mask touches 0 of 12 tiles" in capsys.readouterr().out


@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_keeps_the_full_plan_beyond_the_batch_limit(plugin, cuda, skip_option, monkeypatch, capsys, method):
    """More active batches than a sparse plan carries (MAX_BATCHES pointers in the kernel arguments; the full path packs its batches into one
    buffer): the job runs on the full plan and says why once.  20 x 20 tiles of 16 at stride 8; the mask leaves out the four tiles of the
    top-left corner, so 396 tiles are touched: 396 batches at tile batch size 1, 198 at 2."""
    E = plugin.engine
    geom = (168, 168, 16, 16, 8)
    g = sr.grid(*geom, 1)
    nmask = np.ones((4, g.H, g.W), np.float32)
    nmask[:, :24, :24] = 0.0
    T, Ta = len(g.boxes), sum(sr.activity(g, nmask))
    assert (T, Ta) == (400, 396) and Ta > E.MAX_BATCHES >= Ta // 2
    torch.manual_seed(5)
    x = torch.randn(N, C, g.H, g.W)
    d, _ = _delegate(plugin, method, nmask, cuda, geom + (1,))
    capsys.readouterr()
    calls = []
    for _ in range(2):
        _evaluate(d, method, x, skip_option, cuda, monkeypatch, calls)
    lines = [l for l in capsys.readouterr().out.splitlines() if "--mdtile-inpaint-skip not applied" in l]
    assert sum(r for r, _ in calls) == 2 * T * N and d.skip_mode == "full" and d.sparse_plan is None
    assert len(lines) == 1 and "396 batches" in lines[0] and str(E.MAX_BATCHES) in lines[0]
    d, _ = _delegate(plugin, method, nmask, cuda, geom + (2,))
    calls = []
    _evaluate(d, method, x, skip_option, cuda, monkeypatch, calls)
    assert sum(r for r, _ in calls) == Ta * N and d.skip_mode == "sparse" and d.sparse_plan.num_batches == Ta // 2
