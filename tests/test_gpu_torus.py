"""Vertical wrap-around and the torus on the GPU (the per-axis kernels of csrc/wrap.hip), BITWISE against the numpy restatement
tests/wrap_ref.py: plan, weight maps, gather, the MultiDiffusion / Mixture-of-Diffusers blend in fp32, fp16 and bf16, the summation order at a
seam, special values, the refused calls, the delegates and the Tiled VAE hook with the options set.  No tolerance appears in this file; half
types follow tests/test_gpu_blend_matrix.py (inputs and tile outputs rounded to the dtype, the fp32 restatement evaluated on those values,
rounded once).

Every case runs N = 2, C = 4.  The small canvases take the launcher's one-plane-per-thread form, the two larger ones its 2- and 4-plane forms."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from hostsim import stub_host as sh

import wrap_ref as tr
from wrap_common import (DT, NAN, N, C, SPECIALS, assert_bitwise as _assert_bitwise, tile_fn as _tile_fn, identity as _identity,
                         on_device as _on_device, maps as _maps, make_delegate, evaluate_delegate, gpu_vae_hook, set_options as _set_options)

pytestmark = pytest.mark.gpu

CASES = tr.CASES
# the blend also runs aligned64 with every batch tensor one element into its storage: the vector path must be skipped
BLEND_CASES = list(CASES) + ["aligned64_misaligned"]


def _base(case):
    return case[:-len("_misaligned")] if case.endswith("_misaligned") else case


@functools.lru_cache(maxsize=None)
def _grid(case):
    return tr.case_grid(_base(case))


def _plan(E, case):
    W, H, tw, th, ov, wx, wy, bs = CASES[_base(case)]
    plan = E.Plan(W, H, tw, th, ov, bs, wrap_x=bool(wx), wrap_y=bool(wy))
    g = _grid(case)
    assert plan.bboxes == list(g.boxes) and plan.tile_bs == g.tile_bs and plan.num_batches == len(g.batches), (plan.bboxes, g.boxes)
    assert plan.num_batches <= E.MAX_BATCHES
    return plan


def _edges(origins, tile, extent):
    """Coordinates on every tile edge (just outside, on it, the quad around it) and on both sides of the seam."""
    return sorted({v % extent for o in origins for v in (o - 1, o, o + 1, o + 3, o + 4, o + tile - 1, o + tile)} | {0, 1, extent - 1, extent - 2})


def _canvas(case, dtype, special=False):
    g = _grid(case)
    torch.manual_seed(len(_base(case)) + 11)
    x = torch.randn(N, C, g.H, g.W)
    if special:
        vals = torch.tensor(SPECIALS)
        for i, c in enumerate(_edges(g.xs, g.tw, g.W)):        # columns of specials, one value per row ...
            x[:, :, :, c] = vals[(torch.arange(g.H) + i) % len(vals)][None, None, :]
        for i, r in enumerate(_edges(g.ys, g.th, g.H)):        # ... and rows of them, one value per column, shifted from row to row
            x[:, :, r, :] = vals[(torch.arange(g.W) * 3 + i) % len(vals)][None, None, :]
    return x.to(dtype)


@functools.lru_cache(maxsize=None)
def _tiles(case, dt, special=False):
    """(canvas, the model outputs of every batch) on the CPU, in the dtype -- computed once per (case, dtype)."""
    g, dtype = _grid(case), DT[dt]
    x = _canvas(case, dtype, special)
    fn = _identity if special else _tile_fn
    outs = [fn(torch.from_numpy(tr.gather(g, x.float().numpy(), b)).to(dtype)) for b in range(len(g.batches))]
    return x, outs


# ---- gather and weight maps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dt", list(DT))
def test_gather_and_gather_all_bitwise(plugin, cuda, case, dt):
    """x_tile[i N + n, c, ty, tx] = x_in[n, c, (y_i + ty) mod H, (x_i + tx) mod W]: mdtile_gather per batch and mdtile_gather_all."""
    E, g = plugin.engine, _grid(case)
    plan = _plan(E, case)
    x, _ = _tiles(case, dt)
    want = [torch.from_numpy(tr.gather(g, x.float().numpy(), b)).to(x.dtype) for b in range(len(g.batches))]
    xd = x.to(cuda)
    got_all = E.gather_all(plan, xd)
    assert len(got_all) == len(want)
    for b, w in enumerate(want):
        if b in (0, len(want) // 2, len(want) - 1):        # the per-batch call: first, middle and last batch (dense50 has 43)
            _assert_bitwise(E.gather(plan, xd, b), w, f"{case} gather batch {b}")
        _assert_bitwise(got_all[b], w, f"{case} gather_all batch {b}")


@pytest.mark.parametrize("case", list(CASES))
def test_weight_maps_bitwise(plugin, cuda, case):
    """The `+=` loop over the tile list with both indices mod the canvas: uniform (MultiDiffusion) and Gaussian (Mixture of Diffusers) tile
    weights, and the in-place form (the map is ADDED to what the buffer holds)."""
    E, g = plugin.engine, _grid(case)
    plan = _plan(E, case)
    m = _maps(E, plan, cuda)
    uni = tr.weight_map(g)
    assert uni.min() >= 1, "every pixel is covered"
    _assert_bitwise(m.weights, torch.from_numpy(uni), f"{case} uniform weight map")
    tile_w = m.tile_w.cpu().numpy()
    _assert_bitwise(m.gsum, torch.from_numpy(tr.weight_map(g, tile_w)), f"{case} Gaussian weight map")
    again = m.weights.clone()
    E.weight_map_add_grid(plan, None, again)
    _assert_bitwise(again, torch.from_numpy(uni + uni), f"{case} weight map added in place")


# ---- blend ---------------------------------------------------------------------------------------------------------------------
def _blend_case(plugin, cuda, case, method, dt, special=False):
    E, g, dtype = plugin.engine, _grid(case), DT[dt]
    plan = _plan(E, case)
    m = _maps(E, plan, cuda)
    x, outs = _tiles(_base(case), dt, special)
    tiles = torch.cat(outs, dim=0).float().numpy()
    if method == "md":
        ref = tr.blend(g, "md", tiles, N, m.weights.cpu().numpy())
        kw = dict(weights=m.weights)
    else:
        ref = tr.blend(g, "mod", tiles, N, None, m.tile_w.cpu().numpy(), m.rescale.cpu().numpy())
        kw = dict(tile_w=m.tile_w, rescale=m.rescale)
    batch = [_on_device(t, cuda, case.endswith("_misaligned")) for t in outs]
    out = torch.full((N, C, g.H, g.W), NAN, dtype=dtype, device=cuda)
    got = E.blend(plan, E.METHOD_MD if method == "md" else E.METHOD_MOD, batch, N, C, out=out, **kw)
    assert got.dtype == dtype
    _assert_bitwise(got, torch.from_numpy(ref).to(dtype), f"{case} {method} {dt}")


@pytest.mark.parametrize("case", BLEND_CASES)
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_blend_bitwise(plugin, cuda, case, method, dt):
    """mdtile_blend on a wrap-y / torus plan == the sequential fp32 `+=` loop in tile order with both indices mod the canvas, then the
    method's epilogue."""
    _blend_case(plugin, cuda, case, method, dt)


@pytest.mark.parametrize("method", ["md", "mod"])
def test_list_order_wins_at_the_seam(plugin, cuda, method):
    """order40 puts three tile rows on every canvas row; on rows 0 - 15 their ascending-index order ((0, 3, 4), (0, 1, 4)) is not the order in
    which they lie on the circle ((3, 4, 0), (4, 0, 1)).  The engine must give the list order.  The restatement is ALSO evaluated with the
    rows walked in circle order and must differ bitwise from the list order on this very input -- otherwise a match would say nothing about
    order."""
    E, g = plugin.engine, _grid("order40")
    plan = _plan(E, "order40")
    m = _maps(E, plan, cuda)
    torch.manual_seed(40)
    tiles = torch.randn(len(g.boxes) * N, C, g.th, g.tw)          # standard-normal tile outputs
    if method == "md":
        args, kw = (m.weights.cpu().numpy(),), dict(weights=m.weights)
    else:
        args, kw = (None, m.tile_w.cpu().numpy(), m.rescale.cpu().numpy()), dict(tile_w=m.tile_w, rescale=m.rescale)
    ref = tr.blend(g, method, tiles.numpy(), N, *args)
    circle = tr.blend_rows_in_circle_order(g, method, tiles.numpy(), N, *args)
    differ = (ref.view(np.int32) != circle.view(np.int32)).any(axis=(0, 1))          # [H, W]: a pixel differs in some plane
    print(f"order40 {method}: {int(differ.sum())} of {differ.size} pixels differ between list and circle order, rows {sorted(set(np.nonzero(differ)[0].tolist()))}")
    assert differ.any(), "circle order equals list order on this input: the case does not test the order"
    assert not differ[16:].any(), "rows 16 - 39 are covered by tile rows whose list order IS their circle order"
    sizes = [len(b) * N for b in g.batches]
    out = torch.full((N, C, g.H, g.W), NAN, device=cuda)
    got = E.blend(plan, E.METHOD_MD if method == "md" else E.METHOD_MOD, [t.to(cuda) for t in tiles.split(sizes, dim=0)], N, C, out=out, **kw)
    _assert_bitwise(got, torch.from_numpy(ref), f"order40 {method} list order")


@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("case", ["order40", "torus_odd", "ring_y"])
def test_special_values_bitwise(plugin, cuda, case, method):
    """+-0, +-inf, NaN, denormals and fp16 max on every tile edge and on both sides of both seams, through an identity model, fp32: the sign
    of zero and every denormal as the sequential loop has them (a sum that starts at +0.0 turns a lone -0.0 into +0.0)."""
    x, _ = _tiles(case, "f32", True)
    assert (x == 0).any() and torch.isinf(x).any() and torch.isnan(x).any() and ((x != 0) & (x.abs() < 1e-38)).any() and (x == 65504.0).any()
    g = _grid(case)
    for r in (0, g.H - 1):
        assert not torch.isfinite(x[0, 0, r]).all() and (x[0, 0, r] == 0).any(), "specials on both sides of the y seam"
    _blend_case(plugin, cuda, case, method, "f32", special=True)


# ---- refused calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["torus_odd", "ring_y"])
def test_refused_calls_write_nothing(plugin, cuda, case):
    """Regions, every MDTILE_BLEND_* flag, a row band, mdtile_gather_range, the packed destination, mdtile_blend_finalize and the dispatch
    query on a wrap-y / torus plan: an error whose text names the reason, and not one byte written."""
    E = plugin.engine
    plan = _plan(E, case)
    g = _grid(case)
    m = _maps(E, plan, cuda)
    _, outs = _tiles(case, "f32")
    batch = [t.to(cuda) for t in outs]
    out = torch.full((N, C, g.H, g.W), NAN, device=cuda)
    region = E.RegionSpec(0, 0, 8, 8, E.REGION_BG, torch.zeros(N, C, 8, 8, device=cuda))
    packed = [torch.cat(batch, dim=0)]
    for what, kw, b in (("regions", dict(regions=[region]), batch), ("flags", dict(partial=True), batch), ("flags", dict(tile_range=(0, 4)), batch),
                        ("flags", dict(packed=True), packed), ("row band", dict(row_range=(0, 8)), batch)):
        with pytest.raises(E.MdtileError, match=what):
            E.blend(plan, E.METHOD_MD, b, N, C, weights=m.weights, out=out, **kw)
    with pytest.raises(E.MdtileError, match="wrap-y.*partial path"):
        E.blend_finalize(plan, E.METHOD_MD, torch.zeros(N, C, g.H, g.W, device=cuda), weights=m.weights, out=out)
    assert torch.isnan(out).all(), "a refused blend wrote to its output"
    buf = torch.full((plan.num_tiles * N, C, g.th, g.tw), NAN, device=cuda)
    x = torch.zeros(N, C, g.H, g.W, device=cuda)
    with pytest.raises(E.MdtileError, match="wrap-y.*tile ranges"):
        E.gather_range(plan, x, buf, 0, plan.num_tiles)
    L = E.lib()
    ptrs = (ctypes.c_void_p * 1)(buf.data_ptr())
    rc = L.mdtile_gather_all(plan.handle, E.dtype_code(torch.float32), N, C, x.data_ptr(), ptrs, 1, None)       # ONE packed destination
    assert rc != 0 and b"no packed form" in L.mdtile_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(buf).all(), "a refused gather wrote to its output"
    with pytest.raises(E.MdtileError, match="wrap-y.*kernel of its own"):
        E.blend_dispatch(plan, torch.float32, N, C)


# ---- the plugin with the options set -------------------------------------------------------------------------------------------
@pytest.fixture
def options():
    """set(wrap_x, wrap_y) on the stub host's command line; both options are gone again afterwards."""
    _, shared = sh.host()
    _set_options(shared, False, False)
    try:
        yield lambda wrap_x, wrap_y: _set_options(shared, wrap_x, wrap_y) or shared
    finally:
        _set_options(shared, False, False)


@pytest.mark.parametrize("case", ["torus_odd", "ring_y"])
@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_with_the_options_bitwise(plugin, cuda, options, method, case):
    """One model evaluation through MultiDiffusion / MixtureOfDiffusers with --mdtile-wrap-y (and --mdtile-wrap-x): the delegate builds the
    plan of the options and its result is the restatement's."""
    g = _grid(case)
    W, H, tw, th, ov, wx, wy, bs = CASES[case]
    shared = options(bool(wx), bool(wy))
    d, p = make_delegate(plugin, method, W, H, tw, th, ov, bs)
    assert d.plan.wrap_y and d.plan.wrap_x == bool(wx) and d.plan.bboxes == list(g.boxes)
    assert p.extra_generation_params["Tiled Diffusion wrap y"] is True and ("Tiled Diffusion wrap x" in p.extra_generation_params) == bool(wx)
    x, outs = _tiles(case, "f32")
    out, map_args = evaluate_delegate(d, method, x, shared, cuda)
    ref = tr.blend(g, method, torch.cat(outs, dim=0).numpy(), N, *map_args)
    _assert_bitwise(out, torch.from_numpy(ref), f"delegate {method} {case}")


@pytest.mark.parametrize("both", [False, True], ids=["wrap_y", "torus"])
@pytest.mark.parametrize("is_decoder", [True, False], ids=["decoder", "encoder"])
def test_vae_hook_wraps_rows_by_its_tile_pad(plugin, cuda, options, is_decoder, both):
    """Tiled VAE with the option(s): the result is the plain hook's on the input padded by hand with the rows of the other edge (11 latent px
    for the decoder, 32 image px for the encoder) -- columns first, then rows, on the torus -- cropped by 8 P / P / 8 per side: torch.equal."""
    hook, P = gpu_vae_hook(plugin, cuda, is_decoder)
    torch.manual_seed(5)
    z = torch.randn(1, 4, 40, 24, device=cuda) if is_decoder else torch.randn(1, 3, 320, 192, device=cuda)
    hand = torch.cat([z[..., -P:], z, z[..., :P]], dim=-1) if both else z
    hand = torch.cat([hand[..., -P:, :], hand, hand[..., :P, :]], dim=-2)
    with torch.no_grad():
        padded = hook(hand)
        plain = hook(z)
        options(both, True)
        got = hook(z)
    cut = 8 * P if is_decoder else P // 8
    want = padded[..., cut:padded.shape[-2] - cut, :]
    if both:
        want = want[..., cut:want.shape[-1] - cut]
    assert got.shape == plain.shape == want.shape
    assert torch.equal(got, want), "hook with the option(s) vs the hand-padded input"
    assert not torch.equal(got, plain), "the option changed nothing"
