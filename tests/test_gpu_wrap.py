"""Horizontal wrap-around on the GPU (the per-axis kernels of csrc/wrap.hip on plain rows), BITWISE against the numpy
restatement tests/wrap_ref.py: plan, weight maps, gather, the MultiDiffusion / Mixture-of-Diffusers blend in fp32, fp16 and bf16, special
values, the refused calls, and the Tiled VAE hook with the option set.  No tolerance appears in this file; half types follow
tests/test_gpu_blend_matrix.py (inputs and tile outputs rounded to the dtype, the fp32 restatement evaluated on those values, rounded once).

Every case runs N = 2, C = 4.  The small canvases take the launcher's one-plane-per-thread form, the two larger ones its 2- and 4-plane forms."""
import functools

import numpy as np
import pytest
import torch

from hostsim import stub_host as sh

import wrap_ref as wr
from wrap_common import (DT, NAN, N, C, SPECIALS, assert_bitwise as _assert_bitwise, tile_fn as _tile_fn, identity as _identity,
                         on_device as _on_device, maps as _maps, make_delegate, evaluate_delegate, gpu_vae_hook, set_options)

pytestmark = pytest.mark.gpu

# id -> (W, H, requested tile_w, tile_h, overlap, tile_bs, misaligned batches).  The overlap is clamped to min(requested tile sizes) - 4, so the
# 48 x 12 tiles at overlap 44 are requested as 48 x 48 on a canvas 12 rows high.
CASES = {
    # W not a multiple of 4, odd origins (0, 9, 18, 27), ragged last quad, three tile rows
    "odd37": (37, 20, 16, 12, 6, 4, False),
    # the seam and tile column 0 16-byte aligned (origins 0, 21, 42 by the grid formula: column 0 takes the vector path, the others the elements)
    "seam64": (64, 16, 32, 32, 8, 2, False),
    # 13 tile columns (stride 50 / 13), 12 or all 13 covering one pixel, twelve tiles wrapping, by 1 px up to tw - 4 = 44 px
    "dense50": (50, 12, 48, 48, 44, 4, False),
    # stride 8, tile 24: three tile columns cover EVERY pixel; at the seam their list order (0, 1, 4 / 0, 3, 4) is not their order on the circle
    "order40": (40, 24, 24, 24, 16, 2, False),
    # the vector path must be skipped: every batch tensor starts one element into its storage
    "seam64_misaligned": (64, 16, 32, 32, 8, 2, True),
    # added: EVERY origin a multiple of 4 (0, 16, 32, 48), the last tile wraps by 16: all quads on the vector path
    "aligned64": (64, 24, 32, 32, 16, 3, False),
    # added: the launcher's other forms.  It gives a thread 4 (2) planes while that leaves >= 131072 threads: H * ceil(W / 4) * 8 / 4 = 131072 at
    # 1024 x 256, and 65536 (so 2 planes: 131072) at 512 x 256.  Upstream's default 96 / 48 grid, odd origins; 128 / 8, origins 0, 113, 227, ...
    "planes2_512": (512, 256, 96, 96, 48, 8, False),
    "planes4_1024": (1024, 256, 128, 128, 8, 8, False),
}


@functools.lru_cache(maxsize=None)
def _grid(case):
    W, H, tw, th, ov, bs, _ = CASES[case]
    g = wr.grid(W, H, tw, th, ov, bs)
    assert g is not None
    return g


def _plan(E, case):
    W, H, tw, th, ov, bs, _ = CASES[case]
    plan = E.Plan(W, H, tw, th, ov, bs, wrap_x=True)
    g = _grid(case)
    assert plan.bboxes == list(g.boxes) and plan.tile_bs == g.tile_bs and plan.num_batches == len(g.batches), (plan.bboxes, g.boxes)
    return plan


def _canvas(case, dtype, special=False):
    g = _grid(case)
    torch.manual_seed(len(case) + 7)
    x = torch.randn(N, C, g.H, g.W)
    if special:
        vals = torch.tensor(SPECIALS)
        cols = sorted({c % g.W for x0 in g.xs for c in (x0 - 1, x0, x0 + 1, x0 + 3, x0 + 4, x0 + g.tw - 1, x0 + g.tw)} | {0, 1, g.W - 1, g.W - 2})
        for i, c in enumerate(cols):                    # columns of specials on every tile edge and on both sides of the seam, one value per row
            x[:, :, :, c] = vals[(torch.arange(g.H) + i) % len(vals)][None, None, :]
        x[:, :, g.H // 2, :] = vals[(torch.arange(g.W) * 3) % len(vals)][None, None, :]
    return x.to(dtype)


@functools.lru_cache(maxsize=None)
def _tiles(case, dt, special=False):
    """(canvas, the model outputs of every batch) on the CPU, in the dtype -- computed once per (case, dtype)."""
    g, dtype = _grid(case), DT[dt]
    x = _canvas(case, dtype, special)
    fn = _identity if special else _tile_fn
    outs = [fn(torch.from_numpy(wr.gather(g, x.float().numpy(), b)).to(dtype)) for b in range(len(g.batches))]
    return x, outs


# ---- gather and weight maps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dt", list(DT))
def test_gather_and_gather_all_bitwise(plugin, cuda, case, dt):
    """x_tile[i N + n, c, ty, tx] = x_in[n, c, y_i + ty, (x_i + tx) mod W]: mdtile_gather per batch and mdtile_gather_all against np.take(mode='wrap')."""
    E, g = plugin.engine, _grid(case)
    plan = _plan(E, case)
    x, _ = _tiles(case, dt)
    want = [torch.from_numpy(wr.gather(g, x.float().numpy(), b)).to(x.dtype) for b in range(len(g.batches))]
    xd = x.to(cuda)
    got_all = E.gather_all(plan, xd)
    assert len(got_all) == len(want)
    for b, w in enumerate(want):
        _assert_bitwise(E.gather(plan, xd, b), w, f"{case} gather batch {b}")
        _assert_bitwise(got_all[b], w, f"{case} gather_all batch {b}")


@pytest.mark.parametrize("case", list(CASES))
def test_weight_maps_bitwise(plugin, cuda, case):
    """The `+=` loop over the tile list with columns mod W: uniform (MultiDiffusion) and Gaussian (Mixture of Diffusers) tile weights, and the
    in-place form (the map is ADDED to what the buffer holds)."""
    E, g = plugin.engine, _grid(case)
    plan = _plan(E, case)
    m = _maps(E, plan, cuda)
    uni = wr.weight_map(g)
    assert uni.min() >= 1, "every column is covered"
    _assert_bitwise(m.weights, torch.from_numpy(uni), f"{case} uniform weight map")
    tile_w = m.tile_w.cpu().numpy()
    _assert_bitwise(m.gsum, torch.from_numpy(wr.weight_map(g, tile_w)), f"{case} Gaussian weight map")
    again = m.weights.clone()
    E.weight_map_add_grid(plan, None, again)
    _assert_bitwise(again, torch.from_numpy(uni + uni), f"{case} weight map added in place")
    with np.errstate(all="ignore"):
        _assert_bitwise(m.rescale, torch.from_numpy((np.float32(1.0) / m.gsum.cpu().numpy()).astype(np.float32)), f"{case} rescale")


# ---- blend ---------------------------------------------------------------------------------------------------------------------
def _blend_case(plugin, cuda, case, method, dt, special=False):
    E, g, dtype = plugin.engine, _grid(case), DT[dt]
    plan = _plan(E, case)
    m = _maps(E, plan, cuda)
    x, outs = _tiles(case, dt, special)
    tiles = torch.cat(outs, dim=0).float().numpy()
    if method == "md":
        ref = wr.blend(g, "md", tiles, N, m.weights.cpu().numpy())
        kw = dict(weights=m.weights)
    else:
        ref = wr.blend(g, "mod", tiles, N, None, m.tile_w.cpu().numpy(), m.rescale.cpu().numpy())
        kw = dict(tile_w=m.tile_w, rescale=m.rescale)
    batch = [_on_device(t, cuda, CASES[case][6]) for t in outs]
    out = torch.full((N, C, g.H, g.W), NAN, dtype=dtype, device=cuda)
    got = E.blend(plan, E.METHOD_MD if method == "md" else E.METHOD_MOD, batch, N, C, out=out, **kw)
    assert got.dtype == dtype
    _assert_bitwise(got, torch.from_numpy(ref).to(dtype), f"{case} {method} {dt}")


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_blend_bitwise(plugin, cuda, case, method, dt):
    """mdtile_blend on a wrap-x plan == the sequential fp32 `+=` loop in tile order with columns mod W, then the method's epilogue."""
    _blend_case(plugin, cuda, case, method, dt)


def test_order_case_covers_every_pixel_three_times():
    """What makes `order40` bite: three tile columns on every pixel, and at the seam their ascending-index order differs from the order in
    which they lie on the circle -- a kernel that walked the cyclic run from its start would add (3, 4, 0) where the tile list adds (0, 3, 4)."""
    g = _grid("order40")
    assert (wr.weight_map(g) == 3).all() and g.cols == 5 and g.xs == (0, 8, 16, 24, 32)
    cover = [c for c in range(g.cols) if (0 - g.xs[c]) % g.W < g.tw]
    assert cover == [0, 3, 4]
    g = _grid("dense50")
    m = wr.weight_map(g)              # 12 of the 13 tile columns on most pixels, ALL of them on some: the cyclic run is then the whole list
    assert g.cols == 13 and m.min() == 12 and m.max() == 13
    wraps = sorted(x + g.tw - g.W for x in g.xs if x + g.tw > g.W)
    assert len(wraps) == 12 and wraps[0] == 1 and wraps[-1] == g.tw - 4, wraps


@pytest.mark.parametrize("method", ["md", "mod"])
def test_special_values_bitwise(plugin, cuda, method):
    """+-0, +-inf, NaN and denormals on every tile edge and on both sides of the seam, through an identity model, fp32: the sign of zero and
    every denormal as the sequential loop has them (a sum that starts at +0.0 turns a lone -0.0 into +0.0)."""
    x, _ = _tiles("order40", "f32", True)
    assert (x == 0).any() and torch.isinf(x).any() and torch.isnan(x).any() and ((x != 0) & (x.abs() < 1e-38)).any()
    _blend_case(plugin, cuda, "order40", method, "f32", special=True)
    _blend_case(plugin, cuda, "odd37", method, "f32", special=True)


# ---- refused calls -------------------------------------------------------------------------------------------------------------
def test_refused_calls_write_nothing(plugin, cuda):
    """Regions, every MDTILE_BLEND_* flag, a row band, mdtile_gather_range, mdtile_blend_finalize and the dispatch query on a wrap-x plan: an
    error whose text names the reason, and not one byte written."""
    E = plugin.engine
    plan = _plan(E, "odd37")
    g = _grid("odd37")
    m = _maps(E, plan, cuda)
    _, outs = _tiles("odd37", "f32")
    batch = [t.to(cuda) for t in outs]
    out = torch.full((N, C, g.H, g.W), NAN, device=cuda)
    region = E.RegionSpec(0, 0, 8, 8, E.REGION_BG, torch.zeros(N, C, 8, 8, device=cuda))
    packed = [torch.cat(batch, dim=0)]
    for what, kw, b in (("regions", dict(regions=[region]), batch), ("flags", dict(partial=True), batch), ("flags", dict(tile_range=(0, 4)), batch),
                        ("flags", dict(packed=True), packed), ("row band", dict(row_range=(0, 8)), batch)):
        with pytest.raises(E.MdtileError, match=what):
            E.blend(plan, E.METHOD_MD, b, N, C, weights=m.weights, out=out, **kw)
    with pytest.raises(E.MdtileError, match="wrap-x"):
        E.blend_finalize(plan, E.METHOD_MD, torch.zeros(N, C, g.H, g.W, device=cuda), weights=m.weights, out=out)
    assert torch.isnan(out).all(), "a refused blend wrote to its output"
    buf = torch.full((plan.num_tiles * N, C, g.th, g.tw), NAN, device=cuda)
    with pytest.raises(E.MdtileError, match="wrap-x"):
        E.gather_range(plan, torch.zeros(N, C, g.H, g.W, device=cuda), buf, 0, plan.num_tiles)
    assert torch.isnan(buf).all(), "a refused gather wrote to its output"
    with pytest.raises(E.MdtileError, match="wrap-x"):
        E.blend_dispatch(plan, torch.float32, N, C)
    # the plain plan of the same arguments is untouched by all this
    plain = E.Plan(37, 20, 16, 12, 6, 4)
    assert not plain.wrap_x and E.blend_dispatch(plain, torch.float32, N, C).kernel in (E.BLEND_KERNEL_PLAIN, E.BLEND_KERNEL_LDS)


# ---- the plugin with the option set --------------------------------------------------------------------------------------------
@pytest.fixture
def wrap_option():
    _, shared = sh.host()
    set_options(shared, True, False)
    try:
        yield shared
    finally:
        set_options(shared, False, False)


@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_with_the_option_bitwise(plugin, cuda, wrap_option, method):
    """One model evaluation through MultiDiffusion / MixtureOfDiffusers with --mdtile-wrap-x: the delegate builds the wrap-x plan and its
    result is the restatement's."""
    g = _grid("odd37")
    W, H, tw, th, ov, bs, _ = CASES["odd37"]
    d, p = make_delegate(plugin, method, W, H, tw, th, ov, bs)
    assert d.plan.wrap_x and p.extra_generation_params["Tiled Diffusion wrap x"] is True
    x, outs = _tiles("odd37", "f32")
    out, map_args = evaluate_delegate(d, method, x, wrap_option, cuda)
    ref = wr.blend(g, method, torch.cat(outs, dim=0).numpy(), N, *map_args)
    _assert_bitwise(out, torch.from_numpy(ref), f"delegate {method}")


@pytest.mark.parametrize("is_decoder", [True, False], ids=["decoder", "encoder"])
def test_vae_hook_wraps_by_its_tile_pad(plugin, cuda, wrap_option, is_decoder):
    """Tiled VAE with the option: the result is the plain hook's on the input padded by hand with the columns of the other edge (11 latent px
    for the decoder, 32 image px for the encoder), cropped by 8 P / P / 8 columns per side -- bit for bit."""
    hook, P = gpu_vae_hook(plugin, cuda, is_decoder)
    torch.manual_seed(5)
    z = torch.randn(1, 4, 24, 56, device=cuda) if is_decoder else torch.randn(1, 3, 192, 448, device=cuda)
    with torch.no_grad():
        got = hook(z)
        set_options(wrap_option, False, False)
        padded = hook(torch.cat([z[..., -P:], z, z[..., :P]], dim=-1))
        plain = hook(z)
    cut = 8 * P if is_decoder else P // 8
    want = padded[..., cut:padded.shape[-1] - cut]
    assert got.shape == plain.shape == want.shape
    _assert_bitwise(got, want.cpu().contiguous(), "hook with wrap-x vs the hand-padded input")
    assert not torch.equal(got, plain), "the option changed nothing"
