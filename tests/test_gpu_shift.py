"""The wrapped tile grid displaced cyclically (mdtile_gather_all_shift / mdtile_blend_shift, csrc/wrap.hip SHIFT kernels) on the
GPU, BITWISE: against the numpy restatement tests/shift_ref.py (np.roll around tests/wrap_ref.py) and, independent of it, against torch.roll around
the unshifted calls on the device.  Gather and blend of both methods in fp32, fp16 and bf16, special values, the refused calls, and the delegates
with --mdtile-grid-shift over three sampler steps.  No tolerance appears in this file; half types follow tests/test_gpu_blend_matrix.py (inputs and
tile outputs rounded to the dtype, the fp32 restatement evaluated on those values, rounded once).

Every case runs N = 2, C = 4; a test is one unshifted reference and one launch per shift of its case."""
import functools

import numpy as np
import pytest
import torch

from hostsim import stub_host as sh

import shift_ref as sr
import wrap_ref as tr
from wrap_common import (DT, NAN, N, C, SPECIALS, assert_bitwise as _assert_bitwise, tile_fn as _tile_fn, identity as _identity,
                         on_device as _on_device, maps as _maps, make_delegate, set_options as _set_options, take as _take)

pytestmark = pytest.mark.gpu

CASE_IDS = ["torus_odd", "ring_y", "order40", "aligned64", "rect44", "planes2_512", "planes4_1024"]
CASES = {k: tr.CASES[k] for k in CASE_IDS}
# aligned64 also runs with every batch tensor one element into its storage: no vector access of a batch is aligned
ALL_CASES = CASE_IDS + ["aligned64_misaligned"]


def _base(case):
    return case[:-len("_misaligned")] if case.endswith("_misaligned") else case


@functools.lru_cache(maxsize=None)
def _grid(case):
    return tr.case_grid(_base(case))


def _shifts(case):
    """(sx, sy) of a case: aligned, odd, next to each seam, the quad cut by the seam (W - 2), restricted to the axes that wrap."""
    W, H, _, _, _, wx, wy, _ = CASES[_base(case)]
    raw = [(0, 0), (1, 0), (4, 0), (0, 1), (3, H - 1), (W - 1, H - 1), (W - 2, 5), ((W // 2) & ~3, 2)]
    assert any(sx % 4 == 0 and sx > 4 for sx, _ in raw)
    out = []
    for sx, sy in raw:
        s = (sx if wx else 0, sy if wy else 0)
        if s not in out:
            out.append(s)
    return out


def _plan(E, case):
    W, H, tw, th, ov, wx, wy, bs = CASES[_base(case)]
    plan = E.Plan(W, H, tw, th, ov, bs, wrap_x=bool(wx), wrap_y=bool(wy))
    g = _grid(case)
    assert plan.bboxes == list(g.boxes) and plan.tile_bs == g.tile_bs and plan.num_batches == len(g.batches), (plan.bboxes, g.boxes)
    return plan


def _edges(origins, tile, extent):
    return sorted({v % extent for o in origins for v in (o - 1, o, o + 1, o + 3, o + 4, o + tile - 1, o + tile)} | {0, 1, extent - 1, extent - 2})


@functools.lru_cache(maxsize=None)
def _canvas(case, dt, special=False):
    g = _grid(case)
    torch.manual_seed(len(case) + 23)
    x = torch.randn(N, C, g.H, g.W)
    if special:
        vals = torch.tensor(SPECIALS)
        for i, c in enumerate(_edges(g.xs, g.tw, g.W)):
            x[:, :, :, c] = vals[(torch.arange(g.H) + i) % len(vals)][None, None, :]
        for i, r in enumerate(_edges(g.ys, g.th, g.H)):
            x[:, :, r, :] = vals[(torch.arange(g.W) * 3 + i) % len(vals)][None, None, :]
    return x.to(DT[dt])


@functools.lru_cache(maxsize=None)
def _tiles(case, dt, special=False):
    """The model outputs of every batch on the CPU, in the dtype: the shift does not change them (the blend takes any tile values)."""
    g = _grid(case)
    x = _canvas(case, dt, special)
    fn = _identity if special else _tile_fn
    return [fn(torch.from_numpy(tr.gather(g, x.float().numpy(), b)).to(DT[dt])) for b in range(len(g.batches))]


_REF = {}


def _unshifted_ref(case, method, dt, special, m):
    """The restatement's blend on the plan where it is (fp32, not yet rounded), once per (case, method, dtype)."""
    key = (case, method, dt, special)
    if key not in _REF:
        g = _grid(case)
        tiles = torch.cat(_tiles(case, dt, special), dim=0).float().numpy()
        if method == "md":
            _REF[key] = tr.blend(g, "md", tiles, N, m.weights.cpu().numpy())
        else:
            _REF[key] = tr.blend(g, "mod", tiles, N, None, m.tile_w.cpu().numpy(), m.rescale.cpu().numpy())
    return _REF[key]


def _map_kw(method, m):
    return dict(weights=m.weights) if method == "md" else dict(tile_w=m.tile_w, rescale=m.rescale)


def _method(E, method):
    return E.METHOD_MD if method == "md" else E.METHOD_MOD


# ---- gather ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES)
@pytest.mark.parametrize("dt", list(DT))
def test_gather_all_shift_bitwise(plugin, cuda, case, dt):
    """x_tile[i N + n, c, ty, tx] = x_in[n, c, (y_i + sy + ty) mod H, (x_i + sx + tx) mod W], against the restatement and against
    mdtile_gather_all of the rolled canvas on the device."""
    E, g = plugin.engine, _grid(case)
    plan = _plan(E, case)
    x = _canvas(_base(case), dt)
    xd = x.to(cuda)
    shape = lambda b: (len(g.batches[b]) * N, C, g.th, g.tw)
    for (sx, sy) in _shifts(case):
        out = [_on_device(torch.full(shape(b), NAN, dtype=x.dtype), cuda, case.endswith("_misaligned")) for b in range(len(g.batches))]
        got = E.gather_all_shift(plan, xd, sx, sy, out=out)
        rolled = E.gather_all(plan, torch.roll(xd, (-sy, -sx), (-2, -1)).contiguous())
        for b in range(len(g.batches)):
            want = torch.from_numpy(sr.gather(g, x.float().numpy(), b, sx, sy)).to(x.dtype)
            _assert_bitwise(got[b], want, f"{case} {dt} gather_all_shift ({sx}, {sy}) batch {b}")
            _assert_bitwise(got[b], rolled[b].cpu(), f"{case} {dt} gather_all_shift ({sx}, {sy}) batch {b} vs gather_all of the rolled canvas")


# ---- blend -----------------------------------------------------------------------------------------------------------------------
def _blend_case(plugin, cuda, case, method, dt, special=False):
    E, g, dtype = plugin.engine, _grid(case), DT[dt]
    plan = _plan(E, case)
    m = _maps(E, plan, cuda)
    ref = _unshifted_ref(_base(case), method, dt, special, m)
    batch = [_on_device(t, cuda, case.endswith("_misaligned")) for t in _tiles(_base(case), dt, special)]
    for (sx, sy) in _shifts(case):
        out = torch.full((N, C, g.H, g.W), NAN, dtype=dtype, device=cuda)
        got = E.blend_shift(plan, _method(E, method), batch, N, C, sx=sx, sy=sy, out=out, **_map_kw(method, m))
        assert got.dtype == dtype
        want = torch.from_numpy(np.roll(ref, (sy, sx), axis=(-2, -1))).to(dtype)
        _assert_bitwise(got, want, f"{case} {method} {dt} blend_shift ({sx}, {sy})")


@pytest.mark.parametrize("case", ALL_CASES)
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_blend_shift_bitwise(plugin, cuda, case, method, dt):
    """mdtile_blend_shift == roll(the sequential fp32 `+=` loop in tile order with the plan's own maps, then the epilogue), rounded once."""
    _blend_case(plugin, cuda, case, method, dt)


@pytest.mark.parametrize("case", ALL_CASES)
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_roll_identity_on_the_device(plugin, cuda, case, method, dt):
    """blend_shift(tiles, sx, sy) == torch.roll(blend(tiles), (sy, sx)) as bits, (0, 0) included: the identity itself, without the restatement."""
    E, g, dtype = plugin.engine, _grid(case), DT[dt]
    plan = _plan(E, case)
    m = _maps(E, plan, cuda)
    batch = [_on_device(t, cuda, case.endswith("_misaligned")) for t in _tiles(_base(case), dt)]
    plain = E.blend(plan, _method(E, method), batch, N, C, **_map_kw(method, m))
    for (sx, sy) in _shifts(case):
        out = torch.full((N, C, g.H, g.W), NAN, dtype=dtype, device=cuda)
        got = E.blend_shift(plan, _method(E, method), batch, N, C, sx=sx, sy=sy, out=out, **_map_kw(method, m))
        _assert_bitwise(got, torch.roll(plain, (sy, sx), (-2, -1)).cpu(), f"{case} {method} {dt} blend_shift ({sx}, {sy}) vs the rolled blend")


@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("case", ["order40", "torus_odd"])
def test_special_values_bitwise(plugin, cuda, case, method):
    """+-0, +-inf, NaN, denormals and fp16 max on every tile edge and on both sides of both seams, through an identity model, fp32."""
    x = _canvas(case, "f32", True)
    assert (x == 0).any() and torch.isinf(x).any() and torch.isnan(x).any() and ((x != 0) & (x.abs() < 1e-38)).any() and (x == 65504.0).any()
    _blend_case(plugin, cuda, case, method, "f32", special=True)


# ---- refused calls ---------------------------------------------------------------------------------------------------------------
def _refused(E, cuda, plan, sx, sy, match):
    """Both shifted calls on `plan` with (sx, sy): MDTILE_E_ARG with a text that matches, and NaN-painted outputs left as they are."""
    th, tw = plan.tile_h, plan.tile_w
    x = torch.zeros(N, C, plan.h, plan.w, device=cuda)
    tiles = [torch.full((len(b) * N, C, th, tw), NAN, device=cuda) for b in plan.batches]
    with pytest.raises(E.MdtileError, match=r"mdtile_gather_all_shift failed \(rc=-1\).*" + match):
        E.gather_all_shift(plan, x, sx, sy, out=tiles)
    out = torch.full((N, C, plan.h, plan.w), NAN, device=cuda)
    ones = [torch.ones_like(t) for t in tiles]
    weights = torch.ones(plan.h, plan.w, device=cuda)
    with pytest.raises(E.MdtileError, match=r"mdtile_blend_shift failed \(rc=-1\).*" + match):
        E.blend_shift(plan, E.METHOD_MD, ones, N, C, sx=sx, sy=sy, weights=weights, out=out)
    torch.cuda.synchronize()
    assert all(torch.isnan(t).all() for t in tiles), "a refused gather wrote to its output"
    assert torch.isnan(out).all(), "a refused blend wrote to its output"


def test_refused_calls_write_nothing(plugin, cuda):
    E = plugin.engine
    assert E.E_ARG == -1
    W, H, tw, th, ov, _, _, bs = CASES["torus_odd"]
    plain = E.Plan(W, H, tw, th, ov, bs)
    _refused(E, cuda, plain, 0, 0, "plain plan")
    _refused(E, cuda, plain, 1, 1, "plain plan")
    sparse = plain.subset([1] + [0] * (plain.num_tiles - 2) + [1], bs)
    _refused(E, cuda, sparse, 0, 0, "sparse plan")
    ring = _plan(E, "ring_y")
    _refused(E, cuda, ring, 1, 0, "x axis does not wrap")
    _refused(E, cuda, ring, 4, 3, "x axis does not wrap")
    torus = _plan(E, "torus_odd")
    _refused(E, cuda, torus, W, 0, "out of range")
    _refused(E, cuda, torus, 0, H, "out of range")
    _refused(E, cuda, torus, -1, 0, "out of range")
    _refused(E, cuda, torus, 0, -4, "out of range")
    # what the wrap-around blend refuses stays refused: a batch count that is not the plan's
    m = _maps(E, torus, cuda)
    out = torch.full((N, C, H, W), NAN, device=cuda)
    a_batch = torch.ones(len(torus.batches[0]) * N, C, th, tw, device=cuda)
    with pytest.raises(E.MdtileError, match="batches given"):
        E.blend_shift(torus, E.METHOD_MD, [a_batch], N, C, sx=1, sy=1, weights=m.weights, out=out)
    with pytest.raises(E.MdtileError, match="Mixture of Diffusers needs"):
        E.blend_shift(torus, E.METHOD_MOD, [torch.ones(len(b) * N, C, th, tw, device=cuda) for b in torus.batches], N, C, sx=1, sy=1, out=out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused blend wrote to its output"


# ---- the delegates with the option set -----------------------------------------------------------------------------------------------
@pytest.fixture
def options():
    """set(wrap_x, wrap_y, shift) on the stub host's command line; the options are gone and the step counter is back afterwards."""
    _, shared = sh.host()

    def set_(wrap_x, wrap_y, shift):
        _set_options(shared, wrap_x, wrap_y)
        if shift:
            shared.cmd_opts.mdtile_grid_shift = True
        elif hasattr(shared.cmd_opts, "mdtile_grid_shift"):
            delattr(shared.cmd_opts, "mdtile_grid_shift")
        return shared

    set_(False, False, False)
    step = shared.state.sampling_step
    try:
        yield set_
    finally:
        set_(False, False, False)
        shared.state.sampling_step = step


@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_moves_the_grid_every_step(plugin, cuda, options, method):
    """MultiDiffusion / MixtureOfDiffusers with --mdtile-wrap-x --mdtile-wrap-y --mdtile-grid-shift over three sampler steps: every step's
    result is the restatement's at that step's pinned shift, the shifts differ, and the image conditioning fed to the model with every batch
    is cut at the shifted tiles."""
    case, seed = "torus_odd", 1234567
    g = _grid(case)
    W, H, tw, th, ov, wx, wy, bs = CASES[case]
    shared = options(True, True, True)
    d, p = make_delegate(plugin, method, W, H, tw, th, ov, bs)
    p.all_seeds = [seed]
    assert d.grid_shift and d.plan.bboxes == list(g.boxes) and (d.wrap_ext, d.wrap_ext_y) == (g.tw, g.th)
    assert p.extra_generation_params["Tiled Diffusion grid shift"] is True
    x = _canvas(case, "f32")
    torch.manual_seed(3)
    icond = torch.randn(N, 5, H, W)
    cond = {"c_crossattn": [torch.zeros(N, 77, 768, device=cuda)], "c_concat": [icond.to(cuda)]}
    if method == "md":
        maps = (d.weights.cpu().numpy()[0, 0],)
    else:
        maps = (None, d.get_tile_weights().cpu().numpy(), d.rescale_factor.cpu().numpy()[0, 0])
    shifts = []
    for step in range(3):
        shared.state.sampling_step = step
        sx, sy = sr.PINNED[(seed, step, 0, W)], sr.PINNED[(seed, step, 1, H)]
        shifts.append((sx, sy))
        seen = []
        if method == "md":
            def repeat(xt, bboxes):
                seen.append(d.get_icond(d.repeat_cond_dict(cond, bboxes)))
                return _tile_fn(xt)
            out = d.sample_one_step(x.to(cuda), None, repeat, None)
        else:
            def model(x_, t_, c_):
                seen.append(d.get_icond(c_))
                return _tile_fn(x_)
            shared.sd_model.apply_model_original_md = model
            out = d.apply_model_hijack(x.to(cuda), torch.zeros(N, device=cuda), cond)
        tiles = [_tile_fn(torch.from_numpy(sr.gather(g, x.numpy(), b, sx, sy))) for b in range(len(g.batches))]
        ref = sr.blend(g, method, torch.cat(tiles, dim=0).numpy(), N, sx, sy, *maps)
        _assert_bitwise(out, torch.from_numpy(ref), f"delegate {method} step {step} shift ({sx}, {sy})")
        boxes = sr.boxes(g, sx, sy)
        assert len(seen) == len(g.batches)
        for b, batch in enumerate(g.batches):
            want = np.concatenate([_take(icond, boxes[t]) for t in batch], axis=0)
            _assert_bitwise(seen[b], torch.from_numpy(np.ascontiguousarray(want)), f"delegate {method} step {step} image conditioning of batch {b}")
    assert len(set(shifts)) == 3, shifts
