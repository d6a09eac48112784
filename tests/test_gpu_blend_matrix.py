"""The blend kernels over the case table of tests/blend_matrix_cases.py, BITWISE against oracle/blend_oracle.py: every dtype (fp32, fp16,
bf16), both methods, every planes-per-block form of k_blend_lds, packed and unpacked tile batches, the rank modes of the multi-GPU path
(row bands, partial sums of tile ranges, finalize), misaligned batch tensors (the k_blend fallback), special values, gather_range.

No tolerance appears in this file.  fp32: the order of operations is upstream's, so the bits are.  Half types: inputs and every tile /
region output are rounded to the dtype, the oracle is evaluated in fp32 on those values, and the result is rounded ONCE to the dtype with
round-to-nearest-even (`.to(dtype)` == __float2half_rn / __float2bfloat16) -- which is what a kernel that accumulates in fp32 and rounds at
its store computes.  Outputs are compared as bit patterns (int32 / int16 views: the sign of zero and denormals count); NaN positions are
compared separately and masked, a NaN's payload is not part of the contract.

Which kernel a case runs is asserted first, through the library's dispatch query, against the label in the case table: a case that drifts
off the path it was written for fails instead of silently testing another one."""
import pytest
import torch

from oracle import blend_oracle as bo
from hostsim import stub_host as sh

import blend_matrix_cases as bm
from test_gpu_blend import _delegate, _random_geometry

pytestmark = pytest.mark.gpu

DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
NAN = float("nan")


# ---- the stand-in model: fp32 arithmetic inside, rounded once to the I/O dtype -- the same bits on the CPU and on the GPU
def _tile_fn(t):
    return bo.synthetic_denoiser(t.float()).to(t.dtype)


def _region_fn(t, idx):
    return bo.synthetic_region_denoiser(t.float(), idx).to(t.dtype)


def _identity(t, *_):
    return t


def _reference(o, x, tile_fn=_tile_fn, region_fn=None):
    """The half reference of the module docstring (for fp32 every conversion below is the identity): x is already rounded to its dtype."""
    dtype = x.dtype
    rf = None if region_fn is None else (lambda t, i: region_fn(t.to(dtype), i).float())
    return o.evaluate(x.float(), lambda t: tile_fn(t.to(dtype)).float(), rf).to(dtype)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _assert_bitwise(got, ref, what):
    got = got.detach().cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {ref.dtype} {tuple(ref.shape)}"
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs ({int(torch.isnan(got).sum())} vs {int(nan.sum())} NaNs)"
    gb, rb = _bits(got), _bits(ref)
    z = torch.zeros((), dtype=gb.dtype)
    bad = torch.where(nan, z, gb) != torch.where(nan, z, rb)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ bitwise; first at {i}: got {got[i].item()!r} "
                             f"(0x{int(gb[i]) & 0xffffffff:x}), want {ref[i].item()!r} (0x{int(rb[i]) & 0xffffffff:x})")


def _assert_dispatch(d, case, what=""):
    """d: the library's answer for the launch at hand; case: the labelled row of the table."""
    if case.kernel == "lds":
        assert d.lds and d.planes == case.lpp, f"{case.id} {what}: labelled k_blend_lds with {case.lpp} planes per block, the launch gets {d}"
    else:
        assert not d.lds, f"{case.id} {what}: labelled k_blend, the launch gets {d}"
        assert (d.vec_quads > 0, d.elem_quads > 0) == ("vec" in case.paths, "elem" in case.paths), f"{case.id} {what}: {d}"


def _evaluate(plugin, d, method, x, tile_fn=_tile_fn, region_fn=_region_fn):
    dev, N = x.device, x.shape[0]
    if method == "md":
        return d.sample_one_step(x, None, lambda xt, b: tile_fn(xt), lambda xr, i, b: region_fn(xr, i))
    _, shared = sh.host()
    shared.sd_model.apply_model_original_md = lambda x_, t_, c_: tile_fn(x_)
    d.custom_apply_model = lambda x_in, t_in, c_in, bbox_id, bbox: region_fn(x_in, bbox_id)
    cond = {"c_crossattn": [torch.zeros(N, 77, 768, device=dev)], "c_concat": [torch.zeros(N, 5, 1, 1, device=dev)]}
    return d.apply_model_hijack(x, torch.zeros(N, device=dev), cond)


def _maps(o, method, cuda):
    if method == "md":
        return dict(weights=o.weights.to(cuda))
    return dict(tile_w=o.tile_weights.to(cuda), rescale=o.rescale.to(cuda))


# ---- delegate path ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bm.DELEGATE_CASES, ids=lambda c: c.id)
def test_delegate_matrix_bitwise(plugin, cuda, case):
    """One model evaluation through the plugin's MultiDiffusion / MixtureOfDiffusers on every geometry of the table, in every dtype."""
    E, dtype = plugin.engine, DT[case.dtype]
    W, H, tw, th, ov, bs = bm.GEOMETRIES[case.geom]
    d = _delegate(plugin, case.method, W, H, tw, th, ov, bs)
    _assert_dispatch(E.blend_dispatch(d.blend_plan(), dtype, case.N, case.C), case)
    o = bo.BlendOracle(case.method, W, H, tw, th, ov, bs)
    torch.manual_seed(len(case.id))
    x = torch.randn(case.N, case.C, H, W).to(dtype)
    out = _evaluate(plugin, d, case.method, x.to(cuda))
    assert out.dtype == dtype
    assert torch.equal(d.weights.cpu(), o.weights)
    _assert_bitwise(out, _reference(o, x), case.id)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("seed", range(32))
def test_random_geometries_half_bitwise(plugin, cuda, seed, dt):
    """The 32 seeded random geometries of test_gpu_blend.py in the half types (which kernel runs follows from the geometry; the bits do not)."""
    dtype = DT[dt]
    method, W, H, tw, th, ov, bs, N = _random_geometry(seed)
    d = _delegate(plugin, method, W, H, tw, th, ov, bs)
    o = bo.BlendOracle(method, W, H, tw, th, ov, bs)
    torch.manual_seed(seed)
    x = torch.randn(N, 4, H, W).to(dtype)
    out = _evaluate(plugin, d, method, x.to(cuda))
    assert torch.equal(d.weights.cpu(), o.weights), (method, W, H, tw, th, ov, bs, N)
    _assert_bitwise(out, _reference(o, x), f"{(method, W, H, tw, th, ov, bs, N)} {dt}")


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("method", bm.METHODS)
def test_regions_on_lds_grid_half_bitwise(plugin, cuda, method, dt):
    """Background and foreground regions over an LDS grid in the half types: the to_f32<T> region reads of the shared tail."""
    E, dtype = plugin.engine, DT[dt]
    regs = [(0.0, 0.0, 0.4, 1.0, "Background", 0.2), (0.3, 0.0, 0.4, 1.0, "Background", 0.2), (0.6, 0.1, 0.4, 0.8, "Foreground", 0.2),
            (0.55, 0.3, 0.3, 0.5, "Foreground", 0.3)]
    W, H, tw, th, ov, bs = 509, 131, 96, 96, 48, 4
    d = _delegate(plugin, method, W, H, tw, th, ov, bs, regs, True)
    assert E.blend_dispatch(d.blend_plan(), dtype, 2, 4).lds
    oregs = [bo.Region(*bo.region_rect(W, H, fx, fy, fw, fh), mode, fr) for (fx, fy, fw, fh, mode, fr) in regs]
    o = bo.BlendOracle(method, W, H, tw, th, ov, bs, oregs, True)
    torch.manual_seed(3)
    x = torch.randn(2, 4, H, W).to(dtype)
    out = _evaluate(plugin, d, method, x.to(cuda))
    assert torch.equal(d.weights.cpu(), o.weights)
    _assert_bitwise(out, _reference(o, x, _tile_fn, _region_fn), f"{method} {dt} regions")


# ---- engine path -----------------------------------------------------------------------------------------------------------
def _partial_restatement(o, tiles, N, lo, hi):
    """Raw fp32 partial sums of tiles [lo, hi): only those tiles, in list order, into a zero buffer; Mixture of Diffusers multiplies by the
    oracle's w, formed exactly as BlendOracle.evaluate forms it."""
    buf = torch.zeros((N, tiles.shape[1], o.H, o.W), dtype=torch.float32)
    for t in range(lo, hi):
        x, y, tw, th = o.boxes[t]
        v = tiles[t * N:(t + 1) * N].float()
        if o.method == "md":
            buf[:, :, y:y + th, x:x + tw] += v
        else:
            wgt = o.tile_weights * o.rescale[:, :, y:y + th, x:x + tw]
            buf[:, :, y:y + th, x:x + tw] += v * wgt
    return buf


def _epilogue_restatement(o, s):
    """BlendOracle.evaluate's last step on summed partials (no regions)."""
    return torch.where(o.weights > 1, s / o.weights, s) if o.method == "md" else s


def _poison_stage(E, plan, code, batch, N, C, packed, maps):
    """Leave NaN in the LDS of every CU: a full blend of all-NaN tiles with the layout of the launch that follows (same plan, dtype, planes
    per block) and one with the other element size (its rows land where the following launch has its zero pads).  A later read of LDS that
    launch did not write itself -- an unstaged row that `ok` fails to mask, a pad nobody zeroed, a row's last record the DMA left out --
    then shows in its result.  Values only; nothing here can fault."""
    dtype = batch[0].dtype
    for dt in (dtype, torch.float16 if dtype == torch.float32 else torch.float32):
        nan_batch = [torch.full(t.shape, NAN, dtype=dt, device=t.device) for t in batch]
        E.blend(plan, code, nan_batch, N, C, packed=packed, **maps)


@pytest.mark.parametrize("group", bm.ENGINE_GROUPS, ids=lambda g: "-".join(map(str, g)))
def test_engine_modes_bitwise(plugin, cuda, group):
    """E.blend on LDS grids at 4, 2 and 1 planes per block: packed == unpacked == oracle; a row band; partial sums of tile ranges split at a
    tile-row boundary and in the middle of a tile row, their finalize; the one-rank launch of the sharded path (range + partial + band)."""
    geom, dt, method, N, C = group
    E, dtype = plugin.engine, DT[dt]
    code = E.METHOD_MD if method == "md" else E.METHOD_MOD
    W, H, tw, th, ov, bs = bm.GEOMETRIES[geom]
    labels = {(c.packed, c.mode): c for c in bm.ENGINE_CASES if (c.geom, c.dtype, c.method, c.N, c.C) == group}
    plan, o = E.Plan(W, H, tw, th, ov, bs), bo.BlendOracle(method, W, H, tw, th, ov, bs)
    torch.manual_seed(len(geom) + N * C)
    x = torch.randn(N, C, H, W).to(dtype)
    outs_cpu = [_tile_fn(o.gather(x, b)) for b in o.batches]
    tiles = torch.cat(outs_cpu, dim=0)
    ref = _reference(o, x)
    outs = [t.to(cuda) for t in outs_cpu]
    maps = _maps(o, method, cuda)
    r_lo, r_hi = bm.row_band(plan)
    for packed in (False, True):
        batch = [tiles.to(cuda)] if packed else outs
        form = "packed" if packed else "unpacked"

        def run(mode, **kw):
            call = E.BlendCall(plan, code, batch, N, C, packed=packed, **maps, **kw)
            _assert_dispatch(call.dispatch(), labels[(packed, mode)], mode)
            _poison_stage(E, plan, code, batch, N, C, packed, maps)
            return call()

        _assert_bitwise(run("full"), ref, f"{form} full")
        # a row band into a NaN-prefilled canvas
        band = torch.full((N, C, H, W), NAN, dtype=dtype, device=cuda)
        run("rows", out=band, row_range=(r_lo, r_hi))
        _assert_bitwise(band[:, :, r_lo:r_hi], ref[:, :, r_lo:r_hi], f"{form} rows [{r_lo}, {r_hi})")
        assert torch.isnan(band[:, :, :r_lo]).all() and torch.isnan(band[:, :, r_hi:]).all(), f"{form}: rows outside [{r_lo}, {r_hi}) were written"
        # two "ranks": partial sums of two tile ranges, their sum, the epilogue
        for ranges in bm.tile_ranges(plan):
            parts = []
            for (lo, hi) in ranges:
                p = run("partial", partial=True, tile_range=(lo, hi))
                assert p.dtype == torch.float32
                _assert_bitwise(p, _partial_restatement(o, tiles, N, lo, hi), f"{form} partial sums of tiles [{lo}, {hi})")
                parts.append(p)
            s = (parts[0] + parts[1]).contiguous()
            fin = E.blend_finalize(plan, code, s, weights=maps.get("weights"), dtype=dtype)
            _assert_bitwise(fin, _epilogue_restatement(o, s.cpu()).to(dtype), f"{form} finalize of {ranges}")
        # one rank's launch of the sharded path: its tile range, partial sums, only the rows its tiles touch
        (lo, hi), _ = bm.tile_ranges(plan)[0]
        y_lo, y_hi = o.boxes[lo][1], o.boxes[hi - 1][1] + th
        p = torch.full((N, C, H, W), NAN, device=cuda)
        run("band", out=p, partial=True, tile_range=(lo, hi), row_range=(y_lo, y_hi))
        _assert_bitwise(p[:, :, y_lo:y_hi], _partial_restatement(o, tiles, N, lo, hi)[:, :, y_lo:y_hi], f"{form} band of tiles [{lo}, {hi})")
        assert torch.isnan(p[:, :, :y_lo]).all() and torch.isnan(p[:, :, y_hi:]).all(), f"{form}: rows outside [{y_lo}, {y_hi}) were written"


@pytest.mark.parametrize("case", bm.MISALIGNED_CASES, ids=lambda c: c.id)
def test_misaligned_batches_fall_back_bitwise(plugin, cuda, case):
    """Batch tensors that are views one element into their storage are not 16-byte aligned: the LDS-DMA cannot take them, the launch must
    fall back to k_blend -- with the same bits."""
    E, dtype = plugin.engine, DT[case.dtype]
    code = E.METHOD_MD if case.method == "md" else E.METHOD_MOD
    W, H, tw, th, ov, bs = bm.GEOMETRIES[case.geom]
    plan, o = E.Plan(W, H, tw, th, ov, bs), bo.BlendOracle(case.method, W, H, tw, th, ov, bs)
    torch.manual_seed(11)
    x = torch.randn(case.N, case.C, H, W).to(dtype)
    outs_cpu = [_tile_fn(o.gather(x, b)) for b in o.batches]
    ref = _reference(o, x)

    def shifted(t):
        store = torch.zeros(t.numel() + 16, dtype=dtype, device=cuda)
        v = store[1:1 + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == v.element_size() and v.is_contiguous()
        return v

    maps = _maps(o, case.method, cuda)
    aligned = E.BlendCall(plan, code, [t.to(cuda) for t in outs_cpu], case.N, case.C, **maps)
    assert aligned.dispatch().lds                                     # the same launch with aligned tensors is an LDS launch
    for packed, batch in ((False, [shifted(t) for t in outs_cpu]), (True, [shifted(torch.cat(outs_cpu, dim=0))])):
        call = E.BlendCall(plan, code, batch, case.N, case.C, packed=packed, **maps)
        _assert_dispatch(call.dispatch(), case, "packed" if packed else "unpacked")
        _assert_bitwise(call(), ref, f"{case.id} {'packed' if packed else 'unpacked'}")
    _assert_bitwise(aligned(), ref, f"{case.id} aligned")


# ---- special values --------------------------------------------------------------------------------------------------------
def _special_canvas(o, N, C, dtype, seed):
    """randn with +-0, +-inf, NaN, fp32 and fp16 denormals, fp16 max and values that round to denormals written on tile edges (first / last
    columns and rows of every tile, the pixels next to them) and in runs across the overlap bands."""
    torch.manual_seed(seed)
    x = torch.randn(N, C, o.H, o.W)
    vals = [0.0, -0.0, float("inf"), float("-inf"), NAN, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 2.0 ** -24, -2.0 ** -24, 3e-8, -3e-8, 6.1e-5, -6.0e-5,
            65504.0, -65504.0, 65520.0, 1.17549435e-38, -1e-10, 3.0e38, -3.0e38]
    xs, ys = sorted({b[0] for b in o.boxes}), sorted({b[1] for b in o.boxes})
    cols = sorted({c for x0 in xs for c in (x0 - 1, x0, x0 + 1, x0 + 2, x0 + 3, x0 + 4, x0 + o.tw - 2, x0 + o.tw - 1, x0 + o.tw) if 0 <= c < o.W})
    rows = sorted({r for y0 in ys for r in (y0 - 1, y0, y0 + 1, y0 + o.th - 1, y0 + o.th) if 0 <= r < o.H} | {o.H // 2, o.H // 2 + 1})
    k = 0
    for r in rows:
        for c in cols:
            for p in range(C):
                x[:, p, r, c] = vals[(k + 5 * p) % len(vals)]
            k += 1
    for i, c in enumerate(cols):                                       # columns of specials down the whole canvas, one value per row
        idx = (torch.arange(o.H) + i) % len(vals)
        x[:, :, :, c] = torch.tensor(vals)[idx][None, None, :]
    for i, r in enumerate(rows):                                       # and rows of them across every overlap band
        idx = (torch.arange(o.W) + 3 * i) % len(vals)
        x[:, :, r, :] = torch.tensor(vals)[idx][None, None, :]
    return x.to(dtype)


@pytest.mark.parametrize("case", bm.SPECIAL_CASES, ids=lambda c: c.id)
def test_special_values_bitwise(plugin, cuda, case):
    """An identity denoiser over inputs seeded with +-0.0, +-inf, NaN, denormals and the fp16 extremes, on an LDS grid and on k_blend grids:
    the sign of zero and every denormal must come out as the oracle has them (a sum that starts at +0.0 turns a lone -0.0 input into +0.0:
    a kernel that copied where upstream adds would show here).  MultiDiffusion weights of 2 and 4 take the
    exponent-arithmetic reciprocal of the tail, the 3-fold overlaps (weights 3 and 6) the true division."""
    E, dtype = plugin.engine, DT[case.dtype]
    W, H, tw, th, ov, bs = bm.GEOMETRIES[case.geom]
    d = _delegate(plugin, case.method, W, H, tw, th, ov, bs)
    _assert_dispatch(E.blend_dispatch(d.blend_plan(), dtype, case.N, case.C), case)
    o = bo.BlendOracle(case.method, W, H, tw, th, ov, bs)
    if case.method == "md" and case.geom == "odd200":
        assert {2.0, 3.0, 4.0, 6.0} <= set(o.weights.unique().tolist())
    x = _special_canvas(o, case.N, case.C, dtype, 17)
    assert (x == 0).any() and torch.isinf(x).any() and torch.isnan(x).any() and ((x != 0) & (x.float().abs() < 1e-38)).any() == (dtype == torch.float32)
    out = _evaluate(plugin, d, case.method, x.to(cuda), _identity, _identity)
    ref = _reference(o, x, _identity)
    _assert_bitwise(out, ref, case.id)


# ---- gather_range ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", bm.DTYPES)
def test_gather_range_fills_only_its_tiles(plugin, cuda, dt):
    """mdtile_gather_range on an odd-origin grid: tiles [lo, hi) of the packed buffer equal slicing, every other tile stays untouched."""
    E, dtype = plugin.engine, DT[dt]
    W, H, tw, th, ov, bs = bm.GEOMETRIES["odd203"]
    plan = E.Plan(W, H, tw, th, ov, bs)
    N, C, T = 2, 3, plan.num_tiles
    torch.manual_seed(4)
    x = torch.randn(N, C, H, W).to(dtype)
    want = torch.cat([x[:, :, by:by + bh, bx:bx + bw] for (bx, by, bw, bh) in plan.bboxes], dim=0)
    for lo, hi in ((0, T), (1, T - 2), (plan.cols - 1, plan.cols + 1), (3, 3)):
        packed = torch.full((T * N, C, th, tw), NAN, dtype=dtype, device=cuda)
        E.gather_range(plan, x.to(cuda), packed, lo, hi)
        got = packed.cpu()
        assert torch.equal(_bits(got[lo * N:hi * N]), _bits(want[lo * N:hi * N])), (lo, hi)
        assert torch.isnan(got[:lo * N]).all() and torch.isnan(got[hi * N:]).all(), f"tiles outside [{lo}, {hi}) were written"
