"""Inpaint tile skipping under the jittered grid (mdtile_lattice_activity / mdtile_lattice_subset_* / mdtile_gather_all_lattice_sparse /
mdtile_blend_lattice_sparse, csrc/lattice.hip) on the GPU, BITWISE (integer views, NaN payloads and zero signs included): against
the numpy restatement tests/lattice_sparse_ref.py, with all tiles active against mdtile_gather_all_lattice / mdtile_blend_lattice, at rest on an
exact-fit canvas against the fixed-grid skip (mdtile_tile_activity / Plan.subset / mdtile_blend_sparse), slot tables with entries out of range,
and the delegates with the three options over three sampler steps.  No tolerance appears in this file; half types follow
tests/test_gpu_blend_matrix.py (inputs and tile outputs rounded to the dtype, the fp32 restatement evaluated on those values, rounded once).

Every mask case has 0 < Ta < T by the restatement (asserted); the designated all / none / out-of-range cases are excepted."""
import functools

import numpy as np
import pytest
import torch

from hostsim import stub_host as sh

import grid_lattice_ref as lr
import lattice_sparse_ref as ls
from wrap_common import DT, NAN, bits, tile_fn as _tile_fn, make_delegate

pytestmark = pytest.mark.gpu

# id -> (W, H, tile, overlap, tile_bs, [(N, C)], shifts)
GEOMETRIES = {
    "40x24": (40, 24, 16, 4, 4, [(2, 4)], [(12, 12), (1, 1), (5, 3)]),      # the host tests' geometry: at rest, most tiles, odd
    "40x28": (40, 28, 16, 4, 4, [(2, 4)], [(12, 12), (7, 2)]),              # exact fit at rest
    "37x23": (37, 23, 16, 0, 3, [(1, 3)], [(16, 16), (5, 3), (1, 1)]),      # ragged last quad, odd planes (one plane per thread), zero overlap
    "40x16": (40, 16, 16, 4, 2, [(1, 4)], [(12, 1), (5, 1)]),               # the tile spans y: only x moves
    "512x512": (512, 512, 64, 8, 8, [(2, 4), (2, 3)], [(5, 3)]),            # planes_per_thread picks 4 planes (N C = 8) and 2 (N C = 6)
}
BIG_PATTERNS = ("block", "corner_br", "second")


@functools.lru_cache(maxsize=None)
def _lat(geom, sx, sy):
    Wc, Hc, tile, ov, bs = GEOMETRIES[geom][:5]
    g = lr.lattice(Wc, Hc, tile, tile, ov, bs, sx, sy)
    assert g is not None
    return g


def _lattice(E, geom, sx, sy):
    Wc, Hc, tile, ov, bs = GEOMETRIES[geom][:5]
    lat = E.Lattice(Wc, Hc, tile, tile, ov, bs, sx, sy)
    g = _lat(geom, sx, sy)
    assert lat.bboxes == list(g.boxes)
    return lat, g


def _points(g, pts, value=1.0, planes=2, base=0.0):
    m = np.full((planes, g.H, g.W), base, np.float32)
    for (y, x) in pts:
        m[planes - 1, y, x] = value
    return m


def _pushed_only_pixel(g):
    """(tile, y, x): a pixel inside the pushed-in box of an edge tile but outside its contributing box, or None (no tile is pushed in)."""
    ym = min(g.H - 1, max(g.vs[0], 0) + 1)
    if g.us[0] < 0 and g.us[0] + g.tw < g.tw:          # the first column is pushed in: it is evaluated over [0, tw) and writes [0, u_0 + tw)
        r = max(rr for rr in range(g.rows) if max(g.vs[rr], 0) <= ym)
        return r * g.cols, ym, g.us[0] + g.tw
    if g.us[-1] > g.W - g.tw:                          # the last column is pushed in: evaluated over [W - tw, W), writes [u_K, W)
        r = max(rr for rr in range(g.rows) if max(g.vs[rr], 0) <= ym)
        return r * g.cols + g.cols - 1, ym, g.us[-1] - 1
    return None


@functools.lru_cache(maxsize=None)
def _patterns(geom, sx, sy):
    """name -> ("mask", [P, H, W] fp32) | ("flags", the test's own flags, uploaded with their ranks)."""
    g = _lat(geom, sx, sy)
    W_, H_ = g.W, g.H
    ym = H_ // 2
    u = g.us[1]                                          # a lattice border column inside the canvas (every geometry has two columns)
    out = {
        "corner_tl": ("mask", _points(g, [(0, 0)])),
        "corner_tr": ("mask", _points(g, [(0, W_ - 1)])),
        "corner_bl": ("mask", _points(g, [(H_ - 1, 0)])),
        "corner_br": ("mask", _points(g, [(H_ - 1, W_ - 1)])),
        "border_u": ("mask", _points(g, [(ym, u)])),
        "border_u_minus_1": ("mask", _points(g, [(ym, u - 1)])),
        "nan": ("mask", _points(g, [(ym, u)], value=NAN, base=-0.0)),              # -0.0 everywhere else: it does not count
        "denormal": ("mask", _points(g, [(ym, u - 1)], value=1e-40, base=-0.0)),
        "negative_fraction": ("mask", _points(g, [(0, W_ - 1)], value=-0.25)),
        "second": ("flags", [1 if t % 2 == 0 else 0 for t in range(len(g.boxes))]),
    }
    v = g.vs[1] if g.rows > 1 else ym
    out["block"] = ("mask", _points(g, [(y, x) for y in range(max(v - 2, 0), min(v + 2, H_)) for x in range(max(u - 3, 0), min(u + 3, W_))]))
    po = _pushed_only_pixel(g)
    if po is not None:
        out["pushed_in_only"] = ("mask", _points(g, [po[1:]]))
    if geom == "512x512":
        out = {k: v_ for k, v_ in out.items() if k in BIG_PATTERNS}
    return out


def _active(geom, sx, sy, name):
    kind, val = _patterns(geom, sx, sy)[name]
    return list(val) if kind == "flags" else ls.activity(_lat(geom, sx, sy), val)


def _cases(geom):
    return [(s, name) for s in GEOMETRIES[geom][6] for name in _patterns(geom, *s)]


def _assert_bits(got, want, what):
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {want.dtype} {tuple(want.shape)}"
    bad = bits(got) != bits(want)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ bitwise; first at {i}: got {got[i].item()!r}, want {want[i].item()!r}")


@functools.lru_cache(maxsize=None)
def _canvas(geom, dt, n, c):
    Wc, Hc = GEOMETRIES[geom][:2]
    torch.manual_seed(len(geom) + 17 * n + c)
    return torch.randn(n, c, Hc, Wc).to(DT[dt])


@functools.lru_cache(maxsize=None)
def _fill(geom, dt, n, c):
    """Random values with NaN payloads, -0.0 and denormals written into the bits."""
    Wc, Hc = GEOMETRIES[geom][:2]
    torch.manual_seed(len(geom) + 5)
    f = torch.randn(n, c, Hc, Wc).to(DT[dt]).contiguous()
    iv = bits(f).view(-1)
    special = {"f32": [0x7FC12345, -0x80000000, 0x00000001, -0x003FFFFF], "f16": [0x7E01, -0x8000, 0x0001, -0x0201],
               "bf16": [0x7FC1, -0x8000, 0x0001, -0x0041]}[dt]
    for k, s in enumerate(special):
        iv[k::7][: max(1, iv.numel() // 28)] = s
    return f


@functools.lru_cache(maxsize=None)
def _tile_w(cuda_index, tw, th):
    import mdtile
    return mdtile.gaussian_weights(tw, th, torch.device("cuda", cuda_index))


def _outputs(g, x, active, n):
    """The model outputs of the active tiles [Ta * n, C, th, tw] in x's dtype, with NaN wherever a value can only feed a pixel that is not live:
    outside the tile's contributing box, and at its pixels that are not live."""
    act = ls.ids(active)
    out = _tile_fn(torch.from_numpy(ls.gather(g, x.float().numpy(), act)).to(x.dtype))
    live = ls.live_map(g, active)
    cb = ls.boxes(g)
    for s, t in enumerate(act):
        bx, by = g.boxes[t][:2]
        y0, y1, x0, x1 = cb[t]
        feeds = np.zeros((g.th, g.tw), bool)
        feeds[y0 - by:y1 - by, x0 - bx:x1 - bx] = live[y0:y1, x0:x1]
        out[s * n:(s + 1) * n][:, :, torch.from_numpy(~feeds)] = NAN
    return out


def _split(t, sizes):
    return [c.contiguous() for c in torch.split(t, sizes)]


def _subset(E, lat, g, geom, s, name, cuda):
    """(flags by the restatement, the binding's LatticeSubset) of one case: the mask through mdtile_lattice_activity, or the test's own upload."""
    kind, val = _patterns(geom, *s)[name]
    active = _active(geom, *s, name)
    if kind == "mask":
        flags, slot = E.lattice_activity(lat, torch.from_numpy(val).to(cuda))
        assert flags == active, f"{geom} {s} {name}: activity {flags} vs {active}"
        assert slot.cpu().tolist() == ls.slots(active), f"{geom} {s} {name}: slots"
    else:
        flags, slot = active, torch.tensor(ls.slots(active), dtype=torch.int32, device=cuda)
    sub = E.LatticeSubset(lat, flags, GEOMETRIES[geom][4], slot)
    assert sub.ids == ls.ids(active) and (sub.num_batches, sub.tile_bs) == ls.batching(sum(active), GEOMETRIES[geom][4])
    assert sub.bboxes == [g.boxes[t] for t in sub.ids]
    return active, sub


# ---- (a) against the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_the_cases_leave_tiles_to_skip(geom):
    """The condition on the inputs, by the restatement alone: 0 < Ta < T for every mask case; the pushed-in-only pixel lies in an inactive tile's
    pushed-in box and is live."""
    seen_pushed = False
    for s, name in _cases(geom):
        g, active = _lat(geom, *s), _active(geom, *s, name)
        assert 0 < sum(active) < len(active), (geom, s, name, active)
        if name == "pushed_in_only":
            t, y, x = _pushed_only_pixel(g)
            bx, by, tw, th = g.boxes[t]
            assert bx <= x < bx + tw and by <= y < by + th and not active[t] and ls.live_map(g, active)[y, x]
            seen_pushed = True
        if name in ("nan", "denormal"):
            assert sum(active) <= 4, "-0.0 counted"
    assert seen_pushed or geom == "40x16" or geom == "512x512"


@pytest.mark.parametrize("geom", list(GEOMETRIES))
def test_activity_and_slots_bitwise(plugin, cuda, geom):
    """Flags and ranks of every mask case, written into NaN-like garbage (no pre-clearing); planes 1 and 2."""
    E = plugin.engine
    for s, name in _cases(geom):
        kind, val = _patterns(geom, *s)[name]
        if kind != "mask":
            continue
        lat, g = _lattice(E, geom, *s)
        for mask in (val, val[1:]):
            flags, slot = E.lattice_activity(lat, torch.from_numpy(np.ascontiguousarray(mask)).to(cuda))
            want = ls.activity(g, mask)
            assert flags == want and slot.cpu().tolist() == ls.slots(want), (geom, s, name)
    # all and none
    lat, g = _lattice(E, geom, *GEOMETRIES[geom][6][-1])
    T = len(g.boxes)
    flags, slot = E.lattice_activity(lat, torch.full((1, g.H, g.W), 1e-45, device=cuda))
    assert flags == [1] * T and slot.cpu().tolist() == list(range(T))
    flags, slot = E.lattice_activity(lat, torch.full((3, g.H, g.W), -0.0, device=cuda))
    assert flags == [0] * T and slot.cpu().tolist() == [-1] * T


@pytest.mark.parametrize("geom", list(GEOMETRIES))
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", list(DT))
def test_gather_and_blend_bitwise(plugin, cuda, geom, method, dt):
    """(a) gather and blend of every case equal the restatement; (c) the pixels that are not live carry fill's bits -- NaN payloads, -0.0 and
    denormals -- and the NaN painted into the active tiles' outputs wherever they feed only such pixels reaches no output."""
    E, dtype = plugin.engine, DT[dt]
    bs = GEOMETRIES[geom][4]
    for (n, c) in GEOMETRIES[geom][5]:
        x, fill = _canvas(geom, dt, n, c), _fill(geom, dt, n, c)
        xd, filld = x.to(cuda), fill.to(cuda)
        for s, name in _cases(geom):
            what = f"{geom} {n}x{c} {method} {dt} {s} {name}"
            lat, g = _lattice(E, geom, *s)
            active, sub = _subset(E, lat, g, geom, s, name, cuda)
            Ta = sum(active)
            assert 0 < Ta < len(active), what
            sizes = [len(b) * n for b in sub.batches]
            got = E.gather_all_lattice_sparse(sub, xd, out=[torch.full((k, c, g.th, g.tw), NAN, dtype=dtype, device=cuda) for k in sizes])
            _assert_bits(torch.cat(got), torch.from_numpy(ls.gather(g, x.float().numpy(), sub.ids)).to(dtype), what + " gather")
            tile_w = _tile_w(cuda.index or 0, g.tw, g.th) if method == "mod" else None
            outs = _outputs(g, x, active, n)
            out = torch.full((n, c, g.H, g.W), NAN, dtype=dtype, device=cuda)
            res = E.blend_lattice_sparse(sub, E.METHOD_MD if method == "md" else E.METHOD_MOD, [t.to(cuda) for t in _split(outs, sizes)], n, c,
                                         fill=filld, tile_w=tile_w, out=out)
            want = ls.blend(g, method, outs.float().numpy(), n, active, fill, tile_w.cpu().numpy() if method == "mod" else None)
            _assert_bits(res, want, what + " blend")
            live = torch.from_numpy(ls.live_map(g, active))
            assert torch.equal(bits(res.cpu())[:, :, ~live], bits(fill)[:, :, ~live]), what + ": a pixel that is not live does not carry fill's bits"
            assert torch.isfinite(res.cpu().float()[:, :, live]).all(), what + ": a value that feeds no live pixel reached the output"


# ---- (b) all tiles active: the full lattice's calls ----------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", list(GEOMETRIES))
@pytest.mark.parametrize("dt", list(DT))
def test_all_active_equals_the_full_lattice_calls(plugin, cuda, geom, dt):
    E, dtype = plugin.engine, DT[dt]
    n, c = GEOMETRIES[geom][5][0]
    x = _canvas(geom, dt, n, c).to(cuda)
    for s in GEOMETRIES[geom][6]:
        lat, g = _lattice(E, geom, *s)
        flags, slot = E.lattice_activity(lat, torch.ones(1, g.H, g.W, device=cuda))
        sub = E.LatticeSubset(lat, flags, GEOMETRIES[geom][4], slot)
        assert sub.num_active == lat.num_tiles and sub.bboxes == lat.bboxes and (sub.num_batches, sub.tile_bs) == (lat.num_batches, lat.tile_bs)
        tiles = E.gather_all_lattice(lat, x)
        for b, t in enumerate(E.gather_all_lattice_sparse(sub, x)):
            _assert_bits(t, tiles[b].cpu(), f"{geom} {dt} {s} gather batch {b}")
        outs = [_tile_fn(t) for t in tiles]
        fill = torch.full((n, c, g.H, g.W), NAN, dtype=dtype, device=cuda)
        for method, tw_ in ((E.METHOD_MD, None), (E.METHOD_MOD, _tile_w(cuda.index or 0, g.tw, g.th))):
            want = E.blend_lattice(lat, method, outs, n, c, tile_w=tw_)
            got = E.blend_lattice_sparse(sub, method, outs, n, c, fill=fill, tile_w=tw_)
            _assert_bits(got, want.cpu(), f"{geom} {dt} {s} method {method} blend")


# ---- (d) at rest on the exact fit: the fixed-grid skip -------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DT))
def test_at_rest_equals_the_fixed_grid_skip(plugin, cuda, dt):
    E, dtype = plugin.engine, DT[dt]
    geom, s = "40x28", (12, 12)
    Wc, Hc, tile, ov, bs = GEOMETRIES[geom][:5]
    n, c = GEOMETRIES[geom][5][0]
    plan = E.Plan(Wc, Hc, tile, tile, ov, bs)
    lat, g = _lattice(E, geom, *s)
    assert lat.bboxes == plan.bboxes
    x, fill = _canvas(geom, dt, n, c).to(cuda), _fill(geom, dt, n, c).to(cuda)
    tile_w = E.gaussian_weights(plan.tile_w, plan.tile_h, cuda)
    for name, (kind, val) in _patterns(geom, *s).items():
        if kind != "mask":
            continue
        mask = torch.from_numpy(val).to(cuda)
        flags, slot = E.lattice_activity(lat, mask)
        assert flags == E.tile_activity(plan, mask), name
        sub, splan = E.LatticeSubset(lat, flags, bs, slot), plan.subset(flags, bs)
        assert sub.bboxes == splan.bboxes and sub.ids == splan.active_ids and (sub.num_batches, sub.tile_bs) == (splan.num_batches, splan.tile_bs)
        tiles = E.gather_all(splan, x)
        for b, t in enumerate(E.gather_all_lattice_sparse(sub, x)):
            _assert_bits(t, tiles[b].cpu(), f"{dt} {name} gather batch {b}")
        outs = [_tile_fn(t) for t in tiles]
        for method, tw_ in (("md", None), ("mod", tile_w)):
            wsum = torch.zeros(Hc, Wc, device=cuda)
            E.weight_map_add_grid(plan, tw_, wsum)
            kw = dict(weights=wsum) if method == "md" else dict(tile_w=tile_w, rescale=E.reciprocal(wsum))
            M = E.METHOD_MD if method == "md" else E.METHOD_MOD
            want = E.blend_sparse(splan, M, outs, n, c, fill=fill, **kw)
            got = E.blend_lattice_sparse(sub, M, outs, n, c, fill=fill, tile_w=tw_)
            _assert_bits(got, want.cpu(), f"{dt} {name} {method} blend")


# ---- (e) slot entries out of range ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["md", "mod"])
def test_slots_out_of_range_give_pixels_that_are_not_live(plugin, cuda, method):
    """A table that is not the flags' ranks: entries < 0 or >= num_active count as "not active" in the gather and in the blend; nothing is read
    or written outside a batch, no error is raised."""
    E = plugin.engine
    geom, s, (n, c) = "40x24", (5, 3), (2, 4)
    lat, g = _lattice(E, geom, *s)
    T = len(g.boxes)
    a, b = 5, 6
    flags = [1 if t in (a, b) else 0 for t in range(T)]
    M = E.METHOD_MD if method == "md" else E.METHOD_MOD
    tile_w = _tile_w(cuda.index or 0, g.tw, g.th) if method == "mod" else None
    x, fill = _canvas(geom, "f32", n, c), _fill(geom, "f32", n, c)
    for table, alive in (({a: 0, b: 2}, [a]), ({a: -7, b: 1}, [b]), ({a: 2 ** 31 - 1, b: -2 ** 31}, []), ({a: 2, b: 3}, [])):
        slot = [-1] * T
        for t, v in table.items():
            slot[t] = v
        sub = E.LatticeSubset(lat, flags, 4, torch.tensor(slot, dtype=torch.int32, device=cuda))
        assert sub.num_active == 2 and sub.num_batches == 1
        got = E.gather_all_lattice_sparse(sub, x.to(cuda), out=[torch.full((2 * n, c, g.th, g.tw), NAN, device=cuda)])[0].cpu()
        want = torch.full((2 * n, c, g.th, g.tw), NAN)
        for t in alive:
            want[table[t] * n:(table[t] + 1) * n] = torch.from_numpy(ls.gather(g, x.numpy(), [t]))
        _assert_bits(got, want, f"{method} {table} gather")
        outs = torch.full((2 * n, c, g.th, g.tw), NAN)
        effective = [1 if t in alive else 0 for t in range(T)]
        for t in alive:
            outs[table[t] * n:(table[t] + 1) * n] = _outputs(g, x, effective, n)
        res = E.blend_lattice_sparse(sub, M, [outs.to(cuda)], n, c, fill=fill.to(cuda), tile_w=tile_w)
        if alive:
            compact = outs[table[alive[0]] * n:(table[alive[0]] + 1) * n]
            want = ls.blend(g, method, compact.numpy(), n, effective, fill, tile_w.cpu().numpy() if method == "mod" else None)
        else:
            want = fill
        _assert_bits(res, want, f"{method} {table} blend")


# ---- (f) the delegates with the options set --------------------------------------------------------------------------------------------
@pytest.fixture
def options():
    _, shared = sh.host()
    step = shared.state.sampling_step
    names = ("mdtile_grid_jitter", "mdtile_inpaint_skip", "mdtile_jitter_inpaint_skip")
    for n in names:
        setattr(shared.cmd_opts, n, True)
    try:
        yield shared
    finally:
        for n in names:
            if hasattr(shared.cmd_opts, n):
                delattr(shared.cmd_opts, n)
        shared.state.sampling_step = step


@pytest.mark.parametrize("method", ["md", "mod"])
def test_delegate_skips_on_the_moving_grid(plugin, cuda, options, method):
    """MultiDiffusion / MixtureOfDiffusers with the three options over three sampler steps, two evaluations each: every result is the
    restatement's on that step's pinned lattice with that step's active tiles and fill = the input, the model sees the active tiles only, and
    the second evaluation of a step reuses the first one's lattice and subset."""
    shared, seed = options, 1234567
    Wc, Hc, tile, ov, bs = GEOMETRIES["40x24"][:5]
    n, c = 2, 4
    d, p = make_delegate(plugin, method, Wc, Hc, tile, tile, ov, bs)
    p.all_seeds = [seed]
    mask = _points(_lat("40x24", 12, 12), [(y, x_) for y in range(9, 13) for x_ in range(17, 22)], planes=1)
    p.nmask = torch.from_numpy(mask)
    assert d.grid_jitter
    x = _canvas("40x24", "f32", n, c)
    cond = {"c_crossattn": [torch.zeros(n, 77, 768, device=cuda)], "c_concat": [torch.zeros(n, 5, 1, 1, device=cuda)]}
    tile_w = d.get_tile_weights() if method == "mod" else None
    counts = []
    for step in range(3):
        shared.state.sampling_step = step
        g = lr.lattice(Wc, Hc, tile, tile, ov, bs, *lr.step_shift(Wc, Hc, tile, tile, ov, seed, step))
        active = ls.activity(g, mask)
        assert 0 < sum(active) < len(active)
        counts.append((sum(active), len(active)))
        grids = []
        for _ in range(2):
            seen = []
            if method == "md":
                out = d.sample_one_step(x.to(cuda), None, lambda xt, b: seen.append(xt.shape[0]) or _tile_fn(xt), None)
            else:
                shared.sd_model.apply_model_original_md = lambda x_, t_, c_: seen.append(x_.shape[0]) or _tile_fn(x_)
                out = d.apply_model_hijack(x.to(cuda), torch.zeros(n, device=cuda), cond)
            assert sum(seen) == sum(active) * n
            outs = _tile_fn(torch.from_numpy(ls.gather(g, x.numpy(), ls.ids(active))))
            want = ls.blend(g, method, outs.numpy(), n, active, x, tile_w.cpu().numpy() if method == "mod" else None)
            _assert_bits(out, want, f"delegate {method} step {step}")
            grids.append(d._subset_at[1])
        assert grids[0] is grids[1] and isinstance(grids[0], plugin.engine.LatticeSubset)
    assert len(set(counts)) > 1 or len(counts) == 3
    assert p.extra_generation_params["Tiled Diffusion jitter inpaint skip"] is True
