"""--mdtile-jitter-inpaint-skip without a GPU: the numpy restatement tests/lattice_sparse_ref.py against the restatements it
is built on (all tiles active: the lattice blend; at rest on an exact-fit canvas: the fixed-grid skip), the property that every pixel with a
non-zero mask is live, header = library = binding for the new struct and calls, every refusal by name (argument checks happen before any device
is touched), the option, and the delegates' wiring on the CPU stub host with engine doubles: one activity decision per sampler step, the model
called on the active tiles only, the empty step, the all-active step on the old calls, the old behaviour without the switch, the "ignored" line,
the progress bar, the infotext, no random generator touched.  The kernels themselves are tested in tests/test_gpu_lattice_sparse.py."""
import argparse
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import grid_lattice_ref as lr
import lattice_sparse_ref as ls
import sparse_ref as sr
from wrap_common import host, wired, delegate, load_preload      # noqa: F401  (host, wired: fixtures)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["mdtile_lattice_activity", "mdtile_lattice_subset_make", "mdtile_lattice_subset_bboxes", "mdtile_gather_all_lattice_sparse",
               "mdtile_blend_lattice_sparse"]
W, H, TILE, OV, BS = 40, 24, 16, 4, 4      # stride 12: 3 columns at rest, 4 at any other shift; 2 rows at shifts 4 .. 12, 3 below
SEED = 1234567
N, C = 2, 4


def _mask(points, planes=1, w=W, h=H):
    m = np.zeros((planes, h, w), np.float32)
    for (y, x) in points:
        m[-1, y, x] = 1.0
    return m


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("shift", [(12, 12), (1, 1), (5, 3)])
def test_all_active_is_the_lattice_blend(method, shift):
    g = lr.lattice(W, H, TILE, TILE, OV, BS, *shift)
    T = len(g.boxes)
    rng = np.random.default_rng(3)
    tiles = rng.standard_normal((T * N, C, g.th, g.tw)).astype(np.float32)
    tw = lr.gaussian(g.tw, g.th).astype(np.float32) if method == "mod" else None
    fill = torch.full((N, C, H, W), float("nan"))
    got = ls.blend(g, method, tiles, N, [1] * T, fill, tw)
    want = torch.from_numpy(lr.blend(g, method, tiles, N, tw))
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert ls.slots([1] * T) == list(range(T)) and ls.live_map(g, [1] * T).all()
    assert ls.activity(g, np.ones((1, H, W), np.float32)) == [1] * T


@pytest.mark.parametrize("method", ["md", "mod"])
def test_at_rest_on_an_exact_fit_it_is_the_fixed_grid_skip(method):
    """40 x 28 at tile 16 / 4: the lattice at rest is the plain grid, contributing box = pushed-in box = the tile."""
    Wc, Hc = 40, 28
    g = lr.lattice(Wc, Hc, TILE, TILE, OV, BS, 12, 12)
    pg = sr.grid(Wc, Hc, TILE, TILE, OV, BS)
    assert list(g.boxes) == list(pg.boxes)
    rng = np.random.default_rng(5)
    tw = lr.gaussian(g.tw, g.th).astype(np.float32) if method == "mod" else None
    for points in ([(0, 0)], [(13, 20)], [(27, 39), (3, 30)], [(14, 14), (20, 5)]):
        mask = _mask(points, 2, Wc, Hc)
        active = ls.activity(g, mask)
        assert active == sr.activity(pg, mask) and 0 < sum(active) < len(active)
        assert np.array_equal(ls.live_map(g, active), sr.live_map(pg, active))
        sub = sr.subset(pg, active, BS)
        assert sub.active_ids == ls.ids(active) and ls.batching(sum(active), BS) == (len(sub.batches), sub.tile_bs)
        x = rng.standard_normal((N, C, Hc, Wc)).astype(np.float32)
        assert np.array_equal(ls.gather(g, x, ls.ids(active)), sr.gather(pg, x, sub.active_ids))
        compact = rng.standard_normal((sum(active) * N, C, g.th, g.tw)).astype(np.float32)
        fill = torch.from_numpy(x)
        full = np.full((len(pg.boxes) * N, C, g.th, g.tw), np.nan, np.float32)
        for s, t in enumerate(sub.active_ids):
            full[t * N:(t + 1) * N] = compact[s * N:(s + 1) * N]
        wsum = lr.weight_map(g, tw)
        with np.errstate(all="ignore"):
            plain = sr.full_blend(pg, method, full, N, wsum, tw, (np.float32(1.0) / wsum).astype(np.float32))
        want = sr.select(sr.live_map(pg, active), torch.from_numpy(plain), fill)
        got = ls.blend(g, method, compact, N, active, fill, tw)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), points


def test_every_pixel_with_a_mask_is_live():
    """Brute force over all shifts of the small canvas and a pixel walk: a non-zero mask pixel activates every tile that covers it.  And the
    contributing box, not the pushed-in one, decides: some shift has an edge tile whose pushed-in box holds the pixel while the tile stays inactive."""
    pushed_in_only = 0
    for sx in range(1, 13):
        for sy in range(1, 13):
            g = lr.lattice(W, H, TILE, TILE, OV, BS, sx, sy)
            for (y, x) in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (sy - 1, sx - 1), (sy, sx), (11, 19), (H - 1, 17), (7, W - 1)]:
                if y < 0 or x < 0:
                    continue
                active = ls.activity(g, _mask([(y, x)]))
                live = ls.live_map(g, active)
                assert live[y, x] and sum(active) >= 1, (sx, sy, y, x)
                for t, (bx, by, tw, th) in enumerate(g.boxes):
                    if bx <= x < bx + tw and by <= y < by + th and not active[t]:
                        pushed_in_only += 1
    assert pushed_in_only > 0
    assert ls.slots([0, 1, 1, 0, 1]) == [-1, 0, 1, -1, 2] and ls.batching(9, 4) == (3, 3) and ls.batching(5, 4) == (2, 3)


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
    fields = re.search(r"typedef struct mdtile_lattice_subset \{(.*?)\} mdtile_lattice_subset;", src, flags=re.S).group(1)
    names = [n.strip().lstrip("*") for decl in re.findall(r"(?:mdtile_lattice|const int\*|int) ([^;]+);", fields) for n in decl.split(",")]
    assert names == [n for n, _ in built_lib._LatticeSubset._fields_] == ["lat", "num_active", "num_batches", "tile_bs", "d_slot"]
    S = built_lib._LatticeSubset
    assert S.lat.offset == 0 and S.num_active.offset == ctypes.sizeof(built_lib._Lattice) == 56 and S.d_slot.offset == 72 and ctypes.sizeof(S) == 80


# ---- what the calls refuse -------------------------------------------------------------------------------------------------------
def _fake(n):
    """n pointers that are not null and are never followed: a refused call reads no device memory."""
    return (ctypes.c_void_p * n)(*([0x1000] * n))


def _flags(lat, ids):
    return (ctypes.c_int * lat.num_tiles)(*[1 if t in ids else 0 for t in range(lat.num_tiles)])


def test_subset_make_and_bboxes(built_lib, monkeypatch):
    E, L = built_lib, built_lib.lib()
    lat = E.Lattice(W, H, TILE, TILE, OV, BS, 5, 3)
    g = lr.lattice(W, H, TILE, TILE, OV, BS, 5, 3)
    assert lat.num_tiles == 12
    sub = E._LatticeSubset()
    ctypes.memset(ctypes.byref(sub), 0x55, ctypes.sizeof(sub))
    before = bytes(sub)
    for args, text in [((lat.ref, _flags(lat, ()), BS, 0x1000), r"mdtile_lattice_subset_make: no active tile: num_active = 0 outside \[1, 12\]"),
                       ((lat.ref, _flags(lat, (1,)), 0, 0x1000), "mdtile_lattice_subset_make: bad tile_bs=0"),
                       ((lat.ref, _flags(lat, (1,)), BS, None), "mdtile_lattice_subset_make: null d_slot"),
                       ((lat.ref, None, BS, 0x1000), "mdtile_lattice_subset_make: null argument")]:
        assert L.mdtile_lattice_subset_make(*args, ctypes.byref(sub)) == E.E_ARG
        assert re.search(text, L.mdtile_last_error().decode()), L.mdtile_last_error()
        assert bytes(sub) == before, "a refused mdtile_lattice_subset_make wrote to the struct"
    broken = E._Lattice(*[getattr(lat._c, n) for n, _ in E._Lattice._fields_])
    broken.sx = 0
    assert L.mdtile_lattice_subset_make(ctypes.byref(broken), _flags(lat, (1,)), BS, 0x1000, ctypes.byref(sub)) == E.E_ARG
    assert re.search(r"mdtile_lattice_subset_make: shift sx = 0 outside", L.mdtile_last_error().decode())
    many = E.Lattice(100, 100, 10, 10, 5, 1, 5, 5)
    assert L.mdtile_lattice_subset_make(many.ref, _flags(many, range(many.num_tiles - 1)), 1, 0x1000, ctypes.byref(sub)) == E.E_ARG
    assert re.search(r"mdtile_lattice_subset_make: 360 active tiles make 360 batches > MDTILE_MAX_BATCHES=320", L.mdtile_last_error().decode())
    assert bytes(sub) == before
    # the largest tile batch size: ceil(Ta / tile_bs) is formed without a sum that could pass INT_MAX
    assert L.mdtile_lattice_subset_make(lat.ref, _flags(lat, (1, 2, 5)), 2 ** 31 - 1, 0x1000, ctypes.byref(sub)) == 0
    assert (sub.num_active, sub.num_batches, sub.tile_bs) == (3, 1, 3)
    buf = (ctypes.c_int * 12)()
    assert L.mdtile_lattice_subset_bboxes(ctypes.byref(sub), _flags(lat, (1, 2, 5)), buf, None) == 0 and list(buf)[:4] == list(g.boxes[1])
    huge_bs = E._LatticeSubset.from_buffer_copy(bytes(sub))
    huge_bs.tile_bs = 2 ** 31 - 1
    assert L.mdtile_lattice_subset_bboxes(ctypes.byref(huge_bs), _flags(lat, (1, 2, 5)), buf, None) == E.E_ARG
    assert "1 batches of 2147483647 for 3 active tiles" in L.mdtile_last_error().decode()
    # the binding's class, with a slot table that is never read on the host
    monkeypatch.setattr(E, "_dev_tensor", lambda t, name, dtype=None: t)
    for ids_ in [(0,), (11,), (1, 2, 5, 6, 7), tuple(range(12)), tuple(range(0, 12, 2))]:
        flags = [1 if t in ids_ else 0 for t in range(12)]
        s = E.LatticeSubset(lat, flags, BS, torch.tensor(ls.slots(flags), dtype=torch.int32))
        assert (s.num_active, s.ids) == (len(ids_), ids_) and (s.num_batches, s.tile_bs) == ls.batching(len(ids_), BS)
        assert s.bboxes == [g.boxes[t] for t in ids_] and [len(b) for b in s.batches] == [min(s.tile_bs, len(ids_) - i * s.tile_bs) for i in range(s.num_batches)]
        buf = (ctypes.c_int * (4 * 12))()
        assert L.mdtile_lattice_subset_bboxes(s.ref, _flags(lat, ids_[1:]), buf, None) == E.E_ARG
        assert re.search(r"mdtile_lattice_subset_bboxes: %d flags are set, the subset has %d" % (len(ids_) - 1, len(ids_)), L.mdtile_last_error().decode())
    with pytest.raises(E.MdtileError, match="no active tile"):
        E.LatticeSubset(lat, [0] * 12, BS, torch.zeros(12, dtype=torch.int32))
    with pytest.raises(E.MdtileError, match="11 flags for 12 tiles"):
        E.LatticeSubset(lat, [1] * 11, BS, torch.zeros(12, dtype=torch.int32))


def test_calls_refuse_before_any_device_is_touched(built_lib):
    E, L = built_lib, built_lib.lib()
    lat = E.Lattice(W, H, TILE, TILE, OV, BS, 5, 3)
    sub = E._LatticeSubset()
    assert L.mdtile_lattice_subset_make(lat.ref, _flags(lat, (1, 2, 5, 6, 7)), BS, 0x1000, ctypes.byref(sub)) == 0
    assert (sub.num_active, sub.num_batches, sub.tile_bs) == (5, 2, 3)
    nb = sub.num_batches

    def copy(**kw):
        c = E._LatticeSubset.from_buffer_copy(bytes(sub))
        for k, v in kw.items():
            if k.startswith("lat_"):
                setattr(c.lat, k[4:], v)
            else:
                setattr(c, k, v)
        return c

    def blend(text, sub_c=None, nbat=nb, fill=0x1000, **kw):
        f = dict(method=E.METHOD_MD, dtype=0, N=2, C=4, flags=0, tile_lo=0, tile_hi=0, row_lo=0, row_hi=0, d_weights=None, d_tile_w=None, d_rescale=None,
                 d_x_out=0x1000)
        f.update(kw)
        a = E._BlendArgs(**f)
        assert L.mdtile_blend_lattice_sparse(ctypes.byref(sub_c if sub_c is not None else sub), ctypes.byref(a), _fake(max(nbat, 1)), nbat, fill, None) == E.E_ARG
        err = L.mdtile_last_error().decode()
        assert err.startswith("mdtile_blend_lattice_sparse: ") and re.search(text, err), err

    def gather(text, sub_c=None, nbat=nb, dtype=0, N=2, C=4, x=0x1000):
        assert L.mdtile_gather_all_lattice_sparse(ctypes.byref(sub_c if sub_c is not None else sub), dtype, N, C, x, _fake(max(nbat, 1)), nbat, None) == E.E_ARG
        err = L.mdtile_last_error().decode()
        assert err.startswith("mdtile_gather_all_lattice_sparse: ") and re.search(text, err), err

    def activity(text, lat_ref=lat.ref, mask=0x1000, planes=1, active=0x1000, slot=0x1000):
        assert L.mdtile_lattice_activity(lat_ref, mask, planes, active, slot, None) == E.E_ARG
        err = L.mdtile_last_error().decode()
        assert err.startswith("mdtile_lattice_activity: ") and re.search(text, err), err

    # what mdtile_blend_lattice / mdtile_gather_all_lattice refuse
    blend("no MDTILE_BLEND_\\* flags", flags=E.BLEND_PARTIAL)
    blend("no row band", row_lo=0, row_hi=8)
    blend("d_weights and d_rescale must be NULL", d_weights=0x1000)
    blend("d_weights and d_rescale must be NULL", d_rescale=0x1000, method=E.METHOD_MOD, d_tile_w=0x1000)
    blend("Mixture of Diffusers needs d_tile_w", method=E.METHOD_MOD)
    blend("bad method", method=2)
    blend("bad dtype", dtype=3)
    blend("bad N=0", N=0)
    blend("bad N=2 C=40000", C=40000)
    blend("null output", d_x_out=None)
    gather("bad dtype", dtype=-1)
    gather("bad N=2 C=40000", C=40000)
    gather("null argument", x=None)
    # the subset's own
    blend("null fill", fill=None)
    blend(r"%d batches given, the subset has %d" % (nb + 1, nb), nbat=nb + 1)
    gather(r"%d batches given, the subset has %d" % (nb - 1, nb), nbat=nb - 1)
    for kw, text in [(dict(lat_sx=0), r"sx = 0 outside \[1, 12\]"), (dict(lat_cols=5), "tiles along x"), (dict(lat_num_tiles=13), "bad lattice"),
                     (dict(num_active=0), r"num_active = 0 outside \[1, 12\]"), (dict(num_active=13), r"num_active = 13 outside \[1, 12\]"),
                     (dict(num_batches=1), "1 batches of 3 for 5 active tiles"), (dict(tile_bs=4), "2 batches of 4 for 5 active tiles"),
                     (dict(num_batches=0), "bad subset"), (dict(tile_bs=0), "bad subset"), (dict(d_slot=None), "null d_slot")]:
        blend(text, sub_c=copy(**kw))
        gather(text, sub_c=copy(**kw))
        buf = (ctypes.c_int * 64)()
        assert L.mdtile_lattice_subset_bboxes(ctypes.byref(copy(**kw)), _flags(lat, (1, 2, 5, 6, 7)), buf, None) == E.E_ARG
        assert L.mdtile_last_error().decode().startswith("mdtile_lattice_subset_bboxes: ")
    # a consistent subset with more batches than the argument block carries (made by hand: subset_make refuses it)
    many = E.Lattice(100, 100, 10, 10, 5, 1, 5, 5)
    big = E._LatticeSubset(many._c, 360, 360, 1, 0x1000)
    blend("MDTILE_MAX_BATCHES", sub_c=big, nbat=360)
    gather("MDTILE_MAX_BATCHES", sub_c=big, nbat=360)
    # Ta == T is allowed: the checks pass up to the batch count
    full = E._LatticeSubset()
    assert L.mdtile_lattice_subset_make(lat.ref, _flags(lat, range(12)), BS, 0x1000, ctypes.byref(full)) == 0 and full.num_active == 12
    blend("4 batches given, the subset has 3", sub_c=full, nbat=4)
    # the activity
    activity("bad planes=0", planes=0)
    activity("bad planes=-1", planes=-1)
    activity("null argument", mask=None)
    activity("null argument", active=None)
    activity("null argument", slot=None)
    broken = E._Lattice(*[getattr(lat._c, n) for n, _ in E._Lattice._fields_])
    broken.sy = 13
    activity(r"sy = 13 outside \[1, 12\]", lat_ref=ctypes.byref(broken))
    huge = E.Lattice(4000, 4000, 16, 16, 4, 4096, 5, 5)
    assert huge.num_tiles > 65535
    activity("at most 65535", lat_ref=huge.ref)


# ---- the option ------------------------------------------------------------------------------------------------------------------
def test_preload_option(host):
    pl, shared = host
    parser = argparse.ArgumentParser()
    load_preload().preload(parser)
    assert parser.parse_args([]).mdtile_jitter_inpaint_skip is False
    got = parser.parse_args(["--mdtile-jitter-inpaint-skip"])
    assert got.mdtile_jitter_inpaint_skip is True and got.mdtile_grid_jitter is False and got.mdtile_inpaint_skip is False
    A = pl.abstractdiffusion.AbstractDiffusion
    assert not hasattr(shared.cmd_opts, "mdtile_jitter_inpaint_skip") and A.jitter_inpaint_skip_requested() is False
    shared.cmd_opts.mdtile_jitter_inpaint_skip = True
    try:
        assert A.jitter_inpaint_skip_requested() is True
    finally:
        del shared.cmd_opts.mdtile_jitter_inpaint_skip
    helps = {a.dest: a.help for a in parser._actions}
    assert "--mdtile-jitter-inpaint-skip" in helps["mdtile_grid_jitter"] and "--mdtile-jitter-inpaint-skip" in helps["mdtile_inpaint_skip"]


# ---- wiring ----------------------------------------------------------------------------------------------------------------------
OPTIONS = ("mdtile_grid_jitter", "mdtile_inpaint_skip", "mdtile_jitter_inpaint_skip", "mdtile_jitter_regions", "mdtile_grid_shift", "mdtile_wrap_x",
           "mdtile_wrap_y")


class Bar:
    """What the delegates ask of tqdm."""

    def __init__(self, total):
        self.total, self.n, self.closed = total, 0, False

    def update(self, n=1):
        self.n += n

    def refresh(self):
        pass

    def close(self):
        self.closed = True


@pytest.fixture
def skipping(wired, monkeypatch):
    """(plugin, shared, calls): wired, the options gone before and after, the step counter restored, every engine call of the paths involved
    replaced by a double that appends its name (and its grid) to `calls`; the host integers (Lattice, LatticeSubset, Plan.subset) are real."""
    pl, shared = wired
    E = pl.engine
    calls = []

    def ref_lattice(lat):
        g = lr.lattice(lat.w, lat.h, TILE, TILE, OV, BS, lat.sx, lat.sy)
        assert list(g.boxes) == lat.bboxes
        return g

    def lattice_activity(lat, mask):
        flags = ls.activity(ref_lattice(lat), mask.numpy())
        calls.append(("activity", lat, tuple(flags)))
        return flags, torch.tensor(ls.slots(flags), dtype=torch.int32)

    def gather_all_lattice_sparse(sub, x_in, out=None):
        calls.append(("sparse gather", sub))
        g = ref_lattice(sub.lat)
        return [torch.from_numpy(ls.gather(g, x_in.numpy(), sub.ids[i * sub.tile_bs:(i + 1) * sub.tile_bs])) for i in range(sub.num_batches)]

    def blend_lattice_sparse(sub, method, batch_out, N_, C_, *, fill, tile_w=None, **kw):
        assert not kw and len(batch_out) == sub.num_batches and (tile_w is not None) == (method == E.METHOD_MOD)
        assert [t.shape[0] for t in batch_out] == [len(b) * N_ for b in sub.batches]
        calls.append(("sparse blend", sub, fill))
        return torch.zeros(N_, C_, sub.h, sub.w)

    def gather_all_lattice(lat, x_in, out=None):
        calls.append(("gather", lat))
        g = ref_lattice(lat)
        return [torch.from_numpy(lr.gather(g, x_in.numpy(), b)) for b in range(len(g.batches))]

    def blend_lattice(lat, method, batch_out, N_, C_, *, tile_w=None, **kw):
        assert not kw and len(batch_out) == lat.num_batches
        calls.append(("blend", lat))
        return torch.zeros(N_, C_, lat.h, lat.w)

    def tile_activity(plan, mask):
        calls.append(("plain activity",))
        return sr.activity(sr.grid(plan.w, plan.h, TILE, TILE, OV, BS), mask.numpy())

    def gather_all(plan, x_in, out=None):
        calls.append(("plain gather", plan))
        return [torch.zeros(len(b) * x_in.shape[0], x_in.shape[1], plan.tile_h, plan.tile_w) for b in plan.batches]

    monkeypatch.setattr(E, "_dev_tensor", lambda t, name, dtype=None: t)
    for name, fn in (("lattice_activity", lattice_activity), ("gather_all_lattice_sparse", gather_all_lattice_sparse),
                     ("blend_lattice_sparse", blend_lattice_sparse), ("gather_all_lattice", gather_all_lattice), ("blend_lattice", blend_lattice),
                     ("tile_activity", tile_activity), ("gather_all", gather_all)):
        monkeypatch.setattr(E, name, fn)
    monkeypatch.setattr(E, "blend", lambda plan, method, batch_out, N_, C_, **kw: calls.append(("plain blend",)) or torch.zeros(N_, C_, plan.h, plan.w))
    monkeypatch.setattr(E, "blend_sparse", lambda plan, method, batch_out, N_, C_, **kw: calls.append(("plain sparse blend",)) or torch.zeros(N_, C_, plan.h, plan.w))
    monkeypatch.setattr(shared.state, "sampling_step", 0)
    for n in OPTIONS:
        if hasattr(shared.cmd_opts, n):
            monkeypatch.delattr(shared.cmd_opts, n)
    yield pl, shared, calls
    for n in OPTIONS:
        if hasattr(shared.cmd_opts, n):
            delattr(shared.cmd_opts, n)


def _job(pl, shared, mask, method="md", options=("mdtile_grid_jitter", "mdtile_inpaint_skip", "mdtile_jitter_inpaint_skip")):
    for k in options:
        setattr(shared.cmd_opts, k, True)
    d, p = delegate(pl, W, H, TILE, TILE, OV, BS, method)
    p.all_seeds = [SEED]
    if mask is not None:
        p.nmask = torch.from_numpy(mask)
    if method == "mod":
        d.rescale_factor = torch.ones(1, 1, H, W)
    return d, p


def _evaluate(d, shared, method, x, seen):
    if method == "md":
        def repeat(xt, bboxes):
            seen.append((xt, list(bboxes)))
            return xt
        return d.sample_one_step(x, None, repeat, None)
    shared.sd_model.apply_model_original_md = lambda x_, t_, c_: seen.append((x_, None)) or x_
    return d.apply_model_hijack(x, torch.zeros(N), {"c_crossattn": [torch.zeros(N, 77, 8)], "c_concat": [torch.zeros(N, 5, 1, 1)]})


def _want(step, mask):
    g = lr.lattice(W, H, TILE, TILE, OV, BS, *lr.step_shift(W, H, TILE, TILE, OV, SEED, step))
    return g, ls.activity(g, mask)


FACE = _mask([(y, x) for y in range(9, 13) for x in range(17, 22)])       # a block in the middle of the canvas


@pytest.mark.parametrize("method", ["md", "mod"])
def test_one_decision_per_step_and_only_the_active_tiles_run(skipping, capsys, method):
    pl, shared, calls = skipping
    d, p = _job(pl, shared, FACE, method)
    assert d.grid_jitter and "Tiled Diffusion jitter inpaint skip" not in (getattr(p, "extra_generation_params", None) or {})
    x = torch.randn(N, C, H, W)
    subsets = []
    for step in (0, 0, 1, 2, 2):
        shared.state.sampling_step = step
        del calls[:]
        seen = []
        out = _evaluate(d, shared, method, x, seen)
        g, active = _want(step, FACE)
        Ta, T = sum(active), len(active)
        assert 0 < Ta < T, "the test's mask must leave tiles to skip"
        assert tuple(out.shape) == (N, C, H, W)
        names = [c[0] for c in calls]
        assert names == (["activity"] if step not in [s for s, _ in subsets] else []) + ["sparse gather", "sparse blend"], (step, names)
        sub = calls[-1][1]
        assert calls[-2][1] is sub and calls[-1][2] is x
        assert sub.ids == ls.ids(active) and sub.num_active == Ta and (sub.num_batches, sub.tile_bs) == ls.batching(Ta, BS)
        assert sum(t.shape[0] for t, _ in seen) == Ta * N and len(seen) == sub.num_batches, "the model runs the active tiles and no other"
        if method == "md":      # the boxes handed on with every batch (image conditioning, ControlNet, StableSR follow them) are the active pushed-in boxes
            assert [(b.x, b.y, b.w, b.h) for _, bb in seen for b in bb] == [g.boxes[t] for t in sub.ids]
        want = ls.gather(g, x.numpy(), sub.ids)
        assert torch.equal(torch.cat([t for t, _ in seen]), torch.from_numpy(want))
        subsets.append((step, sub))
    assert subsets[0][1] is subsets[1][1] and subsets[3][1] is subsets[4][1] and subsets[0][1] is not subsets[2][1]
    assert len({(s.lat.sx, s.lat.sy) for _, s in subsets}) == 3
    assert p.extra_generation_params["Tiled Diffusion jitter inpaint skip"] is True and p.extra_generation_params["Tiled Diffusion grid jitter"] is True
    text = capsys.readouterr().out
    g0, a0 = _want(0, FACE)
    assert text.count("[Tiled Diffusion]") == 1 and f"inpaint mask touches {sum(a0)} of {len(a0)} tiles of the first step's grid" in text


def test_the_empty_step_calls_nothing_and_returns_a_fresh_tensor(skipping):
    pl, shared, calls = skipping
    d, _ = _job(pl, shared, np.zeros((1, H, W), np.float32))
    x = torch.randn(N, C, H, W)
    seen = []
    for step in (0, 1):
        shared.state.sampling_step = step
        out = _evaluate(d, shared, "md", x, seen)
        assert torch.equal(out, x) and out is not x
    assert not seen and [c[0] for c in calls] == ["activity", "activity"]


@pytest.mark.parametrize("method", ["md", "mod"])
def test_all_active_runs_the_old_calls(skipping, method):
    pl, shared, calls = skipping
    d, _ = _job(pl, shared, np.full((1, H, W), -0.5, np.float32), method)
    seen = []
    _evaluate(d, shared, method, torch.randn(N, C, H, W), seen)
    assert [c[0] for c in calls] == ["activity", "gather", "blend"] and calls[1][1] is calls[2][1] is calls[0][1]
    assert sum(t.shape[0] for t, _ in seen) == calls[0][1].num_tiles * N


def test_too_many_compact_batches_run_the_full_lattice(skipping, capsys, monkeypatch):
    pl, shared, calls = skipping
    d, _ = _job(pl, shared, np.concatenate([_mask([(0, 0)]), _mask([(H - 1, W - 1)])]))
    monkeypatch.setattr(pl.engine, "MAX_BATCHES", 0)       # after the grid was planned: the full lattice passed its own check there
    x = torch.randn(N, C, H, W)
    for step in (0, 1):
        shared.state.sampling_step = step
        _evaluate(d, shared, "md", x, [])
    assert [c[0] for c in calls] == ["activity", "gather", "blend"] * 2
    text = capsys.readouterr().out
    assert text.count("--mdtile-inpaint-skip not applied") == 1 and "more than the 0 a lattice subset carries" in text


@pytest.mark.parametrize("method", ["md", "mod"])
def test_without_the_switch_the_old_line_and_the_fixed_grid(skipping, capsys, method):
    pl, shared, calls = skipping
    d, p = _job(pl, shared, FACE, method, options=("mdtile_grid_jitter", "mdtile_inpaint_skip"))
    x = torch.randn(N, C, H, W)
    for step in (0, 1):
        shared.state.sampling_step = step
        _evaluate(d, shared, method, x, [])
    assert [c[0] for c in calls] == ["plain activity", "plain gather", "plain sparse blend", "plain gather", "plain sparse blend"]
    assert d.skip_mode == "sparse" and calls[1][1] is d.sparse_plan
    text = capsys.readouterr().out
    assert '--mdtile-inpaint-skip decided "sparse" for this job (tiles are skipped on the fixed grid)' in text
    assert text.count("--mdtile-grid-jitter not applied") == 1 and "jitter-inpaint-skip" not in text
    assert "Tiled Diffusion jitter inpaint skip" not in (getattr(p, "extra_generation_params", None) or {})


@pytest.mark.parametrize("options,missing", [(("mdtile_jitter_inpaint_skip",), "--mdtile-grid-jitter and --mdtile-inpaint-skip"),
                                             (("mdtile_jitter_inpaint_skip", "mdtile_grid_jitter"), "--mdtile-inpaint-skip is"),
                                             (("mdtile_jitter_inpaint_skip", "mdtile_inpaint_skip"), "--mdtile-grid-jitter is")])
def test_ignored_without_its_companions(skipping, capsys, options, missing):
    pl, shared, calls = skipping
    d, _ = _job(pl, shared, FACE, options=options)
    x = torch.randn(N, C, H, W)
    for step in (0, 1):
        shared.state.sampling_step = step
        _evaluate(d, shared, "md", x, [])
    text = capsys.readouterr().out
    assert text.count("--mdtile-jitter-inpaint-skip ignored") == 1 and missing in text
    names = [c[0] for c in calls]
    if "mdtile_grid_jitter" in options:
        assert names == ["gather", "blend"] * 2                       # jitter alone: every tile of the moving grid
    elif "mdtile_inpaint_skip" in options:
        assert names == ["plain activity"] + ["plain gather", "plain sparse blend"] * 2
    else:
        assert names == ["plain gather", "plain blend"] * 2


def test_the_preconditions_of_the_skip_keep_their_lines_and_the_full_lattice_runs(skipping, capsys):
    pl, shared, calls = skipping
    d, _ = _job(pl, shared, None)                                        # no p.nmask
    x = torch.randn(N, C, H, W)
    _evaluate(d, shared, "md", x, [])
    assert [c[0] for c in calls] == ["gather", "blend"] and d.skip_mode == "full"
    text = capsys.readouterr().out
    assert "--mdtile-inpaint-skip not applied: the job has no inpaint mask (p.nmask)" in text
    del calls[:]
    d, _ = _job(pl, shared, _mask([(0, 0)], w=W + 1))                     # a mask of another size
    _evaluate(d, shared, "md", x, [])
    assert [c[0] for c in calls] == ["gather", "blend"] and "the mask has size" in capsys.readouterr().out


def test_noise_inversion_runs_the_fixed_grid_with_every_tile(skipping, capsys):
    pl, shared, calls = skipping
    d, _ = _job(pl, shared, FACE)
    x = torch.randn(1, C, H, W)
    cond = {"c_crossattn": [torch.zeros(1, 77, 8)], "c_concat": [torch.zeros(1, 5, 1, 1)]}
    shared.sd_model.apply_model = lambda x_, t_, cond=None: x_
    d.get_noise(x, torch.zeros(1), cond, 0)
    assert [c[0] for c in calls] == ["plain gather", "plain blend"] and calls[0][1] is d.plan
    del calls[:]
    _evaluate(d, shared, "md", torch.randn(N, C, H, W), [])            # the sampler's own evaluations skip on the moving grid
    assert [c[0] for c in calls] == ["activity", "sparse gather", "sparse blend"]


def test_the_bar_ends_at_the_calls_made(skipping):
    pl, shared, calls = skipping
    mask = FACE
    d, _ = _job(pl, shared, mask)
    steps = 4
    shared.state.sampling_steps = steps
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    budget = d.total_bboxes
    assert budget == 3                                                   # the largest lattice: 12 tiles in batches of 4
    d.pbar = Bar(budget * steps)
    x = torch.randn(N, C, H, W)
    made = 0
    for step in range(steps):
        shared.state.sampling_step = step
        for _ in range(2):                                               # cond and uncond: one decision, one adjustment
            seen = []
            _evaluate(d, shared, "md", x, seen)
        g, active = _want(step, mask)
        made += ls.batching(sum(active), BS)[0]
    assert d.pbar.total == made < budget * steps


def test_the_bar_does_not_overrun_with_one_evaluation_per_step(skipping):
    """The left half of the canvas: steps of two compact batches, so the bar advances; its count never passes its total, which ends at the batches run."""
    pl, shared, calls = skipping
    mask = _mask([(y, x) for y in range(H) for x in range(W // 2)])
    d, _ = _job(pl, shared, mask)
    steps = 6
    shared.state.sampling_steps = steps
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    d.pbar = Bar(d.total_bboxes * steps)
    x = torch.randn(N, C, H, W)
    made, per_step = 0, []
    for step in range(steps):
        shared.state.sampling_step = step
        _evaluate(d, shared, "md", x, [])
        g, active = _want(step, mask)
        assert 0 < sum(active) < len(active)
        per_step.append(ls.batching(sum(active), BS)[0])
        made += per_step[-1]
        assert d.pbar.n <= made and d.pbar.n <= d.pbar.total, (step, d.pbar.n, d.pbar.total)
    assert max(per_step) >= 2 and d.pbar.n > 0, "the mask must make the bar advance"
    assert d.pbar.total == made and d.pbar.n <= made


def test_the_random_generators_are_left_alone(skipping):
    pl, shared, calls = skipping
    d, _ = _job(pl, shared, FACE)
    x = torch.randn(N, C, H, W)
    torch_state, numpy_state = torch.get_rng_state(), np.random.get_state()
    for step in range(5):
        shared.state.sampling_step = step
        _evaluate(d, shared, "md", x, [])
    assert len({(c[1].lat.sx, c[1].lat.sy) for c in calls if c[0] == "sparse blend"}) > 1
    assert torch.equal(torch.get_rng_state(), torch_state)
    after = np.random.get_state()
    assert after[0] == numpy_state[0] and np.array_equal(after[1], numpy_state[1]) and after[2:] == numpy_state[2:]
