"""The blend dispatch, observed without a GPU: mdtile_blend_dispatch is the host function the launcher itself calls (csrc/blend.hip), so
what it answers here is what a launch gets on the device.  Every case of tests/blend_matrix_cases.py must land on the kernel and the
planes-per-block it is labelled with, and together the cases must reach every k_blend_lds instantiation that ships (3 dtypes x 2 methods
x LPP {4, 2, 1} x packed / unpacked = 36) and, per dtype, k_blend on its vector and its element path -- a geometry that drifts off the
path it was written for fails here instead of silently testing something else."""
import itertools

import pytest
import torch

import blend_matrix_cases as bm

TORCH_DTYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def _query(E, plans, c):
    if c.geom not in plans:
        plans[c.geom] = E.Plan(*bm.GEOMETRIES[c.geom])
    plan = plans[c.geom]
    kw = {}
    if c.mode in ("rows", "band"):
        kw["row_range"] = bm.row_band(plan)
    if c.mode in ("partial", "band"):
        kw["partial"], kw["tile_range"] = True, bm.tile_ranges(plan)[0][0]
    return plan, E.blend_dispatch(plan, TORCH_DTYPE[c.dtype], c.N, c.C, packed=c.packed, aligned=c.aligned, **kw)


def test_case_ids_are_unique():
    ids = [c.id for c in bm.CASES]
    assert len(ids) == len(set(ids))


def test_every_case_lands_on_its_labelled_kernel(built_lib):
    E, plans = built_lib, {}
    for c in bm.CASES:
        plan, d = _query(E, plans, c)
        if c.kernel == "lds":
            assert d.lds and d.planes == c.lpp, f"{c.id}: labelled k_blend_lds LPP {c.lpp}, dispatch says {d}"
            row_bytes = plan.tile_w * (4 if c.dtype == "f32" else 2)
            assert d.shape == 256 and 0 < d.lds_bytes <= 64 * 1024 and d.lds_bytes == _nr_max(plan) * d.ncs * (row_bytes + 32) * d.planes, c.id
        else:
            assert not d.lds and d.lds_bytes == 0, f"{c.id}: labelled k_blend, dispatch says {d}"
            assert ((d.vec_quads > 0), (d.elem_quads > 0)) == ("vec" in c.paths, "elem" in c.paths) and d.walk_quads == 0, f"{c.id}: {d}"
            assert (c.N * c.C) % d.planes == 0 and (d.planes, d.shape) in ((8, 4), (8, 2), (4, 4), (4, 2), (2, 4), (1, 4)), f"{c.id}: {d}"


def _nr_max(plan):
    ys = sorted(set(b[1] for b in plan.bboxes))
    return max(sum(1 for y0 in ys if y0 <= y < y0 + plan.tile_h) for y in range(plan.h))


def test_cases_reach_every_shipping_instantiation(built_lib):
    E, plans = built_lib, {}
    lds, plain = set(), set()
    modes = set()
    for c in bm.CASES:
        _, d = _query(E, plans, c)
        packed = c.packed or plans[c.geom].num_batches > E.MAX_BATCHES
        if d.lds:
            lds.add((c.dtype, c.method, d.planes, packed))
            modes.add((c.dtype, c.method, d.planes, c.mode))
        else:
            plain.update((c.dtype, p) for p, n in (("vec", d.vec_quads), ("elem", d.elem_quads)) if n > 0)
    want = set(itertools.product(bm.DTYPES, bm.METHODS, (4, 2, 1), (False, True)))
    assert lds == want, f"k_blend_lds instantiations no case reaches: {sorted(want - lds)}"
    assert plain == set(itertools.product(bm.DTYPES, ("vec", "elem"))), plain
    # the rank modes are runtime flags of those instantiations: every (dtype, method, LPP) runs each of them
    want_modes = set(itertools.product(bm.DTYPES, bm.METHODS, (4, 2, 1), ("full", "rows", "partial", "band")))
    assert want_modes <= modes, sorted(want_modes - modes)


def test_dispatch_rules_one_by_one(built_lib):
    """The rules of the launcher, each on a geometry that differs from an LDS one in that rule alone."""
    E = built_lib
    f32, f16 = torch.float32, torch.float16
    odd = E.Plan(*bm.GEOMETRIES["odd200"])
    assert E.blend_dispatch(odd, f32, 2, 4).lds and E.blend_dispatch(odd, f16, 2, 4).lds
    assert not E.blend_dispatch(odd, f32, 2, 4, aligned=False).lds                      # misaligned batch pointers
    assert not E.blend_dispatch(odd, f32, 2, 4, num_batches=0).lds                      # no grid (regions only)
    assert not E.blend_dispatch(E.Plan(200, 136, 96, 96, 8, 4), f32, 2, 4).lds           # origins 0, 52, 104: all multiples of 4 -> k_blend ties or wins
    assert not E.blend_dispatch(E.Plan(200, 136, 96, 96, 80, 4), f32, 2, 4).lds          # > 3 covering tiles per axis
    assert E.blend_dispatch(E.Plan(*bm.GEOMETRIES["lanes64"]), f32, 2, 4).lds            # 1 KiB rows: the last size one wave-instruction moves
    assert not E.blend_dispatch(E.Plan(*bm.GEOMETRIES["lanes33"]), f32, 2, 4).lds        # 1056-byte rows
    assert not E.blend_dispatch(E.Plan(*bm.GEOMETRIES["row200B"]), f16, 2, 4).lds        # 200-byte rows are no whole 16-byte records
    big = E.Plan(*bm.GEOMETRIES["b441"])
    assert [E.blend_dispatch(big, dt, 2, 4).planes for dt in (f32, f16)] == [2, 4]       # LPP by stage size (<= 64 KB)
    # a flag changes the launch's work, not the kernel; k_blend's planes per thread follow the rows of the launch
    full = E.blend_dispatch(odd, f32, 2, 4)
    for kw in (dict(partial=True, tile_range=(0, 4)), dict(row_range=(35, 102)), dict(packed=True)):
        assert E.blend_dispatch(odd, f32, 2, 4, **kw)[:5] == full[:5], kw
    wide = E.Plan(1024, 1024, 128, 128, 8, 4)                                            # origins 0, 112, 224, ...
    assert E.blend_dispatch(wide, f32, 2, 4)[:3] == (E.BLEND_KERNEL_PLAIN, 8, 2)
    assert E.blend_dispatch(wide, f32, 2, 4, row_range=(0, 256))[:3] == (E.BLEND_KERNEL_PLAIN, 4, 4)
    with pytest.raises(E.MdtileError, match="batches given"):
        E.blend_dispatch(odd, f32, 2, 4, num_batches=odd.num_batches + 1)
    with pytest.raises(E.MdtileError, match="bad row range"):
        E.blend_dispatch(odd, f32, 2, 4, row_range=(10, 137))
