"""A/B of region control under the jittered grid (csrc/lattice.hip: k_lattice_blend<..., REGIONS>) against the calls of before,
the protocol of probes/shift_ab.py: one process, COLD (rotating buffer sets larger than the 256 MiB Infinity Cache), 20 back-to-back
evaluations per HIP-event pair, median of 7 rounds, the arms ALTERNATING inside every round in an order rotated per round -- at latent 1024^2,
tile 128 / overlap 0 and 128 / 8, fp32 and fp16, N = 2, C = 4, MultiDiffusion and Mixture of Diffusers, at rest and at the shift (5, 3).  One
evaluation = every gather + the blend:
    (a) rest / (5, 3)   mdtile_gather_all_lattice + mdtile_blend_lattice: no regions.  The baseline; its kernels are the parent commit's (the device
                        code of lattice.hip was compared with the parent's and is identical)
    (b) rest / (5, 3)   the same gather + mdtile_blend_lattice_regions with 0 regions and a NULL region map: what the new kernel costs a job that
                        never takes it
    (c) rest / (5, 3)   + 4 regions, 2 background + 2 foreground, each a quarter of the canvas: 4 mdtile_gather_rect and the region tail
    plain + regions     beside (c): mdtile_gather_all + 4 mdtile_gather_rect + mdtile_blend on the PLAIN plan of the same size with the same regions
(b) is checked first against (a), bitwise.  Jobs without regions never take (b): it is here to price the kernel, not to replace a call.
    python probes/lattice_regions_ab.py            (on the GPU box; the shipping library)"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd"))
import mdtile as E          # noqa: E402

dev = torch.device("cuda:0")
N, C, BS = 2, 4, 8
N_CALLS, ROUNDS = 20, 7


def timed_alternating(arms):
    """arms: name -> list of callables (one per buffer set).  Every round times each arm once, in an order rotated from round to round
    -> name -> (median us, best us)."""
    for calls in arms.values():
        for c in calls[:3]:
            c()
    ts = {name: [] for name in arms}
    names = list(arms)
    for r in range(ROUNDS):
        for name in names[r % len(names):] + names[:r % len(names)]:
            calls = arms[name]
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(N_CALLS):
                calls[i % len(calls)]()
            e.record()
            torch.cuda.synchronize()
            ts[name].append(s.elapsed_time(e) / N_CALLS * 1e3)
    return {name: (sorted(t)[len(t) // 2], min(t)) for name, t in ts.items()}


def quarter_regions(W, H):
    """(x, y, w, h, mode): 2 BG + 2 FG, each W/2 x H/2, overlapping one another, all inside the canvas."""
    w, h = W // 2, H // 2
    return [(W // 8, H // 8, w, h, E.REGION_BG), (3 * W // 8, H // 4, w, h, E.REGION_BG), (W // 2, H // 2, w, h, E.REGION_FG),
            (W // 4, 3 * H // 8, w, h, E.REGION_FG)]


class Evaluation:
    """One evaluation on fixed buffers, its C arguments built once.  kind: "old" (mdtile_blend_lattice), "new" (mdtile_blend_lattice_regions with
    `regions`), "plain" (mdtile_gather_all + mdtile_blend on a plain plan with `regions`)."""

    def __init__(self, kind, grid, method, x, tiles, out, maps, regions):
        L_ = E.lib()
        dt, st, nb, xp = E.dtype_code(x.dtype), E._stream(), len(tiles), x.data_ptr()
        W, H = grid.w, grid.h
        m = maps if kind == "plain" else dict(tile_w=maps.get("tile_w"))
        _, self.a, self.ptrs = E._blend_operands(grid, method, tiles, N, C, x.dtype, x.dtype, x.device, out, m.get("weights"), m.get("tile_w"), m.get("rescale"))
        a, ptrs = ctypes.byref(self.a), self.ptrs
        self.routs = [torch.empty(N, C, r[3], r[2], dtype=x.dtype, device=dev) for r in regions]
        self.rw = [torch.rand(r[3], r[2], device=dev) for r in regions]
        self.rarr = (E._Region * max(1, len(regions)))(*[E._Region(r[0], r[1], r[2], r[3], r[4], 0, o.data_ptr(), w.data_ptr())
                                                         for r, o, w in zip(regions, self.routs, self.rw)])
        self.keep = (grid, x, tiles, out, maps)
        steps = []
        if kind == "plain":
            h = grid.handle
            steps.append(lambda: L_.mdtile_gather_all(h, dt, N, C, xp, ptrs, nb, st))
        else:
            ref = grid.ref
            steps.append(lambda: L_.mdtile_gather_all_lattice(ref, dt, N, C, xp, ptrs, nb, st))
        for r, o in zip(regions, self.routs):
            steps.append(lambda r=r, o=o: L_.mdtile_gather_rect(dt, N, C, W, H, xp, r[0], r[1], r[2], r[3], o.data_ptr(), st))
        if kind == "plain":
            rarr, nr = self.rarr, len(regions)
            steps.append(lambda: L_.mdtile_blend(h, a, ptrs, nb, rarr, nr, st))
        elif kind == "old":
            steps.append(lambda: L_.mdtile_blend_lattice(ref, a, ptrs, nb, st))
        else:
            region_w = maps.get("region_w") if regions else None
            self.lr = E._LatticeRegions(self.rarr, len(regions), None if region_w is None else region_w.data_ptr())
            lr = ctypes.byref(self.lr)
            steps.append(lambda: L_.mdtile_blend_lattice_regions(ref, a, ptrs, nb, lr, st))
        self.steps = steps
        for s_ in steps:
            assert s_() == 0, L_.mdtile_last_error()

    def __call__(self):
        for s_ in self.steps:
            s_()


def run(W, H, tile, ov, dtype):
    plain = E.Plan(W, H, tile, tile, ov, BS)
    stride = plain.tile_w - plain.overlap
    lattices = {"rest": E.Lattice(W, H, tile, tile, ov, BS, stride, stride), "(5, 3)": E.Lattice(W, H, tile, tile, ov, BS, 5, 3)}
    es = 4 if dtype == torch.float32 else 2
    regions = quarter_regions(W, H)
    tile_w = E.gaussian_weights(plain.tile_w, plain.tile_h, dev)
    most = max(l.num_tiles for l in lattices.values())
    canvas = es * N * C * H * W
    moved = 2 * most * es * N * C * plain.tile_h * plain.tile_w + 2 * canvas
    sets = max(3, int(700e6 // moved) + 1)
    print(f"\nlatent {W} x {H}, tile {plain.tile_w} / overlap {plain.overlap}, {str(dtype).split('.')[-1]}: "
          + ", ".join(f"{k} {l.num_tiles} tiles in {l.num_batches} batches" for k, l in lattices.items())
          + f" (plain plan: {plain.num_tiles}); N = {N}, C = {C}; up to {moved / 1e6:.0f} MB per gather + blend pair, {sets} buffer sets", flush=True)
    xs = [torch.randn(N, C, H, W, device=dev).to(dtype) for _ in range(sets)]
    outs = [torch.empty(N, C, H, W, dtype=dtype, device=dev) for _ in range(sets)]

    def tile_bufs(grid):
        return [[torch.empty(len(b) * N, C, plain.tile_h, plain.tile_w, dtype=dtype, device=dev) for b in grid.batches] for _ in range(sets)]

    bufs = {k: tile_bufs(l) for k, l in lattices.items()}
    plain_bufs = tile_bufs(plain)
    for method, name in ((E.METHOD_MD, "md "), (E.METHOD_MOD, "mod")):
        md = method == E.METHOD_MD
        region_w = torch.zeros(H, W, device=dev)
        weights = torch.zeros(H, W, device=dev)
        E.weight_map_add_grid(plain, None if md else tile_w, weights)
        for (x, y, w, h, m) in regions:
            if m == E.REGION_BG:
                g = None if md else E.gaussian_weights(w, h, dev)
                E.weight_map_add_rect(region_w, x, y, w, h, g, 1.0)
                E.weight_map_add_rect(weights, x, y, w, h, g, 1.0)
        lat_maps = dict(tile_w=None if md else tile_w, region_w=region_w)
        plain_maps = dict(weights=weights) if md else dict(tile_w=tile_w, rescale=E.reciprocal(weights))

        def evals(kind, key, regs):
            if kind == "plain":
                return [Evaluation(kind, plain, method, xs[i], plain_bufs[i], outs[i], plain_maps, regs) for i in range(sets)]
            return [Evaluation(kind, lattices[key], method, xs[i], bufs[key][i], outs[i], lat_maps, regs) for i in range(sets)]

        # correctness first: (b) == (a), bitwise, at rest and shifted
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        for key in lattices:
            evals("old", key, [])[0]()
            want = outs[0].clone()
            outs[0].fill_(float("nan"))
            evals("new", key, [])[0]()
            print(f"  {name} {key}: blend_lattice_regions(0 regions) == blend_lattice: {torch.equal(outs[0].view(bits), want.view(bits))}", flush=True)

        arms = {}
        for key in lattices:
            arms[f"(a) {key}: gather_all_lattice + blend_lattice"] = evals("old", key, [])
            arms[f"(b) {key}: gather_all_lattice + blend_lattice_regions, 0 regions"] = evals("new", key, [])
            arms[f"(c) {key}: + 4 gather_rect, 4 regions"] = evals("new", key, regions)
        arms["plain plan: gather_all + 4 gather_rect + blend, 4 regions"] = evals("plain", None, regions)
        res = timed_alternating(arms)
        for arm, (med, best) in res.items():
            key = arm.split(":")[0][4:]
            ref = res.get(f"(a) {key}: gather_all_lattice + blend_lattice", res["(a) rest: gather_all_lattice + blend_lattice"])[0]
            print(f"  {name} {arm:72s} {med:8.2f} us (best {best:7.2f})  x{med / ref:5.3f} of (a)", flush=True)


def main():
    for (tile, ov) in ((128, 0), (128, 8)):
        for dtype in (torch.float32, torch.float16):
            run(1024, 1024, tile, ov, dtype)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
