"""A/B of region control on a wrap-around canvas (csrc/wrap.hip: k_walk_blend<..., REGIONS>; csrc/wrap_regions.hip: the rect kernels) against the calls
of before, the protocol of probes/shift_ab.py: one process, COLD (rotating buffer sets larger than the 256 MiB Infinity Cache), 20 back-to-back
evaluations per HIP-event pair, median of 7 rounds, the arms ALTERNATING inside every round -- at latent 1024^2 closed in both axes and
1024 x 512 closed in x, tile 128 / overlap 8 and 96 / 48, fp32 and fp16, N = 2, C = 4, MultiDiffusion and Mixture of Diffusers.  One evaluation =
every gather + the blend:
    (a) rest / shift   mdtile_gather_all + mdtile_blend, mdtile_gather_all_shift + mdtile_blend_shift: no regions.  The baseline; their kernels are
                       the parent commit's (every k_wrap_* / k_walk_blend* instruction stream was compared with the parent's and is identical)
    (b) rest / shift   the same gathers + mdtile_blend_wrap_regions with 0 regions and a zero region map: what the two-map sum and the division cost
    (c) rest / shift   + 4 regions, 2 background + 2 foreground, each a quarter of the canvas, two of them across a seam: 4 mdtile_gather_rect_wrap
                       and the region tail
    plain + regions    beside (c): mdtile_gather_all + 4 mdtile_gather_rect + mdtile_blend on the PLAIN plan of the same size, the same regions clipped
(b) is checked first against (a), bitwise.  Jobs without regions never take (b): it is here to price the kernel, not to replace a call.
    python probes/wrap_regions_ab.py            (on the GPU box; the shipping library)"""
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


def quarter_regions(W, H, wrap_y):
    """(x, y, w, h, mode): 2 BG + 2 FG, each W/2 x H/2; the first and the third cross the x seam, the third the y seam too where y wraps."""
    w, h = W // 2, H // 2
    return [(3 * W // 4, H // 8, w, h, E.REGION_BG), (W // 8, H // 4, w, h, E.REGION_BG),
            (7 * W // 8, 5 * H // 8 if wrap_y else 3 * H // 8, w, h, E.REGION_FG), (W // 4, H // 2, w, h, E.REGION_FG)]


class Evaluation:
    """One evaluation on fixed buffers, its C arguments built once.  kind: "old" (mdtile_blend / mdtile_blend_shift), "new" (mdtile_blend_wrap_regions,
    with `regions`), "plain" (mdtile_blend on a plain plan with `regions`, already clipped)."""

    def __init__(self, kind, plan, method, x, tiles, out, maps, shift, regions, wrap):
        L_ = E.lib()
        dt, st, h, nb, xp = E.dtype_code(x.dtype), E._stream(), plan.handle, len(tiles), x.data_ptr()
        old_maps = maps["old"] if kind != "new" else dict(tile_w=maps["old"].get("tile_w"))
        _, self.a, self.ptrs = E._blend_operands(plan, method, tiles, N, C, x.dtype, x.dtype, x.device, out, old_maps.get("weights"), old_maps.get("tile_w"),
                                                 old_maps.get("rescale"))
        a, ptrs = ctypes.byref(self.a), self.ptrs
        sx, sy = shift
        self.routs = [torch.empty(N, C, r[3], r[2], dtype=x.dtype, device=dev) for r in regions]
        self.rw = [torch.rand(r[3], r[2], device=dev) for r in regions]
        self.rarr = (E._Region * max(1, len(regions)))(*[E._Region(r[0], r[1], r[2], r[3], r[4], 0, o.data_ptr(), w.data_ptr())
                                                         for r, o, w in zip(regions, self.routs, self.rw)])
        self.keep = (plan, x, tiles, out, maps)
        steps = []
        if (sx, sy) == (0, 0):
            steps.append(lambda: L_.mdtile_gather_all(h, dt, N, C, xp, ptrs, nb, st))
        else:
            steps.append(lambda: L_.mdtile_gather_all_shift(h, dt, N, C, xp, ptrs, nb, sx, sy, st))
        for r, o in zip(regions, self.routs):
            if kind == "new":
                steps.append(lambda r=r, o=o: L_.mdtile_gather_rect_wrap(dt, N, C, plan.w, plan.h, xp, r[0], r[1], r[2], r[3], wrap[0], wrap[1], o.data_ptr(), st))
            else:
                steps.append(lambda r=r, o=o: L_.mdtile_gather_rect(dt, N, C, plan.w, plan.h, xp, r[0], r[1], r[2], r[3], o.data_ptr(), st))
        if kind == "new":
            self.wr = E._WrapRegions(self.rarr, len(regions), maps["grid_w"].data_ptr(), maps["region_w"].data_ptr(), sx, sy)
            wr = ctypes.byref(self.wr)
            steps.append(lambda: L_.mdtile_blend_wrap_regions(h, a, ptrs, nb, wr, st))
        elif (sx, sy) == (0, 0):
            rarr, nr = self.rarr, len(regions)
            steps.append(lambda: L_.mdtile_blend(h, a, ptrs, nb, rarr, nr, st))
        else:
            steps.append(lambda: L_.mdtile_blend_shift(h, a, ptrs, nb, sx, sy, st))
        self.steps = steps
        for s_ in steps:
            assert s_() == 0, L_.mdtile_last_error()

    def __call__(self):
        for s_ in self.steps:
            s_()


def run(W, H, wrap_y, tile, ov, dtype):
    plan = E.Plan(W, H, tile, tile, ov, BS, wrap_x=True, wrap_y=wrap_y)
    plain = E.Plan(W, H, tile, tile, ov, BS)
    wrap = (1, int(wrap_y))
    es = 4 if dtype == torch.float32 else 2
    shift = (5, 3 if wrap_y else 0)
    regions = quarter_regions(W, H, wrap_y)
    clipped = [(x, y, min(w, W - x), min(h, H - y), m) for (x, y, w, h, m) in regions]
    tile_w = E.gaussian_weights(plan.tile_w, plan.tile_h, dev)

    def plan_maps(p):
        weights, gsum = torch.zeros(H, W, device=dev), torch.zeros(H, W, device=dev)
        E.weight_map_add_grid(p, None, weights)
        E.weight_map_add_grid(p, tile_w, gsum)
        return weights, gsum

    canvas = es * N * C * H * W
    moved = 2 * plan.num_tiles * es * N * C * plan.tile_h * plan.tile_w + 2 * canvas
    sets = max(3, int(700e6 // moved) + 1)
    print(f"\nlatent {W} x {H} {'torus' if wrap_y else 'wrap-x'}, tile {plan.tile_w} / overlap {plan.overlap}, {str(dtype).split('.')[-1]}: {plan.num_tiles} tiles in "
          f"{plan.num_batches} batches (plain plan: {plain.num_tiles}); N = {N}, C = {C}; {moved / 1e6:.0f} MB per gather + blend pair, {sets} buffer sets", flush=True)
    xs = [torch.randn(N, C, H, W, device=dev).to(dtype) for _ in range(sets)]
    outs = [torch.empty(N, C, H, W, dtype=dtype, device=dev) for _ in range(sets)]

    def tile_bufs(p):
        return [[torch.empty(len(b) * N, C, p.tile_h, p.tile_w, dtype=dtype, device=dev) for b in p.batches] for _ in range(sets)]

    bufs, plain_bufs = tile_bufs(plan), tile_bufs(plain)
    for method, name in ((E.METHOD_MD, "md "), (E.METHOD_MOD, "mod")):
        md = method == E.METHOD_MD
        maps = {}
        for key, p in (("wrap", plan), ("plain", plain)):
            weights, gsum = plan_maps(p)
            zero = torch.zeros(H, W, device=dev)
            with_regions = zero.clone()
            for (x, y, w, h, m) in regions:
                if m == E.REGION_BG:
                    E.weight_map_add_rect_wrap(with_regions, x, y, w, h, None if md else E.gaussian_weights(w, h, dev), 1.0, wrap_x=True, wrap_y=wrap_y)
            old = dict(weights=weights) if md else dict(tile_w=tile_w, rescale=E.reciprocal(gsum))
            maps[key] = dict(old=old, grid_w=weights if md else gsum, zero=zero, with_regions=with_regions)

        def evals(kind, shift_, regs, key="wrap", region_w="zero"):
            p, b = (plan, bufs) if key == "wrap" else (plain, plain_bufs)
            m = dict(maps[key], region_w=maps[key][region_w])
            return [Evaluation(kind, p, method, xs[i], b[i], outs[i], m, shift_, regs, wrap) for i in range(sets)]

        # correctness first: (b) == (a), bitwise, at rest and shifted
        for s_ in ((0, 0), shift):
            evals("old", s_, [])[0]()
            want = outs[0].clone()
            outs[0].fill_(float("nan"))
            evals("new", s_, [])[0]()
            bits = torch.int32 if dtype == torch.float32 else torch.int16
            print(f"  {name} shift {s_}: blend_wrap_regions(0 regions) == the blend of before: {torch.equal(outs[0].view(bits), want.view(bits))}", flush=True)

        arms = {
            "(a) rest : gather_all + blend": evals("old", (0, 0), []),
            "(a) shift: gather_all_shift + blend_shift": evals("old", shift, []),
            "(b) rest : gather_all + blend_wrap_regions, 0 regions": evals("new", (0, 0), []),
            "(b) shift: gather_all_shift + blend_wrap_regions, 0 regions": evals("new", shift, []),
            "(c) rest : + 4 gather_rect_wrap, 4 regions": evals("new", (0, 0), regions, region_w="with_regions"),
            "(c) shift: + 4 gather_rect_wrap, 4 regions": evals("new", shift, regions, region_w="with_regions"),
            "plain plan: gather_all + 4 gather_rect + blend, 4 clipped regions": evals("plain", (0, 0), clipped, key="plain"),
        }
        res = timed_alternating(arms)
        base = {"rest": res["(a) rest : gather_all + blend"][0], "shift": res["(a) shift: gather_all_shift + blend_shift"][0]}
        for arm, (med, best) in res.items():
            ref = base["shift" if "shift" in arm.split(":")[0] else "rest"]
            print(f"  {name} {arm:68s} {med:8.2f} us (best {best:7.2f})  x{med / ref:5.3f} of (a)", flush=True)


def main():
    for (W, H, wrap_y) in ((1024, 1024, True), (1024, 512, False)):
        for (tile, ov) in ((128, 8), (96, 48)):
            for dtype in (torch.float32, torch.float16):
                run(W, H, wrap_y, tile, ov, dtype)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
