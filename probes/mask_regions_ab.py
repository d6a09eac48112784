"""A/B of free-form mask regions (csrc/blend.hip: k_blend<..., MASKED>, csrc/mask_regions.hip) against the calls of before, the
protocol of probes/lattice_regions_ab.py: one process, COLD (rotating buffer sets larger than the 256 MiB Infinity Cache), 20 back-to-back calls per
HIP-event pair, median of 7 rounds, the arms ALTERNATING inside every round in an order rotated per round -- at latent 1024^2, tile 128 / overlap 8,
fp32 and fp16, N = 2, C = 4, MultiDiffusion and Mixture of Diffusers, four regions (2 BG + 2 FG), each a quarter of the canvas:
    (a) mdtile_blend with the four rectangles: the baseline; its kernels are the parent commit's (device code compared, identical)
    (b) mdtile_blend_mask_regions with the same rectangles and NULL covers: what the MASKED kernel costs beside it (checked bitwise against (a))
    (c) mdtile_blend_mask_regions with a disc in every rectangle
and, once per job and region:
    mdtile_mask_cover_u8 on an 8192^2 mask -> 1024^2 coverage, against mdtile_stream_copy of the 64 MiB it reads
    mdtile_mask_region on a quarter-canvas disc with a feather ratio of 0.2 (R = 51) and without a feather
    python probes/mask_regions_ab.py            (on the GPU box; the shipping library)"""
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
W = H = 1024


def timed_alternating(arms, n_calls=N_CALLS):
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
            for i in range(n_calls):
                calls[i % len(calls)]()
            e.record()
            torch.cuda.synchronize()
            ts[name].append(s.elapsed_time(e) / n_calls * 1e3)
    return {name: (sorted(t)[len(t) // 2], min(t)) for name, t in ts.items()}


def quarter_regions():
    w, h = W // 2, H // 2
    return [(W // 8, H // 8, w, h, E.REGION_BG), (3 * W // 8, H // 4, w, h, E.REGION_BG), (W // 2, H // 2, w, h, E.REGION_FG),
            (W // 4, 3 * H // 8, w, h, E.REGION_FG)]


def disc(w, h):
    i, j = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    return (((2 * i - h + 1) ** 2 * w * w + (2 * j - w + 1) ** 2 * h * h) <= w * w * h * h).to(torch.uint8).to(dev)


class Blend:
    """One blend on fixed buffers, its C arguments built once.  kind: "plain" (mdtile_blend) | "masked" (mdtile_blend_mask_regions, covers or NULL)."""

    def __init__(self, kind, plan, method, tiles, out, maps, regions, routs, rw, covers):
        L_ = E.lib()
        _, self.a, self.ptrs = E._blend_operands(plan, method, tiles, N, C, out.dtype, out.dtype, dev, out, maps.get("weights"), maps.get("tile_w"), maps.get("rescale"))
        rarr = [E._Region(r[0], r[1], r[2], r[3], r[4], 0, o.data_ptr(), w.data_ptr()) for r, o, w in zip(regions, routs, rw)]
        self.keep = (plan, tiles, out, maps, routs, rw, covers)
        a, ptrs, nb, st, h, nr = ctypes.byref(self.a), self.ptrs, len(tiles), E._stream(), plan.handle, len(regions)
        if kind == "plain":
            self.arr = (E._Region * nr)(*rarr)
            self.fn = lambda: L_.mdtile_blend(h, a, ptrs, nb, self.arr, nr, st)
        else:
            self.arr = (E._MaskRegion * nr)(*[E._MaskRegion(r, None if c is None else c.data_ptr()) for r, c in zip(rarr, covers)])
            self.fn = lambda: L_.mdtile_blend_mask_regions(h, a, ptrs, nb, self.arr, nr, st)
        assert self.fn() == 0, L_.mdtile_last_error()

    def __call__(self):
        self.fn()


def run_blend(dtype):
    plan = E.Plan(W, H, 128, 128, 8, BS)
    es = 4 if dtype == torch.float32 else 2
    regions = quarter_regions()
    moved = plan.num_tiles * es * N * C * plan.tile_h * plan.tile_w + es * N * C * H * W * 2
    sets = max(3, int(700e6 // moved) + 1)
    print(f"\nlatent {W} x {H}, tile {plan.tile_w} / overlap {plan.overlap}, {str(dtype).split('.')[-1]}: {plan.num_tiles} tiles in {plan.num_batches} batches; "
          f"N = {N}, C = {C}; 4 quarter-canvas regions; ~{moved / 1e6:.0f} MB per blend, {sets} buffer sets", flush=True)
    tiles = [[torch.randn(len(b) * N, C, plan.tile_h, plan.tile_w, device=dev).to(dtype) for b in plan.batches] for _ in range(sets)]
    outs = [torch.empty(N, C, H, W, dtype=dtype, device=dev) for _ in range(sets)]
    routs = [[torch.randn(N, C, r[3], r[2], device=dev).to(dtype) for r in regions] for _ in range(sets)]
    rw = [torch.rand(r[3], r[2], device=dev) for r in regions]
    discs = [disc(r[2], r[3]) for r in regions]
    tile_w = E.gaussian_weights(plan.tile_w, plan.tile_h, dev)
    for method, name in ((E.METHOD_MD, "md "), (E.METHOD_MOD, "mod")):
        md = method == E.METHOD_MD
        weights = torch.zeros(H, W, device=dev)
        E.weight_map_add_grid(plan, None if md else tile_w, weights)
        maps = dict(weights=weights) if md else dict(tile_w=tile_w, rescale=E.reciprocal(weights))

        def calls(kind, covers):
            return [Blend(kind, plan, method, tiles[i], outs[i], maps, regions, routs[i], rw, covers) for i in range(sets)]

        bits = torch.int32 if dtype == torch.float32 else torch.int16
        calls("plain", None)[0]()
        want = outs[0].clone()
        outs[0].fill_(float("nan"))
        calls("masked", [None] * 4)[0]()
        print(f"  {name} blend_mask_regions(NULL covers) == blend: {torch.equal(outs[0].view(bits), want.view(bits))}", flush=True)
        arms = {"(a) mdtile_blend, 4 rectangles": calls("plain", None),
                "(b) mdtile_blend_mask_regions, NULL covers": calls("masked", [None] * 4),
                "(c) mdtile_blend_mask_regions, 4 discs": calls("masked", discs)}
        res = timed_alternating(arms)
        ref = res["(a) mdtile_blend, 4 rectangles"][0]
        for arm, (med, best) in res.items():
            print(f"  {name} {arm:48s} {med:8.2f} us (best {best:7.2f})  x{med / ref:5.3f} of (a)", flush=True)


def run_masks():
    L_, st = E.lib(), E._stream()
    Wm = Hm = 8192
    sets = 12      # 12 x 64 MiB masks: every call reads a mask that has left the Infinity Cache
    i, j = torch.meshgrid(torch.arange(Hm, device=dev), torch.arange(Wm, device=dev), indexing="ij")
    base = ((((i - Hm // 2) ** 2 + (j - Wm // 2) ** 2) < (Wm // 3) ** 2).to(torch.uint8) * 255)
    masks = [base.clone() for _ in range(sets)]
    dsts = [torch.empty(Hm, Wm, dtype=torch.uint8, device=dev) for _ in range(2)]
    cover = torch.empty(H, W, dtype=torch.uint8, device=dev)
    box = torch.empty(5, dtype=torch.int32, device=dev)
    arms = {"mdtile_mask_cover_u8, 8192^2 -> 1024^2": [lambda m=m: L_.mdtile_mask_cover_u8(m.data_ptr(), Wm, Hm, W, H, cover.data_ptr(), box.data_ptr(), st) for m in masks],
            "mdtile_stream_copy of the 64 MiB it reads": [lambda m=m, k=k: L_.mdtile_stream_copy(m.data_ptr(), dsts[k % 2].data_ptr(), Wm * Hm, st) for k, m in enumerate(masks)]}
    print(f"\nmask {Wm} x {Hm} -> coverage {W} x {H}; {sets} masks in rotation", flush=True)
    for arm, (med, best) in timed_alternating(arms).items():
        print(f"  {arm:48s} {med:8.2f} us (best {best:7.2f})", flush=True)
    print(f"  box = {box.tolist()}", flush=True)
    x, y, x1, y1, _ = box.tolist()
    w, h = x1 - x, y1 - y
    rcover = torch.empty(h, w, dtype=torch.uint8, device=dev)
    feather = torch.empty(h, w, device=dev)
    q = disc(W // 2, H // 2)
    canvas = torch.zeros(H, W, dtype=torch.uint8, device=dev)
    canvas[H // 4:H // 4 + H // 2, W // 4:W // 4 + W // 2] = q
    rc2, f2 = torch.empty(H // 2, W // 2, dtype=torch.uint8, device=dev), torch.empty(H // 2, W // 2, device=dev)
    arms = {f"mdtile_mask_region, the {w} x {h} disc, ratio 0.2": [lambda: L_.mdtile_mask_region(cover.data_ptr(), W, H, x, y, w, h, 0.2, rcover.data_ptr(), feather.data_ptr(), st)],
            "mdtile_mask_region, quarter-canvas disc, ratio 0.2": [lambda: L_.mdtile_mask_region(canvas.data_ptr(), W, H, W // 4, H // 4, W // 2, H // 2, 0.2, rc2.data_ptr(), f2.data_ptr(), st)],
            "mdtile_mask_region, quarter-canvas disc, no feather": [lambda: L_.mdtile_mask_region(canvas.data_ptr(), W, H, W // 4, H // 4, W // 2, H // 2, 0.0, rc2.data_ptr(), None, st)]}
    for arm, (med, best) in timed_alternating(arms, n_calls=5).items():
        print(f"  {arm:52s} {med:9.2f} us (best {best:8.2f})  (warm: the coverage is 1 MiB)", flush=True)


def main():
    for dtype in (torch.float32, torch.float16):
        run_blend(dtype)
        torch.cuda.empty_cache()
    run_masks()


if __name__ == "__main__":
    main()
