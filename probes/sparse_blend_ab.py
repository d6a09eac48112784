"""A/B of tile skipping (csrc/wrap.hip: k_wrap_gather with the active table, k_walk_blend<..., SPARSE>), the protocol of probes/wrap_ab.py and
probes/seam_blend_ab.py: one process, COLD (rotating buffer sets larger than the 256 MiB Infinity Cache), 20 back-to-back calls per HIP-event
pair, median of 7 rounds -- at latent 1024^2, tile 128 / overlap 8 (81 tiles), fp32, N = 2, C = 4, MultiDiffusion and Mixture of Diffusers:
    sparse ~1/10   gather_all on the sparse plan + mdtile_blend_sparse for a mask that touches about a tenth of the tiles
    sparse all     the same with every tile active (the price of the slot hop and the liveness pass alone)
    plain          mdtile_gather_all + mdtile_blend on the full plan
    copy           mdtile_stream_copy of each pair's bytes: the floor.  Plain: canvas read + tiles written + tiles read + canvas written.  Sparse:
                   the active tiles' rectangles read (at most the canvas), their tiles written and read, `fill` read at the pixels that are
                   not live, the canvas written
mdtile_tile_activity (once per job) is timed beside them.  The sparse result is checked first against where(live, blend(parent), fill), bitwise.
    python probes/sparse_blend_ab.py            (on the GPU box; the shipping library)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd"))
import mdtile as E          # noqa: E402

dev = torch.device("cuda:0")
N, C, L, TILE, OV, BS = 2, 4, 1024, 128, 8, 8


def timed(calls, n=20, rounds=7):
    for c in calls[:3]:
        c()
    ts = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(n):
            calls[i % len(calls)]()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / n * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0]


def report(name, us, nbytes):
    med, best = us
    print(f"  {name:52s} {med:8.2f} us (best {best:7.2f})  {nbytes / med * 1e-3:7.0f} GB/s", flush=True)


def main():
    plan = E.Plan(L, L, TILE, TILE, OV, BS)
    T = plan.num_tiles
    weights = torch.zeros(L, L, device=dev)
    E.weight_map_add_grid(plan, None, weights)
    tile_w = E.gaussian_weights(plan.tile_w, plan.tile_h, dev)
    gsum = torch.zeros(L, L, device=dev)
    E.weight_map_add_grid(plan, tile_w, gsum)
    rescale = E.reciprocal(gsum)
    maps = {E.METHOD_MD: dict(weights=weights), E.METHOD_MOD: dict(tile_w=tile_w, rescale=rescale)}

    # a face-sized repaint: a 210 x 200 latent-px rectangle off the grid lines
    mask = torch.zeros(4, L, L, device=dev)
    mask[:, 350:550, 230:440] = 1.0
    active = E.tile_activity(plan, mask)
    tenth = plan.subset(active, BS)
    every = plan.subset([1] * T, BS)
    print(f"latent {L}^2, tile {plan.tile_w} / overlap {plan.overlap}: {T} tiles; the mask touches {tenth.num_tiles} ({tenth.num_batches} batches of "
          f"{tenth.tile_bs}); N = {N}, C = {C}, fp32")

    canvas = 4 * N * C * L * L
    tile_bytes = 4 * N * C * plan.tile_h * plan.tile_w
    sets = max(3, int(700e6 // (2 * canvas + T * tile_bytes)) + 1)
    xs = [torch.randn(N, C, L, L, device=dev) for _ in range(sets)]
    outs = [torch.empty(N, C, L, L, device=dev) for _ in range(sets)]

    def buffers(p):
        return [[torch.empty(len(b) * N, C, p.tile_h, p.tile_w, device=dev) for b in p.batches] for _ in range(sets)]

    def live_map(flags):
        live = torch.ones(L, L, dtype=torch.bool, device=dev)
        for a, (x, y, w, h) in zip(flags, plan.bboxes):
            if not a:
                live[y:y + h, x:x + w] = False
        return live

    def sparse_bytes(p, flags):
        """What the sparse pair moves: the gather reads the active tiles' rectangles only, the blend reads `fill` where no tile decides."""
        dead = 1.0 - float(live_map(flags).sum()) / (L * L)
        return int(min(canvas, p.num_tiles * tile_bytes) + 2 * p.num_tiles * tile_bytes + dead * canvas + canvas)

    # correctness first: the sparse blend against where(live, blend(parent), fill) on the device
    live = live_map(active)
    full_tiles = E.gather_all(plan, xs[0])
    sub_tiles = E.gather_all(tenth, xs[0])
    for method, name in ((E.METHOD_MD, "MultiDiffusion"), (E.METHOD_MOD, "Mixture of Diffusers")):
        want = torch.where(live, E.blend(plan, method, full_tiles, N, C, **maps[method]), xs[1])
        got = E.blend_sparse(tenth, method, sub_tiles, N, C, fill=xs[1], **maps[method])
        print(f"  {name}: blend_sparse == where(live, blend(parent), fill), bitwise: {torch.equal(got.view(torch.int32), want.view(torch.int32))}"
              f"  ({int(live.sum())} of {L * L} pixels live)")

    act_masks = [mask.clone() for _ in range(sets)]
    report("mdtile_tile_activity (4 planes, once per job)", timed([(lambda m=m: E.tile_activity(plan, m)) for m in act_masks]), 4 * 4 * L * L)

    for method, name in ((E.METHOD_MD, "md "), (E.METHOD_MOD, "mod")):
        for label, p, flags in ((f"sparse {tenth.num_tiles}/{T}", tenth, active), (f"sparse {T}/{T}", every, [1] * T)):
            bufs = buffers(p)
            moved = sparse_bytes(p, flags)

            def call(i, p=p, bufs=bufs):
                E.gather_all(p, xs[i], out=bufs[i])
                E.blend_sparse(p, method, bufs[i], N, C, fill=xs[i], out=outs[i], **maps[method])
            report(f"{name} {label}: gather_all + blend_sparse", timed([(lambda i=i: call(i)) for i in range(sets)]), moved)
            del bufs
        bufs = buffers(plan)
        calls = [E.BlendCall(plan, method, bufs[i], N, C, out=outs[i], **maps[method]) for i in range(sets)]

        def plain(i, bufs=bufs, calls=calls):
            E.gather_all(plan, xs[i], out=bufs[i])
            calls[i]()
        moved = 2 * T * tile_bytes + 2 * canvas
        report(f"{name} plain: gather_all + mdtile_blend", timed([(lambda i=i: plain(i)) for i in range(sets)]), moved)
        del bufs, calls
    half = (2 * T * tile_bytes + 2 * canvas) // 2 // 16 * 16
    cps = [E.StreamCopyCall(torch.randn(half // 4, device=dev), torch.empty(half // 4, device=dev)) for _ in range(sets)]
    report(f"stream copy {half / 1e6:.0f} MB -> {half / 1e6:.0f} MB (the plain arm's bytes)", timed(cps), 2 * half)
    half = sparse_bytes(tenth, active) // 2 // 16 * 16
    cps = [E.StreamCopyCall(torch.randn(half // 4, device=dev), torch.empty(half // 4, device=dev)) for _ in range(sets)]
    report(f"stream copy {half / 1e6:.0f} MB -> {half / 1e6:.0f} MB (the sparse {tenth.num_tiles}/{T} arm's bytes)", timed(cps), 2 * half)


if __name__ == "__main__":
    main()
