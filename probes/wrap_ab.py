"""A/B of the wrap-x and torus blends (csrc/wrap.hip), one process, COLD (rotating buffer sets larger than the 256 MiB Infinity Cache),
20 back-to-back launches per HIP-event pair, median of 7 rounds -- the method of DESIGN.md 3.4 / probes/blend_r6_ab.py -- at latent 1024^2,
tile 128 / overlap 8 and tile 96 / overlap 48, N = 2, C = 4, fp32, MultiDiffusion:
    torus      mdtile_blend on the plan closed in both axes (mdtile_plan_create_wrap(1, 1): k_walk_blend, cyclic rows and columns)
    wrap-x     mdtile_blend on the wrap-x plan (mdtile_plan_create_wrap(1, 0): the same k_walk_blend on plain rows)
    plain      mdtile_blend on the plain plan of the same canvas (what it dispatches: k_blend / k_blend_lds), batches handed over the same way
    copy       mdtile_stream_copy of the wrap-x launch's bytes: the floor of one launch of that size
The torus and wrap-x results are checked first against a torch restatement of the sequential `+=` loop on the device (bitwise).
    python probes/wrap_ab.py            (on the GPU box; the shipping library)"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd"))
import mdtile as E          # noqa: E402

dev = torch.device("cuda:0")
N, C = 2, 4


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
    print(f"  {name:38s} {med:7.2f} us (best {best:6.2f})  {nbytes / med * 1e-3:7.0f} GB/s", flush=True)


def setup(plan):
    weights = torch.zeros(1, 1, plan.h, plan.w, device=dev)
    E.weight_map_add_grid(plan, None, weights)
    nbytes = 4 * (plan.num_tiles * N * C * plan.tile_h * plan.tile_w + N * C * plan.h * plan.w) + 4 * plan.h * plan.w
    sets = max(8, int(700e6 // nbytes) + 1)
    rows = [len(b) * N for b in plan.batches]
    bufs = [(list(torch.randn(plan.num_tiles * N, C, plan.tile_h, plan.tile_w, device=dev).split(rows, dim=0)),
             torch.empty(N, C, plan.h, plan.w, device=dev)) for _ in range(sets)]
    calls = [E.BlendCall(plan, E.METHOD_MD, t, N, C, out=o, weights=weights) for t, o in bufs]
    return weights, nbytes, bufs, calls


def restatement(plan, tiles, weights):
    buf = torch.zeros(N, C, plan.h, plan.w, device=dev)
    flat = torch.cat(tiles, dim=0)
    for t, (x, y, w, h) in enumerate(plan.bboxes):
        cols = (x + torch.arange(w, device=dev)) % plan.w
        rows = ((y + torch.arange(h, device=dev)) % plan.h)[:, None]
        buf[:, :, rows, cols] += flat[t * N:(t + 1) * N]
    return torch.where(weights > 1, buf / weights, buf)


for (L, tile, ov) in ((1024, 128, 8), (1024, 96, 48)):
    wplan, pplan = E.Plan(L, L, tile, tile, ov, 4, wrap_x=True), E.Plan(L, L, tile, tile, ov, 4)
    tplan = E.Plan(L, L, tile, tile, ov, 4, wrap_x=True, wrap_y=True)
    print(f"{L}x{L} latent, tile {tile} overlap {ov}: torus {tplan.cols} x {tplan.rows} tiles, wrap-x {wplan.cols} x {wplan.rows}, "
          f"plain {pplan.cols} x {pplan.rows}")
    weights, tbytes, bufs, calls = setup(tplan)
    got = calls[0]()
    torch.cuda.synchronize()
    same = torch.equal(got.view(torch.int32), restatement(tplan, bufs[0][0], weights).view(torch.int32))
    print(f"  torus == sequential loop, bitwise: {same}")
    report(f"torus ({tbytes / 1e6:.1f} MB, {len(bufs)} sets)", timed(calls), tbytes)
    del bufs, calls
    torch.cuda.empty_cache()
    weights, nbytes, bufs, calls = setup(wplan)
    got = calls[0]()
    torch.cuda.synchronize()
    same = torch.equal(got.view(torch.int32), restatement(wplan, bufs[0][0], weights).view(torch.int32))
    print(f"  wrap-x == sequential loop, bitwise: {same}")
    report(f"wrap-x ({nbytes / 1e6:.1f} MB, {len(bufs)} sets)", timed(calls), nbytes)
    half = (nbytes // 2 + 4095) // 4096 * 4096
    cps = [E.StreamCopyCall(torch.randn(half // 4, device=dev), torch.empty(half // 4, device=dev)) for _ in range(len(bufs))]
    report(f"stream copy {half / 1e6:.1f} MB -> {half / 1e6:.1f} MB", timed(cps), 2 * half)
    del cps, bufs, calls
    torch.cuda.empty_cache()
    _, pbytes, pbufs, pcalls = setup(pplan)
    d = pcalls[0].dispatch()
    report(f"plain, {'k_blend_lds' if d.lds else 'k_blend'} ({pbytes / 1e6:.1f} MB, {len(pbufs)} sets)", timed(pcalls), pbytes)
    del pbufs, pcalls
    torch.cuda.empty_cache()
