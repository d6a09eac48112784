"""A/B of the cross-faded tile assembly (csrc/vae_assemble.hip: k_vae_seam_blend), the protocol of probes/wrap_ab.py: one
process, COLD (rotating buffer sets larger than the 256 MiB Infinity Cache), 20 back-to-back launches per HIP-event pair, median of 7
rounds -- on the 16 tiles of the 8K decode (latent 1024^2, tile 256, N = 1, C = 3), b = 16 and b = 88:
    blend      mdtile_vae_assemble_blend
    plain      mdtile_vae_assemble on the same table
    copy       mdtile_stream_copy of the result's bytes: the floor of one launch that writes the image
and the whole 8K fast decode (SD-topology decoder, default-init weights) with VAEHook.seam_blend = 16 against the option off, alternating
calls in the same process, 3 per arm: what the smaller narrowing and the kept tiles cost.  The blend's result is checked first against a
torch restatement on the device (bitwise).
    python probes/seam_blend_ab.py            (on the GPU box; the shipping library)"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd"))
import mdtile as E          # noqa: E402

dev = torch.device("cuda:0")
N, C, L, TS = 1, 3, 1024, 256


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
    print(f"  {name:44s} {med:8.2f} us (best {best:7.2f})  {nbytes / med * 1e-3:7.0f} GB/s", flush=True)


def restatement(tiles, rows, cols, band, RH, RW):
    """include/mdtile.h's definition with torch ops on the device: per tile in ascending index, acc += w * v over its out box grown by b."""
    out = torch.empty(N, C, RH, RW, device=dev)
    acc = torch.zeros(N, C, RH, RW, device=dev)
    inband = torch.zeros(RH, RW, dtype=torch.bool, device=dev)
    xs = [tiles[c][2][0] for c in range(cols)] + [RW]
    ys = [tiles[r * cols][2][2] for r in range(rows)] + [RH]
    ar = torch.arange(max(RH, RW), device=dev)

    def axis(edges, k, n, size):        # (integer weight, in a band) of tile k along one axis for every coordinate
        w, band_here = torch.zeros(size, dtype=torch.int64, device=dev), torch.zeros(size, dtype=torch.bool, device=dev)
        a = ar[:size]
        w[edges[k] + (band if k > 0 else 0):edges[k + 1] - (band if k < n - 1 else 0)] = 1
        if k > 0:
            m = (a >= edges[k] - band) & (a < edges[k] + band)
            w[m], band_here[m] = (2 * (a - edges[k] + band) + 1)[m], True
        if k < n - 1:
            m = (a >= edges[k + 1] - band) & (a < edges[k + 1] + band)
            w[m], band_here[m] = (4 * band - (2 * (a - edges[k + 1] + band) + 1))[m], True
        return w, band_here
    for i, (t, ib, ob) in enumerate(tiles):
        r, c = divmod(i, cols)
        wy, by = axis(ys, r, rows, RH)
        wx, bx = axis(xs, c, cols, RW)
        ty, tx = ib[2] * 8, ib[0] * 8
        th, tw = t.shape[2:]
        w = (wy[ty:ty + th, None] * wx[None, tx:tx + tw]).float()
        both = (by[ty:ty + th, None] | bx[None, tx:tx + tw]) & (w > 0)
        inband[ty:ty + th, tx:tx + tw] |= both
        acc[:, :, ty:ty + th, tx:tx + tw] = torch.where(both, acc[:, :, ty:ty + th, tx:tx + tw] + w * t, acc[:, :, ty:ty + th, tx:tx + tw])
        own = (w > 0) & ~both
        out[:, :, ty:ty + th, tx:tx + tw] = torch.where(own, t, out[:, :, ty:ty + th, tx:tx + tw])
    by_any = torch.zeros(RH, dtype=torch.bool, device=dev)
    bx_any = torch.zeros(RW, dtype=torch.bool, device=dev)
    for Y in ys[1:-1]:
        by_any[Y - band:Y + band] = True
    for X in xs[1:-1]:
        bx_any[X - band:X + band] = True
    D = torch.where(by_any, 4 * band, 1)[:, None] * torch.where(bx_any, 4 * band, 1)[None, :]
    return torch.where(inband, acc / D.float(), out)


def assembly():
    ins, outs = E.vae_split_tiles(L, L, TS, True)
    rows = cols = 4
    assert len(ins) == 16
    RH = RW = L * 8
    nbytes = 2 * 4 * N * C * RH * RW
    sets = max(3, int(700e6 // nbytes) + 1)
    print(f"8K decode assembly: {len(ins)} tiles of up to {max((i[1] - i[0]) * 8 for i in ins)} px, result {N}x{C}x{RH}x{RW} "
          f"({nbytes / 2e6:.0f} MB written), {sets} buffer sets")
    bufs = [([(torch.randn(N, C, (ib[3] - ib[2]) * 8, (ib[1] - ib[0]) * 8, device=dev), ib, ob) for ib, ob in zip(ins, outs)],
             torch.empty(N, C, RH, RW, device=dev)) for _ in range(sets)]
    for band in (16, 88):
        tiles, out = bufs[0]
        E.vae_assemble_blend(tiles, rows, cols, out, band, True)
        torch.cuda.synchronize()
        same = torch.equal(out.view(torch.int32), restatement(tiles, rows, cols, band, RH, RW).view(torch.int32))
        print(f"  b = {band}: blend == restatement on the device, bitwise: {same}")
        report(f"blend b = {band}", timed([(lambda t=t, o=o: E.vae_assemble_blend(t, rows, cols, o, band, True)) for t, o in bufs]), nbytes)
    report("plain (mdtile_vae_assemble)", timed([(lambda t=t, o=o: E.vae_assemble(t, o, True)) for t, o in bufs]), nbytes)
    half = nbytes // 2
    cps = [E.StreamCopyCall(torch.randn(half // 4, device=dev), torch.empty(half // 4, device=dev)) for _ in range(sets)]
    report(f"stream copy {half / 1e6:.0f} MB -> {half / 1e6:.0f} MB", timed(cps), nbytes)


def decode():
    from hostsim import stub_host as sh, ldm_decoder as ld
    sh.install("cuda:0")
    pl = sh.load_plugin()
    dec = ld.make_decoder(0).to(dev)
    dec.original_forward = dec.forward
    torch.manual_seed(0)
    z = torch.randn(1, 4, L, L, device=dev)
    hooks = {}
    for band in (0, 16):
        hooks[band] = pl.tilevae.VAEHook(dec, TS, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
        hooks[band].seam_blend = band
    with torch.no_grad():
        hooks[0](z)                                        # warm-up: packs the weights, fills the allocator
        times = {0: [], 16: []}
        for _ in range(3):
            for band in (0, 16):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hooks[band](z)
                torch.cuda.synchronize()
                times[band].append((time.perf_counter() - t0) * 1e3)
    for band in (0, 16):
        ts = sorted(times[band])
        print(f"  8K fast decode, seam_blend = {band:2d}: median {ts[1]:8.1f} ms  ({', '.join(f'{t:.1f}' for t in times[band])})", flush=True)
    print(f"  max VRAM allocated {torch.cuda.max_memory_allocated(dev) / 2**30:.2f} GiB")


if __name__ == "__main__":
    assembly()
    torch.cuda.empty_cache()
    if "--no-decode" not in sys.argv:
        decode()
