"""Times Noise Inversion's renoise mask on the GPU (csrc/retouch.hip): mdtile_retouch_mask and mdtile_renoise_resize on an 8192^2 image, grey
and RGB, k in {2, 64, 512}; AbstractDiffusion.renoise_mask() end to end (PIL image in host memory -> mask on the latent grid, upload
included); and, once, the numpy restatement of the definition (tests/retouch_ref.py) on the host cores.

    python tools/renoise_ab.py [--size 8192] [--reps 20] [--no-host] [--out FILE.json]

The parent of this path was OpenCV on the CPU and cannot run where OpenCV is absent, so nothing here is an A/B against it: the numpy time
is a STAND-IN for a host-side filter (same passes over the same image, numpy instead of OpenCV), not a baseline.

Timing: device events around ONE call, median of --reps calls after 3 warm-up calls, on the same buffers.  The working set of a call at
8192^2 (image 67 / 201 MB, row sums 537 MB, mask 268 MB) is several times the 256 MB Infinity Cache, so repeated calls are cold in the sense
that matters.  Bytes are the algorithm's own (computed from the shapes below), fractions are of 8.0 TB/s."""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

HBM_PEAK = 8.0e12


def mask_bytes(H, W, ch):
    """k_retouch_rows: image in, 8 B of row sums out; k_retouch_cols: the row sums in (every further read of a row is a cache hit by design:
    a chunk re-reads rows it or its neighbour loaded k rows earlier), 4 B of mask out."""
    return {"rows": H * W * (ch + 8), "cols": H * W * (8 + 4)}


def resize_bytes(H, W, h, w):
    return 4 * H * W * min(1.0, 4.0 * h * w / (H * W)) + 4 * h * w      # four taps per output pixel; never more than the mask itself


def event_time(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(ts), min(ts), max(ts)


def device_image(S, rgb, dev):
    """Smooth gradient + fine texture on a third of the 16-px cells + flat quarters, generated on the GPU (the timing does not depend on it)."""
    g = torch.Generator(device=dev).manual_seed(5)
    yy = torch.arange(S, device=dev, dtype=torch.float32)[:, None]
    xx = torch.arange(S, device=dev, dtype=torch.float32)[None, :]
    chans = []
    for c in range(3 if rgb else 1):
        v = 127.5 + 90.0 * torch.sin(xx / (17.0 + 5 * c)) * torch.cos(yy / (23.0 - 3 * c)) + 0.01 * (xx - yy)
        tex = torch.randint(-40, 41, (S, S), generator=g, device=dev).float() * ((((xx // 16) + (yy // 16)) % 3) == 0)
        chans.append((v + tex).round().clamp(0, 255).to(torch.uint8))
    img = torch.stack(chans, dim=-1)
    q = S // 4
    img[:q, :q] = 93
    img[:q, S - q:] = 0
    img[S - q:, :q] = 255
    return img.contiguous() if rgb else img[..., 0].contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the numpy restatement on the host cores (about a minute and ~10 GB at 8192^2)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("renoise_ab.py measures on the GPU: no device found (nothing is timed on the CPU)")
    import __graft_entry__ as ge
    ge.build()
    from hostsim import stub_host as sh
    sh.install("cuda:0")
    sh.set_device("cuda:0")
    pl = sh.load_plugin()
    E, dev = pl.engine, torch.device("cuda:0")
    S, lat = a.size, a.size // 8
    res = {"size": S, "reps": a.reps, "device": torch.cuda.get_device_name(0), "hbm_peak_Bps": HBM_PEAK, "mask": [], "resize": [], "end_to_end": []}
    imgs = {rgb: device_image(S, rgb, dev) for rgb in (False, True)}
    print(f"| call | input | k | median ms (min-max) | bytes (rows + cols) | TB/s | of 8 TB/s |\n|---|---|---:|---:|---:|---:|---:|")
    masks = {}
    for rgb in (False, True):
        for k in (2, 64, 512):
            t, lo, hi = event_time(lambda: E.retouch_mask(imgs[rgb], k), a.reps)
            b = mask_bytes(S, S, 3 if rgb else 1)
            tot = b["rows"] + b["cols"]
            res["mask"].append({"rgb": rgb, "k": k, "s": t, "min_s": lo, "max_s": hi, "bytes": b})
            print(f"| mdtile_retouch_mask (2 kernels) | {'RGB' if rgb else 'grey'} {S}^2 | {k} | {t * 1e3:.3f} ({lo * 1e3:.3f}-{hi * 1e3:.3f}) | "
                  f"{b['rows'] / 1e6:.0f} + {b['cols'] / 1e6:.0f} MB | {tot / t / 1e12:.2f} | {tot / t / HBM_PEAK:.2f} |")
            if rgb:
                masks[k] = E.retouch_mask(imgs[rgb], k)
    for k in (64,):
        for s in (1.0,):
            t, lo, hi = event_time(lambda: E.renoise_resize(masks[k], (lat, lat), s), a.reps)
            b = resize_bytes(S, S, lat, lat)
            res["resize"].append({"k": k, "strength": s, "s": t, "min_s": lo, "max_s": hi, "bytes": b})
            print(f"| mdtile_renoise_resize | mask {S}^2 -> {lat}^2 | - | {t * 1e3:.3f} ({lo * 1e3:.3f}-{hi * 1e3:.3f}) | {b / 1e6:.0f} MB | "
                  f"{b / t / 1e12:.2f} | {b / t / HBM_PEAK:.2f} |")
    # end to end: the product's renoise_mask() on a PIL image in host memory (pageable), upload included, host clock around a synchronise
    from PIL import Image
    for rgb in (True, False):
        pil = Image.fromarray(imgs[rgb].cpu().numpy())
        p = SimpleNamespace(init_images=[pil])
        for k in (2, 64, 512):
            me = SimpleNamespace(noise_inverse_renoise_strength=1.0, noise_inverse_renoise_kernel=k)
            ts = []
            for i in range(4):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                m = pl.abstractdiffusion.AbstractDiffusion.renoise_mask(me, p, (lat, lat))
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            res["end_to_end"].append({"rgb": rgb, "k": k, "first_s": ts[0], "median_of_next3_s": statistics.median(ts[1:])})
            print(f"| renoise_mask() end to end, upload included | PIL {'RGB' if rgb else 'L'} {S}^2 | {k} | {statistics.median(ts[1:]) * 1e3:.1f} "
                  f"(first call {ts[0] * 1e3:.1f}) | upload {S * S * (3 if rgb else 1) / 1e6:.0f} MB | - | - |")
            assert tuple(m.shape) == (lat, lat)
    if not a.no_host:
        import retouch_ref as rr
        k = 64
        host = imgs[True].cpu().numpy()
        t0 = time.perf_counter()
        want = rr.retouch_mask(host, k)
        t = time.perf_counter() - t0
        same = bool(np.array_equal(want, masks[k].cpu().numpy()))
        res["host_numpy"] = {"rgb": True, "k": k, "s": t, "threads": os.environ.get("OMP_NUM_THREADS"), "gpu_mask_bitwise_equal": same}
        print(f"| numpy restatement on the host cores, once (a stand-in for the OpenCV path, NOT a baseline) | RGB {S}^2 | {k} | {t * 1e3:.0f} | - | - | - |")
        print(f"GPU mask at {S}^2, k = {k}, RGB == numpy restatement bit for bit: {same}")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
