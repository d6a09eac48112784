"""The colour fix (csrc/colorfix.hip) measured: prints one table and one JSON line.

    python probes/colorfix_ab.py [--reps 20] [--size 8192] [--e2e-size 2048]                      (on the GPU box)
    rocprofv3 --kernel-trace --stats -d DIR -- python probes/colorfix_ab.py --reps 5               the per-kernel split

  engine calls   mdtile.colorfix_wavelet, hist_u8 and lut_u8 on a size^2 RGB image: device events around ONE call, the median of --reps calls
                 after 3 warm-up calls, each beside mdtile_stream_copy moving the bytes the algorithm itself reads + writes (wavelet: 2 images read
                 + 1 written; histogram: 1 read; table: 1 read + 1 written).  The copy is the yardstick; "of copy" = copy time / call time.
  end to end     tile_utils.utils.color_fix_image at e2e-size^2 RGB with and without the kept device tensor, its parts (upload, kernels, download,
                 fromarray) apart, beside the numpy integer restatement (tests/colorfix_ref.py) on the host cores -- the only host implementation
                 there is.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from hostsim import stub_host as sh  # noqa: E402

sh.install("cuda:0")
sh.set_device("cuda:0")
pl = sh.load_plugin()
E, U = pl.engine, pl.utils
import colorfix_ref as cr  # noqa: E402
from PIL import Image  # noqa: E402

Image.MAX_IMAGE_PIXELS = None
DEV = torch.device("cuda:0")


def event_ms(fn, reps, warmup=3):
    """Device time of single calls of fn: events around each, [median, min, max] of `reps` after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def copy_ms(moved_bytes, reps):
    """mdtile_stream_copy reading + writing moved_bytes in all."""
    half = moved_bytes // 2 // 16 * 16
    a = torch.empty(half, dtype=torch.uint8, device=DEV)
    b = torch.empty_like(a)
    call = E.StreamCopyCall(a, b)
    out = event_ms(call, reps)
    out["bytes"] = 2 * half
    return out


def wall_ms(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def engine_calls(n, reps):
    g = torch.Generator(device=DEV).manual_seed(1)
    content = torch.randint(0, 256, (n, n, 3), dtype=torch.uint8, device=DEV, generator=g)
    style = torch.randint(0, 256, (n, n, 3), dtype=torch.uint8, device=DEV, generator=g)
    flat = torch.full((n, n, 3), 128, dtype=torch.uint8, device=DEV)
    lut = torch.randint(0, 256, (3, 256), dtype=torch.uint8, device=DEV, generator=g)
    image = n * n * 3
    rows = {}
    for name, fn, moved in (("wavelet", lambda: E.colorfix_wavelet(content, style), 3 * image),
                            ("hist_u8", lambda: E.hist_u8(content), image),
                            ("hist_u8 (flat image)", lambda: E.hist_u8(flat), image),
                            ("lut_u8", lambda: E.lut_u8(content, lut), 2 * image)):
        call, copy = event_ms(fn, reps), copy_ms(moved, reps)
        rows[name] = {"call": call, "algorithm_bytes": moved, "stream_copy": copy,
                      "of_copy_rate": round(copy["median_ms"] / call["median_ms"] * moved / copy["bytes"], 4),
                      "algorithm_TBps": round(moved / call["median_ms"] / 1e9, 3)}
    rows["wavelet"]["moved_with_int32_intermediate_bytes"] = 3 * image + 8 * image + 2 * image      # + mid written and read, + content / style read again
    return rows


def end_to_end(n, reps):
    rng = np.random.default_rng(2)
    result = Image.fromarray(rng.integers(0, 256, size=(n, n, 3), dtype=np.uint8))
    init = Image.fromarray(rng.integers(0, 256, size=(n, n, 3), dtype=np.uint8))
    kept = (init, U.image_to_device(init))
    t0 = time.perf_counter()
    want = cr.wavelet_int(np.asarray(result), np.asarray(init))
    host_ms = (time.perf_counter() - t0) * 1e3
    out = {"size": n, "numpy_restatement_ms": round(host_ms, 1)}
    for mode in ("wavelet", "adain"):
        got = U.color_fix_image(result, init, mode, kept)                  # warm-up: pinned buffer, kernels
        if mode == "wavelet":
            out["bytes_differ_from_restatement"] = int((np.asarray(got) != want).sum())
        with_kept, without = [], []
        for _ in range(reps):
            with_kept.append(wall_ms(lambda: U.color_fix_image(result, init, mode, kept))[0])
            without.append(wall_ms(lambda: U.color_fix_image(result, init, mode))[0])
        parts = {"upload": [], "kernels": [], "download": [], "fromarray": []}
        fix = E.colorfix_wavelet if mode == "wavelet" else E.colorfix_adain
        for _ in range(reps):
            ms, t = wall_ms(lambda: U.image_to_device(result))
            parts["upload"].append(ms)
            ms, o = wall_ms(lambda: fix(t, kept[1]))
            parts["kernels"].append(ms)
            host = torch.empty(o.shape, dtype=torch.uint8, pin_memory=True)
            ms, _ = wall_ms(lambda: host.copy_(o, non_blocking=True))
            parts["download"].append(ms)
            ms, _ = wall_ms(lambda: Image.fromarray(host.numpy()))
            parts["fromarray"].append(ms)
        out[mode] = {"with_kept_ms": round(statistics.median(with_kept), 3), "without_kept_ms": round(statistics.median(without), 3),
                     "parts_median_ms": {k: round(statistics.median(v), 3) for k, v in parts.items()}}
    out["speedup_over_numpy_with_kept"] = round(host_ms / out["wavelet"]["with_kept_ms"], 1)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=8192)
    ap.add_argument("--e2e-size", type=int, default=2048)
    a = ap.parse_args()
    result = {"probe": "colorfix_ab", "reps": a.reps, "size": a.size, "engine": engine_calls(a.size, a.reps),
              "end_to_end": end_to_end(a.e2e_size, min(a.reps, 5))}
    print(f"{'call at %d^2 RGB' % a.size:<24} {'median ms':>10} {'min':>8} {'max':>8} {'copy ms':>9} {'of copy':>8} {'TB/s':>7}")
    for name, r in result["engine"].items():
        print(f"{name:<24} {r['call']['median_ms']:>10.4f} {r['call']['min_ms']:>8.4f} {r['call']['max_ms']:>8.4f} {r['stream_copy']['median_ms']:>9.4f} "
              f"{r['of_copy_rate']:>8.3f} {r['algorithm_TBps']:>7.3f}")
    e = result["end_to_end"]
    print(f"color_fix_image at {e['size']}^2 RGB: numpy restatement {e['numpy_restatement_ms']} ms; " +
          "; ".join(f"{m}: {e[m]['with_kept_ms']} ms with / {e[m]['without_kept_ms']} ms without the kept tensor, parts {e[m]['parts_median_ms']}"
                    for m in ("wavelet", "adain")))
    print(json.dumps(result))
