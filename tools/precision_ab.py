#!/usr/bin/env python3
"""A/B of the matrix-core precision modes on the benchmark's decode: the seeded SD decoder of hostsim/ldm_decoder.py (bench.py's), a 1024 x 1024
latent (an 8K image), decoder tile 256, fast mode, one process, one GPU.  Per mode: one warm-up decode, then `--reps` decodes timed with CUDA
events (ms per decode, min and median), and the max-abs / rel-L2 error of the mode's image against the BF16X3 image.
    python tools/precision_ab.py [--modes bf16x3,bf16] [--latent 1024] [--tile 256] [--reps 2] [--out file.json]
For per-kernel times run one mode per process under a kernel trace, e.g.
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/precision_ab.py --modes bf16 --reps 1
(--modes bf16 alone skips the error column: it needs the BF16X3 image of the same process).  A mode may be listed twice
(--modes bf16x3,bf16,f16,bf16x3): the repeat is reported as "bf16x3#2", and the difference between the two BF16X3 rows is printed as the
run-to-run spread a speed-up has to exceed."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

MODES = {"bf16x3": 0, "f32": 1, "bf16": 2, "f16": 5}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="bf16x3,bf16")
    ap.add_argument("--latent", type=int, default=1024)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import __graft_entry__ as ge
    from hostsim import ldm_decoder as ld
    from hostsim import stub_host as sh
    assert torch.cuda.is_available(), "needs a GPU"
    ge.build()
    sh.install("cuda:0")
    sh.set_device("cuda:0")
    pl = sh.load_plugin()
    E = pl.engine
    dev = torch.device("cuda:0")
    dec = ld.make_decoder(0).to(dev)
    dec.original_forward = dec.forward
    hook = pl.tilevae.VAEHook(dec, a.tile, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
    z = torch.randn(1, 4, a.latent, a.latent, generator=torch.Generator(device="cpu").manual_seed(2)).to(dev)
    import builtins
    _print = builtins.print
    rows, images = [], {}
    for name in a.modes.split(","):
        mode = MODES[name]
        n_seen = sum(1 for r in rows if r["mode"].split("#")[0] == name)
        name = name if n_seen == 0 else f"{name}#{n_seen + 1}"
        with torch.no_grad(), E.precision(mode):
            builtins.print = lambda *x, **k: None        # the plugin's progress chatter
            try:
                img = hook(z)                            # warm-up (and the image compared below)
                torch.cuda.synchronize()
                ms = []
                for _ in range(a.reps):
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    s.record()
                    out = hook(z)
                    e.record()
                    torch.cuda.synchronize()
                    ms.append(s.elapsed_time(e))
                    del out
            finally:
                builtins.print = _print
        images[name] = img.float().cpu()
        del img
        ms.sort()
        rows.append({"mode": name, "ms_min": ms[0], "ms_median": ms[len(ms) // 2], "reps": a.reps})
    base = images.get("bf16x3")
    for r in rows:
        if base is not None and r["mode"] != "bf16x3":
            d = (images[r["mode"]].double() - base.double())
            r["rel_err_max_vs_bf16x3"] = d.abs().max().item() / base.abs().max().item()
            r["rel_l2_vs_bf16x3"] = (d.norm() / base.double().norm()).item()
            r["finite"] = bool(torch.isfinite(images[r["mode"]]).all())
        print(json.dumps(r))
    if "bf16x3" in images and "bf16" in images:
        t3 = next(r for r in rows if r["mode"] == "bf16x3")["ms_min"]
        t1 = next(r for r in rows if r["mode"] == "bf16")["ms_min"]
        print(json.dumps({"latent": a.latent, "tile": a.tile, "speedup_bf16_over_bf16x3": t3 / t1}))
    tmin = {r["mode"]: r["ms_min"] for r in rows}
    if "bf16x3" in tmin and "f16" in tmin:
        line = {"latent": a.latent, "tile": a.tile, "speedup_f16_over_bf16x3": tmin["bf16x3"] / tmin["f16"]}
        if "bf16" in tmin:
            line["f16_over_bf16"] = tmin["f16"] / tmin["bf16"]
        if "bf16x3#2" in tmin:
            line["bf16x3_run_to_run_ms"] = abs(tmin["bf16x3"] - tmin["bf16x3#2"])
            line["f16_gain_ms"] = min(tmin["bf16x3"], tmin["bf16x3#2"]) - tmin["f16"]
        print(json.dumps(line))
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"latent": a.latent, "tile": a.tile, "rows": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
