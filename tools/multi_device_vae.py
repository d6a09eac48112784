#!/usr/bin/env python3
"""Tiled VAE on several device slots of one process (VAEHook.devices) against one device: an alternating A/B in ONE process.

    python tools/multi_device_vae.py --devices 0,0,0,0,0,0,0,0 --latent 1024 --tile 256            (8K fast decode, 8 slots on cuda:0)
    python tools/multi_device_vae.py --devices 0,1,2,3 --mode slow                                    (4 GPUs: the scaling curve, point by point)

Prints ONE JSON line: the median wall time of each arm (host clock around a call that ends in a device synchronize), whether the two
images are torch.equal, which slot decoded each tile, and the tile assembly of the last multi-slot call (mdtile_vae_assemble) timed alone
with HIP events: its bytes (valid windows read + written), its GB/s and its fraction of mdtile_stream_copy moving the same bytes.
Random-weight SD decoder / encoder (ch=128), seeded input; --direction encode takes an image of 8 x latent px per side.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _event_ms(fn, k: int) -> float:
    import torch
    fn()
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--devices", default="0,0", help="the slots of the B arm: CUDA indices, cuda:0 first (default 0,0)")
    ap.add_argument("--direction", choices=["decode", "encode"], default="decode")
    ap.add_argument("--mode", choices=["fast", "slow"], default="fast")
    ap.add_argument("--latent", type=int, default=1024, help="latent side (decode input; the encode input is 8x this)")
    ap.add_argument("--tile", type=int, default=256, help="decoder tile (latent px) / encoder tile (image px)")
    ap.add_argument("--reps", type=int, default=3, help="timed calls per arm, alternating")
    ap.add_argument("--warmup", type=int, default=1, help="untimed calls per arm first")
    ap.add_argument("--asm-iters", type=int, default=20, help="event-timed repetitions of the assembly and of the copy")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("multi_device_vae.py needs a GPU (the engine has no CPU path)")
    import __graft_entry__ as ge
    with contextlib.redirect_stdout(sys.stderr):
        ge.build()
    from hostsim import stub_host as sh, ldm_decoder as ld
    torch.cuda.set_device(0)
    dev0 = torch.device("cuda", 0)
    sh.install(dev0)
    sh.set_device(dev0)
    pl = sh.load_plugin()
    E = pl.engine
    slots = [int(v) for v in args.devices.split(",")]
    is_dec = args.direction == "decode"
    fast = args.mode == "fast"
    net = (ld.make_decoder(0) if is_dec else ld.make_encoder(0)).to(dev0)
    net.original_forward = net.forward
    hook = pl.tilevae.VAEHook(net, args.tile, is_decoder=is_dec, fast_decoder=fast, fast_encoder=fast, color_fix=False)
    L = args.latent
    g = torch.Generator(device="cpu").manual_seed(0)
    x = (torch.randn(1, 4, L, L, generator=g) if is_dec else torch.randn(1, 3, 8 * L, 8 * L, generator=g)).to(dev0)

    captured = {}
    real_assemble = E.vae_assemble

    def capture(tiles, result, is_decoder=True):            # the tiles of the last multi-slot call, for the assembly timing below
        captured.update(tiles=list(tiles), result=result, is_decoder=is_decoder)
        return real_assemble(tiles, result, is_decoder)

    E.vae_assemble = capture

    def sync_all():
        for d in sorted(set(slots) | {0}):
            torch.cuda.synchronize(d)

    def call(devs):
        hook.devices = devs
        captured.clear()
        sync_all()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(sys.stderr):
            out = hook(x)
        sync_all()
        return time.perf_counter() - t0, out

    times = {"one": [], "slots": []}
    last = {}
    for r in range(args.warmup + args.reps):
        order = [("one", None), ("slots", slots)] if r % 2 == 0 else [("slots", slots), ("one", None)]
        for name, devs in order:
            last[name] = None                                   # the previous image of this arm is not kept alive through the call
            t, last[name] = call(devs)
            if r >= args.warmup:
                times[name].append(t)
        if r == args.warmup + args.reps - 1 and order[-1][0] == "one":
            t, last["slots"] = call(slots)                       # the captured tiles belong to a multi-slot call
    equal = bool(torch.equal(last["one"], last["slots"]))
    max_abs = float((last["one"].float() - last["slots"].float()).abs().max().item())
    tile_slots = hook.last_tile_slots
    del last

    asm = None
    if captured:
        tiles, result, isd = captured["tiles"], captured["result"], captured["is_decoder"]
        N, C = result.shape[:2]
        px = sum((ob[1] - ob[0]) * (ob[3] - ob[2]) for _, _, ob in tiles)
        nbytes = 2 * 4 * N * C * px                              # every valid element read once and written once
        t_asm = _event_ms(lambda: real_assemble(tiles, result, isd), args.asm_iters)
        half = (nbytes // 2) // 16 * 16
        src = torch.empty(half // 4, dtype=torch.float32, device=dev0).normal_()
        dst = torch.empty_like(src)
        copy = E.StreamCopyCall(src, dst)
        t_copy = _event_ms(copy, args.asm_iters)
        asm = {"tiles": len(tiles), "bytes": nbytes, "ms": round(t_asm, 4), "GBps": round(nbytes / (t_asm * 1e-3) / 1e9, 1),
               "stream_copy_ms": round(t_copy, 4), "stream_copy_GBps": round(2 * half / (t_copy * 1e-3) / 1e9, 1),
               "fraction_of_stream_copy": round(t_copy / t_asm * nbytes / (2 * half), 3), "tile_devices": sorted({t.device.index for t, _, _ in tiles})}
    one_ms, slot_ms = statistics.median(times["one"]) * 1e3, statistics.median(times["slots"]) * 1e3
    print(json.dumps({
        "tool": "multi_device_vae", "direction": args.direction, "mode": args.mode, "latent": L, "tile": args.tile, "devices": slots,
        "devices_visible": torch.cuda.device_count(), "reps": args.reps, "warmup": args.warmup,
        "one_device_ms_median": round(one_ms, 2), "slots_ms_median": round(slot_ms, 2), "ratio_slots_over_one": round(slot_ms / one_ms, 4),
        "one_device_ms": [round(t * 1e3, 2) for t in times["one"]], "slots_ms": [round(t * 1e3, 2) for t in times["slots"]],
        "bit_identical": equal, "max_abs_diff": max_abs, "last_tile_slots": tile_slots, "assemble": asm}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
