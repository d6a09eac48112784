#!/usr/bin/env python3
"""
bench.py -- latent-px/s of the tile-blend + tiled-VAE-decode hot path on an 8K image (BASELINE.json metric).

    python bench.py --gpus 1 --steps K --warmup W [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...
    python bench.py --gpus N ...                     (no launcher environment: bench.py starts its N ranks itself, same line, rc 0)
    python bench.py --gpus N --single-process ...    (ONE process driving N devices: mdtile_shard_init + VAEHook.devices, the form a webui uses)

One "step" = the whole hot path for ONE 8192x8192 image (latent 1024x1024, SDXL config of BASELINE.json):
    `--evals` (20) model evaluations of  [ tile gather (K2) -> overlap blend (K3-K7) ]   with 128x128 tiles, overlap 8,
    then ONE tiled VAE decode of the latent (decoder tile 256 = upstream's default for > 30 GB, fast mode).
The UNet itself is out of scope: the blend consumes pre-generated, HBM-resident tile outputs
~N(0,1); the VAE is an SD/SDXL-shaped decoder (ch=128, ch_mult 1-2-4-4) with seeded random weights (no checkpoints
offline).  Inputs are resident in HBM before the timed region; nothing is cached between steps.  In fast mode the decoder tiles shed the
part of their padding that the remaining 3x3 convs cannot carry into the valid rectangle ("live-window narrowing", scripts/tilevae.py:
live_windows; the assembled image is bit-identical to the whole-tile sweep; `config.vae_live_window`, MDTILE_LIVE_WINDOW=0 = whole tiles).
`whole_tiles` in the JSON line (--full) is the same step timed with the narrowing off, with `bit_identical_image` = torch.equal of the two 8K images.

N > 1: strong scaling of the same image -- diffusion tiles in row bands per rank with a neighbour halo exchange of the
overlap-row partial sums, VAE tiles dealt round-robin, the fast-mode GroupNorm estimator split by rows across the ranks
(mdtile/seqpar.py), the decoded tile rectangles gathered to rank 0 INSIDE the timed region (rank 0 ends every step with the
assembled 8192x8192 image, like the single-GPU run).  ONE RCCL communicator per rank: the engine's own (C ABI, csrc/shard.hip)
carries the whole data plane; torch.distributed runs on gloo for the control plane only (id broadcast, votes, barrier, the max
over ranks of the clock).  If the engine's communicator cannot be brought up on every rank, the job creates ONE torch "nccl"
group instead and the same collectives run there.
A plain run only sets up, warms up, times its steps, writes --dump-outputs and prints the JSON line.  With `--full` it then runs
the untimed passes (on N = 1 unless said otherwise), and the line carries what they measured (null without `--full`):
`stage_ms` (every form), `roofline` (every rank; the kernel class with the largest share of the step: the split-bf16 MFMA 3x3 conv;
flops = the ones executed, peak = 2500/3 TFLOP/s for a kernel that spends 3 bf16 MFMAs per product; `traffic` = HBM bytes
per launch when MDTILE_PMC_SUMMARY points at tools/pmc_summary.py's json of a previous rocprofv3 --pmc pass),
`roofline_blend` (the HBM-bound blend kernel), `whole_tiles`, `value_f32`, `parity`, `companions` and `cpu_baseline` (the
oracle = CPU port of the reference algorithm, timed on this box's host cores on a bounded sample); `--encode` adds its roofline
and parity, `--single-process` its `debug_check`.  The --no-* options drop single passes of a --full run.  `--debug-single-device`
(N > 1 ranks on one GPU) is a functional check whatever --full says: its `debug_check` is always computed.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
PLUGIN = os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd")
for _p in (ROOT, PLUGIN):
    if _p not in sys.path:
        sys.path.insert(0, _p)

HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)
MFMA_F32_PEAK_TFLOPS = 157.3   # MI355X_MICROARCH.md: fp32-input MFMA = fp32 vector peak
MFMA_BF16_PEAK_TFLOPS = 2500.0  # MI355X_MICROARCH.md: dense bf16 MFMA
# split-bf16 kernels issue 3 bf16 MFMAs per fp32-class product: their ceiling in ALGORITHMIC (fp32-equivalent) flops
MFMA_BF16X3_PEAK_TFLOPS = MFMA_BF16_PEAK_TFLOPS / 3.0

# the untimed passes a plain run leaves out (each can also be dropped from a --full run on its own)
FULL_PASSES = ("no_cpu_baseline", "no_whole_tile_pass", "no_f32_pass", "no_profile_pass", "no_oracle_pass", "no_stress_pass", "no_companions")


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--latent", type=int, default=1024, help="latent side (1024 = 8192x8192 image)")
    ap.add_argument("--tile", type=int, default=128)
    ap.add_argument("--overlap", type=int, default=8)
    ap.add_argument("--tile-bs", type=int, default=4)
    ap.add_argument("--evals", type=int, default=20, help="model evaluations (sampler steps) per image")
    ap.add_argument("--method", default="md", choices=["md", "mod"])
    ap.add_argument("--vae-tile", type=int, default=256)
    ap.add_argument("--slow-vae", action="store_true", help="slow-mode GroupNorm (pooled per norm) instead of fast mode")
    ap.add_argument("--no-vae", action="store_true")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every untimed pass: the per-stage split, the per-kernel and blend rooflines, the whole-tile and "
                         "strict-fp32 companion steps, the parity legs against the oracle, the companion configurations and the CPU baseline (several "
                         "minutes at the default size).  Without it the run only sets up, warms up, times its steps, dumps its outputs if asked and prints "
                         "the line; the fields of the skipped passes are null.  The --no-* options below drop single passes of a --full run")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-whole-tile-pass", action="store_true", help="skip the companion step with the live-window narrowing off (whole_tiles in the JSON line)")
    ap.add_argument("--no-f32-pass", action="store_true", help="skip the strict-fp32 companion decode (parity.rel_err_vs_f32, value_f32)")
    ap.add_argument("--no-profile-pass", action="store_true", help="skip the HIP-event roofline pass and the decode of the per-stage split (PMC runs)")
    ap.add_argument("--no-oracle-pass", action="store_true", help="skip parity.rel_err_vs_oracle (assembled cfg3 decode vs the oracle on the GPU, untimed)")
    ap.add_argument("--no-stress-pass", action="store_true", help="skip parity.rel_err_vs_oracle_stress (cfg3 decode of the trained-like 'stress' decoder vs the oracle on the GPU, untimed)")
    ap.add_argument("--encode", action="store_true", help="the ENCODE direction instead (SURVEY section 8 f1): one line for the tiled VAE encode of an "
                    "8192x8192 image at encoder tile 3072 -- time, dominant kernel + roofline fraction, parity of one tile vs the oracle")
    ap.add_argument("--encode-side", type=int, default=8192)
    ap.add_argument("--encode-tile", type=int, default=3072)
    ap.add_argument("--cpu-vae-latent", type=int, default=88, help="width of the 64-row latent of the CPU VAE sample")
    ap.add_argument("--no-companions", action="store_true", help="skip the `companions` object (the other configurations of SURVEY section 8d: slow mode, "
                    "encode, cfg3 MoD + decode at tile 256 / 64, cfg2 / cfg4@ov64 / cfg5 blends; untimed for the headline, ~60 s)")
    ap.add_argument("--single-process", action="store_true",
                    help="N > 1 inside ONE process: the blend through mdtile.Shard(dev_ids) + ShardedBlend (row bands, halo exchange behind the C ABI), the "
                         "decode through VAEHook.devices (tiles dealt to the devices, one stream each) -- what an A1111 process can use (SURVEY 8e)")
    ap.add_argument("--debug-single-device", action="store_true",
                    help="functional check of the N > 1 flow on ONE GPU: every rank uses cuda:0 and gloo (host-staged) instead "
                         "of RCCL; the numbers it prints are meaningless")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned (blend output, decoded image; the encode's latent "
                         "moments with --encode) as DIR/<name>.npy, float32, at most 48 MiB in all: an array larger than its cap is "
                         "replaced by a fixed, seeded sample of its elements (DIR/manifest.json says which).  Inputs are seeded: the "
                         "same arguments give the same inputs on every run")
    args = ap.parse_args()
    if not args.full:
        for name in FULL_PASSES:
            setattr(args, name, True)
    return args


class Profile:
    """Per-launch HIP-event timing of the engine's kernels on torch's current stream (the stream they are launched on)."""

    def __init__(self):
        self.records = []   # (tag, work, start_event, end_event)
        self.extra = []     # (tag, n, work, seconds) measured elsewhere

    def wrap(self, tag, work, fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        self.records.append((tag, work, s, e))
        return out

    def add(self, tag, n, work, secs):
        self.extra.append((tag, n, work, secs))

    def summary(self):
        torch.cuda.synchronize()
        agg = {}
        for tag, n, work, secs in self.extra:
            a = agg.setdefault(tag, [0, 0.0, 0.0])
            a[0] += n
            a[1] += work
            a[2] += secs
        for tag, work, s, e in self.records:
            a = agg.setdefault(tag, [0, 0.0, 0.0])
            a[0] += 1
            a[1] += work
            a[2] += s.elapsed_time(e) * 1e-3
        return agg

def _free_port() -> int:
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def self_launch(args) -> int:
    """`python bench.py --gpus N` with no launcher environment (no WORLD_SIZE): start the N ranks here -- the same
    `python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port <free>` the driver's documented
    command uses, on this file with the same arguments -- and hand its exit code on.  Rank 0 of the children prints the one JSON line
    (this process prints nothing on stdout).  On a box with fewer than N GPUs the ranks share cuda:0 over gloo (`--debug-single-device`:
    the complete N-rank flow as a functional run; the line says so in `transport` / `devices_visible`)."""
    import subprocess
    visible = torch.cuda.device_count() if torch.cuda.is_available() else 0
    if visible < 1:
        raise SystemExit("bench.py needs an MI355X (no CPU fallback path exists in the product)")
    argv = list(sys.argv[1:])
    if visible < args.gpus and "--debug-single-device" not in argv:
        argv.append("--debug-single-device")
        print(f"[bench] {visible} GPU(s) visible, {args.gpus} ranks asked for: every rank uses cuda:0 and gloo (functional run of the N-rank flow; "
              "its numbers say nothing about scaling)", file=sys.stderr)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__)] + argv
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MDTILE_BENCH_LAUNCHER="bench.py (spawned torch.distributed.run itself)")
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC: RCCL / device-memory sharing across processes needs it on this driver
    env.setdefault("OMP_NUM_THREADS", "8")
    return subprocess.run(cmd, env=env).returncode


class Instrument:
    """Context manager: a HIP-event pair around every conv / attention launch the engine's Python entry points make, booked under the
    kernel symbol (family) the C ABI dispatches that call to.  The events sit on torch's current stream = the stream of the launch."""

    def __init__(self, E, prof: Profile):
        self.E, self.prof = E, prof

    def __enter__(self):
        E, prof = self.E, self.prof
        PC = E.PackedConv
        bfx = E.get_precision() == E.PRECISION_BF16X3
        self._saved = (PC.__call__, PC.call_rec, PC.down2, E.vae_attn, PC.call_stats, PC.call_rec_stats)
        o_call, o_rec, o_down, o_attn, o_cs, o_crs = self._saved

        def handover(self_, x, upsample2x, token_major, exact):
            B, cin, H, W = x.shape
            if upsample2x:
                H, W = 2 * H, 2 * W
            flops = 2.0 * B * H * W * self_.cout * cin * self_.ksize * self_.ksize
            bf = bfx and not exact and not token_major and cin % 16 == 0
            if self_.ksize == 1:
                tag = "k_conv1x1_stream<*> / k_conv1x1_bf16x3<*>" if (bf and cin % 32 == 0) else "k_conv<1,*> (exact fp32 MFMA)"
            elif upsample2x and bf:
                flops *= 4.0 / 9.0      # sub-pixel form of nearest-2x + 3x3 conv: four 2x2 convs -> 4/9 of the MACs are EXECUTED
                tag = "k_upconv_bf16x3<*> (fp32 hand-over)"
            else:
                tag = "k_conv3x3_bf16x3<*> (fp32 hand-over)" if bf else "k_conv3x3_fewcin<*> (conv_in, fp32 FMA)" if cin in (3, 4) and not token_major \
                    else "k_conv<3,*> (exact fp32 MFMA)"
            return tag, flops

        def rec(self_, x, upsample2x, window):
            # record kernels: the tag IS the kernel symbol mdtile_conv2d_rec launches (csrc/vae_conv_rec.hip, dispatch at the end)
            B, cin, H, W = x.shape
            if window is not None:
                H, W = window[2], window[3]      # live-window narrowing: the flops EXECUTED are those of the window
            if upsample2x:
                H, W = 2 * H, 2 * W
            flops = 2.0 * B * H * W * self_.cout * cin * 9
            if upsample2x:
                return "k_upconv_rec", flops * 4.0 / 9.0
            return ("k_conv3x3_rec<2, 2, 4>" if self_.cout % 128 == 0 else "k_conv3x3_rec<1, 1, 2>"), flops

        def t_call(self_, x, residual=None, upsample2x=False, token_major=False, exact=False, pre_gn=None):
            tag, flops = handover(self_, x, upsample2x, token_major, exact)
            return prof.wrap(tag, flops, lambda: o_call(self_, x, residual, upsample2x, token_major, exact, pre_gn))

        def t_cs(self_, x, pre_gn, residual=None, groups=32):
            tag, flops = handover(self_, x, False, False, False)
            return prof.wrap(tag, flops, lambda: o_cs(self_, x, pre_gn, residual, groups))

        def t_rec(self_, x, residual=None, upsample2x=False, want_f32=True, want_rec=False, rec_coef=None, window=None, family=0):
            tag, flops = rec(self_, x, upsample2x, window)
            return prof.wrap(tag, flops, lambda: o_rec(self_, x, residual, upsample2x, want_f32, want_rec, rec_coef, window, family))

        def t_crs(self_, x, residual=None, upsample2x=False, family=0, groups=32):
            tag, flops = rec(self_, x, upsample2x, None)
            return prof.wrap(tag, flops, lambda: o_crs(self_, x, residual, upsample2x, family, groups))

        def t_down(self_, x):
            B, cin, H, W = x.shape
            ho, wo = (H - 2) // 2 + 1, (W - 2) // 2 + 1
            return prof.wrap("k_conv3x3_bf16x3<*, false, 2> (Downsample)" if bfx else "k_conv<3,*,2> (exact fp32 MFMA)", 2.0 * B * ho * wo * self_.cout * cin * 9,
                             lambda: o_down(self_, x))

        def t_attn(q, k, v, scale, exact=False, v_channel_major=False):
            B, Cc, T = q.shape
            return prof.wrap("k_attn_bf16x3<512>" if bfx and not exact and Cc == 512 else "k_attn_bf16x3<*>" if bfx and not exact else "k_attn<*> (exact fp32 MFMA)",
                             4.0 * B * T * T * Cc, lambda: o_attn(q, k, v, scale, exact, v_channel_major))

        PC.__call__, PC.call_rec, PC.down2, E.vae_attn, PC.call_stats, PC.call_rec_stats = t_call, t_rec, t_down, t_attn, t_cs, t_crs
        return self

    def __exit__(self, *exc):
        PC = self.E.PackedConv
        PC.__call__, PC.call_rec, PC.down2, self.E.vae_attn, PC.call_stats, PC.call_rec_stats = self._saved
        return False


def _quiet(fn):
    """Run fn() with the plugin's progress chatter kept off stdout (the JSON line must stay the only line there)."""
    import builtins
    keep = builtins.print
    builtins.print = lambda *a, **k: None
    try:
        return fn()
    finally:
        builtins.print = keep


DUMP_SEED = 0
DUMP_FULL_ELEMS = 8 << 20       # the whole blend output of the default 1024^2 latent (N=2, C=4), or the encoder moments: 32 MiB
DUMP_IMAGE_ELEMS = 4 << 20      # a 16 MiB sample of the 8K image (805 MB of float32 in full)


def dump_outputs(out_dir: str, arrays: dict) -> None:
    """--dump-outputs: name -> (tensor, max elements).  A tensor above its cap is written as the values at a fixed set of flat indices
    (seeded by DUMP_SEED and the tensor's size only, so two builds sample the same positions)."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    manifest = {}
    for name, (t, cap) in arrays.items():
        flat = t.detach().reshape(-1)
        entry = {"shape": list(t.shape), "dtype": str(t.dtype), "sampled": flat.numel() > cap}
        if entry["sampled"]:
            idx = torch.randint(flat.numel(), (cap,), generator=torch.Generator().manual_seed(DUMP_SEED)).unique()   # sorted
            flat = flat[idx.to(flat.device)]
            entry.update(sample_seed=DUMP_SEED, sample_size=int(idx.numel()))
        a = flat.cpu().numpy() if entry["sampled"] else t.detach().cpu().numpy()
        np.save(os.path.join(out_dir, name + ".npy"), a.astype(np.float64 if t.dtype == torch.float64 else np.float32))
        manifest[name] = entry
    with open(os.path.join(out_dir, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)


def err_metrics(out: torch.Tensor, ref: torch.Tensor):
    """(max |d| / max |ref|, rms(d) / max |ref|, ||d||_2 / ||ref||_2): the range-normalised figures every parity leg has printed since
    round 2, and the relative L2 error (the stricter reading of "1e-3 rel-err")."""
    d = (out.float() - ref.float())
    den = ref.float().abs().max().item()
    l2 = (d.double().pow(2).sum().sqrt() / ref.double().pow(2).sum().sqrt()).item()
    return float(d.abs().max().item() / den), float((d.pow(2).mean().sqrt() / den).item()), float(l2)


def measure_vae(E, hook, x, runs: int = 1):
    """One tiled VAE pass three ways: warm (untimed), `runs` timed passes on the wall clock, one instrumented pass whose per-launch HIP-event
    times are summed -- kernel_sum / wall says how much of the pass is GPU kernels of the conv / attention families (the rest: host gaps,
    the small elementwise / statistics / crop kernels)."""
    _quiet(lambda: hook(x))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(runs):
        y = _quiet(lambda: hook(x))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / runs
    prof = Profile()
    with Instrument(E, prof):
        _quiet(lambda: hook(x))
    agg = {k: v for k, v in prof.summary().items() if k.startswith("k_")}
    ksum = sum(v[2] for v in agg.values()) * 1e3
    top = sorted(agg.items(), key=lambda kv: -kv[1][2])[:3]
    del y
    return {"ms": round(ms, 2), "kernel_sum_ms": round(ksum, 2), "kernel_sum_over_wall": round(ksum / ms, 4),
            "top_kernels_ms": {k: round(v[2] * 1e3, 2) for k, v in top}}


def blend_setup(E, dev, W, H, tile, overlap, tile_bs, method_name, region_fracs=(), N=2, C=4, seed=1):
    """Engine-level state of one blend configuration, as the delegates build it (tile_methods/*.py: init_grid_bbox, init_custom_bbox, init_done):
    plan, weight map (+ 1 per background region for MD, Gaussian layers + reciprocal for MoD), pre-generated tile / region outputs ~N(0,1),
    the marshalled gather and blend calls and the blend's algorithmic bytes."""
    import math
    method = E.METHOD_MD if method_name == "md" else E.METHOD_MOD
    plan = E.Plan(W, H, tile, tile, overlap, tile_bs)
    weights = torch.zeros(1, 1, H, W, device=dev)
    tile_w = E.gaussian_weights(plan.tile_w, plan.tile_h, dev) if method == E.METHOD_MOD else None
    E.weight_map_add_grid(plan, tile_w, weights)
    g = torch.Generator(device="cpu").manual_seed(seed)
    specs, region_bytes = [], 0
    rects = []
    for (fx, fy, fw, fh, mode, fr) in region_fracs:
        x, y = max(0, int(fx * W)), max(0, int(fy * H))
        w, h = min(W - x, math.ceil(fw * W)), min(H - y, math.ceil(fh * H))
        rects.append((x, y, w, h, mode, fr))
    rw = []
    for (x, y, w, h, mode, fr) in rects:
        if mode == "bg":
            cw = E.gaussian_weights(w, h, dev) if method == E.METHOD_MOD else None
            E.weight_map_add_rect(weights, x, y, w, h, cw, 1.0)
            rw.append(cw)
        else:
            rw.append(E.feather_mask(w, h, fr, dev))
    rescale = None
    if method == E.METHOD_MOD:
        rescale = E.reciprocal(weights)
        for k, (x, y, w, h, mode, fr) in enumerate(rects):
            if mode == "bg":
                E.rect_mul_canvas(rw[k], rescale, x, y, w, h)
    for k, (x, y, w, h, mode, fr) in enumerate(rects):
        out = torch.randn(N, C, h, w, generator=g).to(dev)
        specs.append(E.RegionSpec(x, y, w, h, E.REGION_BG if mode == "bg" else E.REGION_FG, out, rw[k]))
        region_bytes += 4 * N * C * h * w + (4 * h * w if rw[k] is not None else 0)
    x_in = torch.randn(N, C, H, W, generator=g).to(dev)
    tile_out = torch.randn(plan.num_tiles * N, C, plan.tile_h, plan.tile_w, generator=g).to(dev)
    x_tiles = torch.empty_like(tile_out)
    out = torch.empty(N, C, H, W, device=dev)
    kw = dict(weights=weights) if method == E.METHOD_MD else dict(tile_w=tile_w, rescale=rescale)
    gather = E.GatherRangeCall(plan, x_in, x_tiles, 0, plan.num_tiles)
    blend = E.BlendCall(plan, method, [tile_out], N, C, out=out, packed=True, regions=specs, **kw)
    nbytes = 4 * (plan.num_tiles * N * C * plan.tile_h * plan.tile_w + N * C * H * W) + 4 * H * W * (1 if method == E.METHOD_MD else 2) + region_bytes
    return plan, gather, blend, nbytes


def time_launches(calls, n: int = 20, rounds: int = 5):
    """Median over `rounds` of the time of `n` back-to-back launches (rotating through `calls`) between ONE pair of HIP events on the launch
    stream, per launch in seconds (an event pair per launch would time the host's launch latency while the GPU idles)."""
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
        ts.append(s.elapsed_time(e) * 1e-3 / n)
    return sorted(ts)[len(ts) // 2]


def blend_companion(E, dev, W, H, tile, overlap, method_name, region_fracs=()):
    """One blend configuration of SURVEY section 8(d) as a companion figure: the blend kernel per launch (HIP events, 20 back to back) and the
    evaluation (tile gather + blend, as the sampler loop issues them) on the wall clock."""
    plan, gather, blend, nbytes = blend_setup(E, dev, W, H, tile, overlap, 4, method_name, region_fracs)
    t_k = time_launches([blend])
    for _ in range(3):
        gather(); blend()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        gather(); blend()
    torch.cuda.synchronize()
    t_eval = (time.perf_counter() - t0) / 20
    return {"blend_us": round(t_k * 1e6, 2), "eval_wall_us": round(t_eval * 1e6, 2), "blend_over_eval": round(t_k / t_eval, 4),
            "tiles": plan.num_tiles, "tile": [plan.tile_w, plan.tile_h], "overlap": plan.overlap, "latent": [W, H], "regions": len(region_fracs),
            "method": method_name, "bytes_per_launch": int(nbytes), "GBps": round(nbytes / t_k / 1e9, 1),
            "frac_of_hbm_peak": round(nbytes / t_k / 1e9 / HBM_PEAK_GBS, 4)}


def run_companions(args, E, pl, ld, dev, dec, z, t_blend_eval):
    """The other configurations SURVEY section 8(d) names, on the driver's default line: untimed for the headline,
    each with its own clock and its kernel-sum / wall ratio.  All on this GPU, default precision, same decoder weights as the headline."""
    out = {}
    tv = pl.tilevae
    t_all = time.perf_counter()
    # --- slow-mode GroupNorm (pooled per norm across tiles, upstream tilevae.py:289-361) on the SAME 8K latent at the bench's decoder tile
    hook = tv.VAEHook(dec, args.vae_tile, is_decoder=True, fast_decoder=False, fast_encoder=False, color_fix=False)
    m = measure_vae(E, hook, z)
    out["slow_vae_ms"] = {"step_ms": round(args.evals * t_blend_eval * 1e3 + m["ms"], 2), "decode": m,
                          "what": f"the headline step with slow-mode GroupNorm: {args.evals} x blend evaluation + tiled decode of the {args.latent}x{args.latent} latent at decoder tile {args.vae_tile}"}
    del hook
    torch.cuda.empty_cache()
    # --- cfg3: 4096^2 Mixture-of-Diffusers (Gaussian weights, 96 / 48) + tiled decode at tile 256 and at tile 64 (fast mode)
    b3 = blend_companion(E, dev, 512, 512, 96, 48, "mod")
    z3 = torch.randn(1, 4, 512, 512, generator=torch.Generator(device="cpu").manual_seed(3)).to(dev)
    for name, ts in (("cfg3_mod_tile256_ms", 256), ("cfg3_tile64_ms", 64)):
        hook = tv.VAEHook(dec, ts, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
        m = measure_vae(E, hook, z3, runs=2)
        out[name] = {"step_ms": round(args.evals * b3["eval_wall_us"] * 1e-3 + m["ms"], 2), "decode": m, "blend": b3 if ts == 256 else None,
                     "what": f"BASELINE cfg3: 4096x4096 (latent 512x512), {args.evals} x Mixture-of-Diffusers blend (100 tiles 96x96, overlap 48) + tiled VAE decode at tile {ts}, fast mode"}
        del hook
    del z3
    torch.cuda.empty_cache()
    # --- blend-only configurations: cfg2 (2048^2 MD 96 / 48), cfg4 at overlap 64 (225 tiles), cfg5 (4096 x 1024 panorama + 3 regions)
    out["cfg2_blend_us"] = blend_companion(E, dev, 256, 256, 96, 48, "md")
    out["cfg4_ov64_blend_us"] = blend_companion(E, dev, 1024, 1024, 128, 64, "md")
    regs = [(0.0, 0.0, 0.4, 1.0, "bg", 0.2), (0.3, 0.0, 0.4, 1.0, "bg", 0.2), (0.6, 0.1, 0.4, 0.8, "fg", 0.2)]
    out["cfg5_regions_blend_us"] = blend_companion(E, dev, 512, 128, 96, 48, "md", regs)
    torch.cuda.empty_cache()
    # --- the ENCODE direction: 8192^2 image at encoder tile 3072 (upstream's recommendation for large VRAM), fast mode
    enc = ld.make_encoder(0).to(dev)
    enc.original_forward = enc.forward
    hook = tv.VAEHook(enc, args.encode_tile, is_decoder=False, fast_decoder=False, fast_encoder=True, color_fix=False)
    xi = torch.randn(1, 3, args.encode_side, args.encode_side, generator=torch.Generator().manual_seed(1)).to(dev)
    m = measure_vae(E, hook, xi)
    out["encode_ms"] = {"step_ms": m["ms"], "encode": m, "latent_px_per_s": round((args.encode_side // 8) ** 2 / (m["ms"] * 1e-3), 1),
                        "what": f"tiled VAE ENCODE of a {args.encode_side}x{args.encode_side} image at encoder tile {args.encode_tile}, fast mode (`bench.py --encode` prints its own line with parity)"}
    del hook, enc, xi
    torch.cuda.empty_cache()
    out["seconds"] = round(time.perf_counter() - t_all, 1)
    out["what"] = ("companion figures, untimed for the headline: one warm + timed pass(es) + one HIP-event-instrumented pass each; `kernel_sum_over_wall` = the conv / "
                   "attention launches' event time over the pass's wall time")
    return out


def run_encode(args, E, pl, ld, dev):
    """`--encode`: the tiled VAE ENCODE (upstream scripts/tilevae.py:155-171 Downsample tasks, :492-496 encoder estimator, :507-656 the tile
    sweep with is_decoder=False) of one image on one GPU: W untimed + K timed encodes, per-kernel HIP-event roofline of one extra encode,
    and -- untimed -- ONE tile of the timed image against the oracle (oracle/vae_oracle.py via oracle/gpu_reference.py, fast mode:
    with every GroupNorm frozen a tile depends on no other tile)."""
    import builtins
    side, tile = args.encode_side, args.encode_tile
    enc = ld.make_encoder(0).to(dev)
    enc.original_forward = enc.forward
    hook = pl.tilevae.VAEHook(enc, tile, is_decoder=False, fast_decoder=False, fast_encoder=not args.slow_vae, color_fix=False)
    x = torch.randn(1, 3, side, side, generator=torch.Generator().manual_seed(1)).to(dev)
    _print = builtins.print

    def quiet(fn):
        builtins.print = lambda *a, **k: None
        try:
            return fn()
        finally:
            builtins.print = _print

    for _ in range(max(1, args.warmup)):
        quiet(lambda: hook(x))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        y = quiet(lambda: hook(x))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / args.steps
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"latent": (y, DUMP_FULL_ELEMS)})
    lat = (side // 8) * (side // 8)
    # per-kernel roofline of one more encode (HIP events around every conv / attention launch, same stream)
    roofline = None
    if args.full:
        prof = Profile()
        with Instrument(E, prof):
            quiet(lambda: hook(x))
        agg = prof.summary()
        mm = {k: v for k, v in agg.items() if k.startswith("k_")}
        dom = max(mm, key=lambda k_: mm[k_][2])
        n, work, secs = mm[dom]
        peak = MFMA_BF16X3_PEAK_TFLOPS if ("bf16x3" in dom or "_rec" in dom) else MFMA_F32_PEAK_TFLOPS
        roofline = {"kernel": dom, "bound": "mfma", "achieved": round(work / secs / 1e12, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                    "frac": round(work / secs / 1e12 / peak, 4), "traffic": None, "launches": n, "avg_us": round(secs / n * 1e6, 1),
                    "share_of_encode": round(secs / (ms * 1e-3), 3),
                    "breakdown_s": {k: round(v[2], 4) for k, v in sorted(agg.items())},
                    "breakdown_tflops": {k: round(v[1] / v[2] / 1e12, 2) for k, v in sorted(mm.items())}}
    # parity: one tile of the timed image vs the oracle on this GPU (fast mode only)
    parity = None
    if not args.no_oracle_pass and not args.slow_vae:
        from oracle import gpu_reference as gr, vae_oracle as vo
        ins, outs = vo.split_tiles(side, side, tile, False)
        pick = len(ins) // 2 if len(ins) > 2 else len(ins) - 1
        t0 = time.perf_counter()
        (ob, crop), = quiet(lambda: gr.tiled_forward_gpu(enc, x, tile, True, is_decoder=False, only_tiles=[pick]))
        t_or = time.perf_counter() - t0
        mine = y.float()[:, :, ob[2]:ob[3], ob[0]:ob[1]]
        den = y.float().abs().max().item()
        crop = crop.to(mine.device)
        d = (mine - crop).abs()
        parity = {"rel_err_vs_oracle_tile": float(d.max().item() / den), "rms_err_vs_oracle_tile": float((d.pow(2).mean().sqrt() / den).item()),
                  "rel_l2_vs_oracle_tile": err_metrics(mine, crop)[2], "tile": pick,
                  "pixel_in_bbox": ins[pick], "latent_out_bbox": ob, "tolerance": 1e-3,
                  "what": f"tile {pick} of {len(ins)} of the TIMED image: the engine's moments vs the oracle's encode of the same tile with its own estimator "
                          f"statistics (torch fp32 on this GPU, {t_or:.0f} s); relative to the output's absolute maximum"}
    # parity on TRAINED-LIKE statistics (hostsim/ldm_decoder.py: apply_stress on the ENCODER): the assembled encode of a 4096 x 4096 image at the same
    # encoder tile (2 x 2 tiles of ~2080^2 px), default precision and the strict-fp32 engine against the oracle on this GPU (untimed)
    if not args.no_stress_pass and not args.slow_vae:
        from oracle import gpu_reference as gr
        del x, y
        torch.cuda.empty_cache()
        enc_s = ld.make_encoder(0, stress=8).to(dev)
        enc_s.original_forward = enc_s.forward
        xs_ = torch.randn(1, 3, 4096, 4096, generator=torch.Generator().manual_seed(5)).to(dev)
        t0 = time.perf_counter()
        ref = quiet(lambda: gr.tiled_forward_gpu(enc_s, xs_, tile, True, is_decoder=False)).float().cpu()
        t_or = time.perf_counter() - t0
        torch.cuda.empty_cache()
        hook_s = pl.tilevae.VAEHook(enc_s, tile, is_decoder=False, fast_decoder=False, fast_encoder=True, color_fix=False)
        out = quiet(lambda: hook_s(xs_)).float().cpu()
        try:
            E.set_precision(E.PRECISION_F32)
            out32 = quiet(lambda: hook_s(xs_)).float().cpu()
        finally:
            E.set_precision(E.PRECISION_BF16X3)
        parity = parity or {"tolerance": 1e-3}
        e, e32 = err_metrics(out, ref), err_metrics(out32, ref)
        parity.update({"rel_err_vs_oracle_stress": e[0], "rms_err_vs_oracle_stress": e[1], "rel_l2_vs_oracle_stress": e[2],
                       "rel_err_vs_oracle_stress_f32_engine": e32[0], "rel_l2_vs_oracle_stress_f32_engine": e32[2],
                       "stress_what": f"assembled ENCODE of a 4096x4096 image at encoder tile {tile} (fast mode) of the trained-like 'stress' encoder (hostsim/ldm_decoder.py: "
                                      f"apply_stress): default precision and the strict-fp32 engine vs the oracle on torch fp32 on this GPU ({t_or:.0f} s); bar 2e-4",
                       "stress_recipe": getattr(enc_s, "stress_info", None)})
    return {"metric": "latent-px/sec tiled-VAE-encode, 8K image", "value": round(lat / (ms * 1e-3), 1), "unit": "latent-px/s", "n_gpus": 1, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms, 2), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32" if E.get_precision() == E.PRECISION_F32 else "bf16x3+f32", "data": "synthetic", "full": args.full,
            "config": {"workload": f"tiled VAE ENCODE of a {side}x{side} image (encoder tile {tile}, {'slow' if args.slow_vae else 'fast'} mode, SD encoder ch=128, random weights) "
                                   f"-> {side // 8}x{side // 8} latent moments", "image": [side, side], "vae_tile": tile},
            "roofline": roofline, "parity": parity, "cpu_baseline": None,
            "note": "companion line of the ENCODE direction (SURVEY section 8 f1); the headline metric of BASELINE.json is the default run"}

def run_single_process(args):
    """`--gpus N --single-process`: the N-device flow inside ONE process -- the only shape an A1111 webui can use ("must be
    single-process multi-device").  Blend: mdtile.Shard(dev_ids) (mdtile_shard_init: one RCCL communicator per device via ncclCommInitAll, or
    peer copies) + mdtile.sharding.ShardedBlend (row bands of tiles per device, halo exchange of the overlap rows behind the C ABI, finalize
    per band).  Decode: VAEHook.devices -- estimator on the first device, tiles dealt to the devices by area, one stream and one packed copy
    of the weights per device, the decoded rectangles copied into the first device's canvas inside the step.  One Python thread issues
    every launch; the devices run asynchronously.  On a box with fewer than N GPUs cuda:0 is listed N times (functional run)."""
    visible = torch.cuda.device_count()
    n = args.gpus
    shared_device = visible < n
    devs = [0] * n if shared_device else list(range(n))
    torch.cuda.set_device(0)
    dev0 = torch.device("cuda", 0)
    import __graft_entry__ as ge
    ge.build()
    from hostsim import stub_host as sh, ldm_decoder as ld
    sh.install(dev0)
    sh.set_device(dev0)
    pl = sh.load_plugin()
    E = pl.engine
    from mdtile import sharding
    try:
        shard = E.Shard(dev_ids=devs)
    except E.MdtileError as e:      # RCCL could not build the in-process communicators: peer copies carry the same calls
        print(f"[bench] mdtile_shard_init over RCCL failed ({e}); retrying on the copy transport", file=sys.stderr)
        os.environ["MDTILE_SHARD_TRANSPORT"] = "copy"
        shard = E.Shard(dev_ids=devs)
    transport = ("rccl (ncclCommInitAll inside the process, C ABI)" if shard.rccl else "copy (peer hipMemcpyAsync + events, C ABI)") + \
        (" -- cuda:0 listed %d times: functional run" % n if shared_device else "")
    shard.selfcheck()
    L, N, C = args.latent, 2, 4
    method = E.METHOD_MD if args.method == "md" else E.METHOD_MOD
    sb = sharding.ShardedBlend(shard, L, L, args.tile, args.tile, args.overlap, args.tile_bs, method)
    plan = sb.local[0]["plan"]
    x_cpu = torch.randn(N, C, L, L, generator=torch.Generator(device="cpu").manual_seed(0))
    full = torch.randn(plan.num_tiles * N, C, plan.tile_h, plan.tile_w, generator=torch.Generator(device="cpu").manual_seed(1))
    xs, pre = [], []
    for i, d in enumerate(devs):
        b = sb.bands[i]
        xs.append(x_cpu.to(torch.device("cuda", d)))
        pre.append(None if b.empty else full[b.tile_lo * N:b.tile_hi * N].to(torch.device("cuda", d)))
    del full
    order = [i for i in range(n) if not sb.bands[i].empty]
    cursor = [0]

    def tile_fn(x_tiles):          # the pre-generated model outputs of the band whose turn it is (ShardedBlend.step walks the local ranks in order)
        i = order[cursor[0] % len(order)]
        cursor[0] += 1
        return pre[i]

    def blend_eval():
        cursor[0] = 0
        return sb.step(xs, tile_fn)

    hook = z = dec = None
    if not args.no_vae:
        if args.slow_vae:
            raise SystemExit("--single-process decodes in fast mode (VAEHook.devices needs no collective: the frozen statistics are computed once and copied)")
        dec = ld.make_decoder(0).to(dev0)
        dec.original_forward = dec.forward
        hook = pl.tilevae.VAEHook(dec, args.vae_tile, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
        hook.devices = devs
        z = torch.randn(1, 4, L, L, generator=torch.Generator(device="cpu").manual_seed(2)).to(dev0)

    def sync_all():
        for d in sorted(set(devs)):
            torch.cuda.synchronize(d)

    last = {}

    def step():
        last.clear()            # the previous step's outputs are not kept alive through this one
        outs = None
        for _ in range(args.evals):
            outs = blend_eval()
        last.update(outs=outs, image=hook(z) if hook is not None else None)

    def timed(fn, k):
        sync_all()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        sync_all()
        return (time.perf_counter() - t0) / k

    for _ in range(args.warmup):
        _quiet(step)
    elapsed = timed(lambda: _quiet(step), args.steps)
    if args.dump_outputs and last:
        dump = {}
        if last["outs"] is not None:      # every band's owned rows, assembled like the one-device blend output
            canvas = torch.zeros(N, C, L, L)
            for i in order:
                b = sb.bands[i]
                canvas[:, :, b.own_lo:b.own_hi] = last["outs"][i][:, :, b.own_lo:b.own_hi].cpu()
            dump["blend_out"] = (canvas, DUMP_FULL_ELEMS)
        if last["image"] is not None:
            dump["image"] = (last["image"], DUMP_IMAGE_ELEMS)
        dump_outputs(args.dump_outputs, dump)
    last.clear()
    t_blend = t_vae = check = None
    if args.full:
        t_blend = timed(blend_eval, args.evals)
        t_vae = timed(lambda: _quiet(lambda: hook(z)), 1) if hook is not None else None
    if args.full and hook is not None:
        # the assembled image of the N-device sweep against the plain one-device sweep of the same latent (same kernels, same frozen
        # statistics: bit for bit) -- and the sharded blend's canvas rows against the one-device blend
        img = _quiet(lambda: hook(z)).float()
        hook.devices = None
        ref = _quiet(lambda: hook(z)).float()
        hook.devices = devs
        check = {"assembled_image_bit_identical_to_one_device": bool(torch.equal(img, ref)),
                 "assembled_image_rel_err_vs_one_device": float((img - ref).abs().max().item() / ref.abs().max().item()), "image_shape": list(img.shape)}
        del img, ref
    if args.full:
        kw = dict(weights=sb.local[0]["weights"]) if method == E.METHOD_MD else dict(tile_w=sb.local[0]["tile_wt"], rescale=sb.local[0]["rescale"])
        with torch.cuda.device(dev0):
            full0 = torch.randn(plan.num_tiles * N, C, plan.tile_h, plan.tile_w, generator=torch.Generator(device="cpu").manual_seed(1)).to(dev0)
            one = E.blend(plan, method, [full0], N, C, packed=True, **kw)
        outs = blend_eval()
        sync_all()
        worst = 0.0
        for i in order:
            b = sb.bands[i]
            worst = max(worst, float((outs[i][:, :, b.row_lo:b.row_hi].to(dev0) - one[:, :, b.row_lo:b.row_hi]).abs().max().item()))
        check = dict(check or {}, sharded_blend_max_abs_diff_vs_one_device=worst)
        del full0, one
    value = L * L / elapsed
    print(json.dumps({
        "metric": "latent-px/sec tile-blend+VAE-decode, 8K image", "value": round(value, 1), "unit": "latent-px/s", "n_gpus": n, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(elapsed * 1e3, 3), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f32" if E.get_precision() == E.PRECISION_F32 else "bf16x3+f32", "data": "synthetic", "full": args.full,
        "config": {"workload": f"{'SDXL ' if L == 1024 else ''}{8 * L}x{8 * L} (latent {L}x{L}): {args.evals} x [tile gather + {'MultiDiffusion' if args.method == 'md' else 'Mixture-of-Diffusers'} "
                               f"blend, {plan.num_tiles} tiles {plan.tile_w}x{plan.tile_h} overlap {plan.overlap}, N=2,C=4] + "
                               + ("no VAE" if hook is None else f"tiled VAE decode (tile {args.vae_tile}, fast mode, SD decoder ch=128, random weights)"),
                   "latent": [L, L], "tile": [plan.tile_w, plan.tile_h], "overlap": plan.overlap, "evals": args.evals, "vae_tile": None if hook is None else args.vae_tile,
                   "sharding": f"ONE process, {n} devices: tile-row bands + halo exchange (mdtile.Shard / ShardedBlend); VAE tiles dealt to the devices by area "
                               "(VAEHook.devices), estimator on the first device, rectangles copied to the first device inside the step"},
        "process_model": "single-process multi-device (mdtile_shard_init + VAEHook.devices)", "devices": devs, "devices_visible": visible,
        "stage_ms": None if t_blend is None else {"blend_eval": round(t_blend * 1e3, 4), "vae_decode": None if t_vae is None else round(t_vae * 1e3, 2)},
        "transport": transport, "debug_check": check, "roofline": None, "cpu_baseline": None,
        "note": "per-kernel roofline, parity legs and cpu_baseline are on the N = 1 line; this line times the single-process form of the N-device flow"}))
    shard.destroy()


def main():
    args = parse()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback path exists in the product)")
    if args.single_process and args.gpus > 1:
        if "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1:
            raise SystemExit("--single-process drives every device from ONE process: do not start it under torch.distributed.run")
        return run_single_process(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher environment: this process becomes the launcher (the bare command must not die before touching a GPU)
        raise SystemExit(self_launch(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start it as `python bench.py --gpus {args.gpus}` (bench.py spawns its ranks) or under "
                         f"torch.distributed.run --nproc-per-node {args.gpus}")
    devices_visible = torch.cuda.device_count()
    if world > 1 and devices_visible < world and not args.debug_single_device:
        # fewer GPUs than ranks (every rank sees the same count): the N-rank flow still runs, with all ranks on cuda:0 over gloo
        args.debug_single_device = True
        if rank == 0:
            print(f"[bench] {devices_visible} GPU(s) visible for {world} ranks: every rank uses cuda:0 and gloo (functional run)", file=sys.stderr)
    if args.debug_single_device:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    import torch.distributed as dist
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("gloo")      # control plane only: id broadcast, votes, barriers, max of the clocks

    import __graft_entry__ as ge
    if rank == 0:
        ge.build()
    if world > 1:
        dist.barrier()
    from hostsim import stub_host as sh   # stand-in A1111 host: drives the plugin without a webui (no arithmetic of the path; hostsim/, not oracle/)
    sh.install(dev)
    sh.set_device(dev)
    pl = sh.load_plugin()
    E = pl.engine
    from mdtile import sharding
    transport = "none"
    if world > 1:
        transport = "gloo (host-staged, functional check only)"
        if not args.debug_single_device:
            # data plane: the engine's own RCCL communicator behind the C ABI (mdtile_shard_init_rank; halo exchange = pack, grouped
            # ncclSend / ncclRecv over xGMI, fixed-order k_halo_add; estimator halos, statistics all-reduce, K / V all-gather and
            # the image gather on the same communicator).  Brought up under a seat belt; the fallback is ONE torch "nccl" group.
            if os.environ.get("MDTILE_SHARD_TORCH", "") != "1" and sharding.init_process_context_checked(rank, world, local_rank):
                transport = "rccl (engine communicator, C ABI)"
            else:
                try:      # the ONE alternative communicator: torch's RCCL backend for the same data-plane calls
                    grp = dist.new_group(backend="nccl", device_id=dev)
                    probe = torch.ones(1, device=dev)
                    dist.all_reduce(probe, group=grp)
                    torch.cuda.synchronize()
                    ok = float(probe.item()) == float(world)
                except Exception as e:      # noqa: BLE001 -- reported in the JSON line; the run continues host-staged over gloo
                    print(f"[bench] rank {rank}: torch nccl group unavailable ({e!r})", file=sys.stderr)
                    ok = False
                flag = torch.tensor([1 if ok else 0], dtype=torch.int32)
                dist.all_reduce(flag, op=dist.ReduceOp.MIN)
                if int(flag.item()) == 1:
                    sharding.set_data_group(grp)
                    transport = "rccl (torch.distributed nccl group)"
                else:
                    transport = "gloo (host-staged: neither RCCL communicator came up)"
    from hostsim import ldm_decoder as ld  # the random-weight SD-shaped decoder definition (the nn.Module the hook is attached to)
    if args.encode:
        if world != 1:
            raise SystemExit("--encode is a single-GPU companion line")
        print(json.dumps(run_encode(args, E, pl, ld, dev)))
        return

    L, N, C = args.latent, 2, 4
    method = E.METHOD_MD if args.method == "md" else E.METHOD_MOD

    # ------------------------------------------------------------------ blend state (init time, untimed)
    plan = E.Plan(L, L, args.tile, args.tile, args.overlap, args.tile_bs)
    weights = torch.zeros(1, 1, L, L, device=dev)
    tile_w = E.gaussian_weights(plan.tile_w, plan.tile_h, dev) if args.method == "mod" else None
    E.weight_map_add_grid(plan, tile_w, weights)
    rescale = E.reciprocal(weights) if args.method == "mod" else None
    ys = sorted(set(b[1] for b in plan.bboxes))
    bands = sharding.band_partition(ys, plan.tile_h, plan.cols, L, world)
    band = bands[rank]
    g = torch.Generator(device="cpu").manual_seed(0)
    x_in = torch.randn(N, C, L, L, generator=g).to(dev)
    # pre-generated model outputs for THIS rank's tiles (packed [T_local*N, C, th, tw]); seeded per tile so that any
    # sharding sees the same data
    g1 = torch.Generator(device="cpu").manual_seed(1)
    all_tiles = None
    n_local = band.tile_hi - band.tile_lo
    if world == 1:
        tile_out = torch.randn(plan.num_tiles * N, C, plan.tile_h, plan.tile_w, generator=g1).to(dev)
    else:
        full = torch.randn(plan.num_tiles * N, C, plan.tile_h, plan.tile_w, generator=g1)
        tile_out = torch.zeros(plan.num_tiles * N, C, plan.tile_h, plan.tile_w, device=dev)
        tile_out[band.tile_lo * N:band.tile_hi * N] = full[band.tile_lo * N:band.tile_hi * N].to(dev)
        del full
    x_tiles = torch.empty_like(tile_out)
    blend_out = torch.empty(N, C, L, L, device=dev)
    partial = torch.zeros(N, C, L, L, device=dev) if world > 1 else None
    kw = dict(weights=weights) if args.method == "md" else dict(tile_w=tile_w, rescale=rescale)

    # the sampler loop re-uses its buffers: both launches are marshalled once (mdtile.BlendCall / GatherRangeCall)
    gather_call = E.GatherRangeCall(plan, x_in, x_tiles, band.tile_lo, band.tile_hi)
    blend_call = E.BlendCall(plan, method, [tile_out], N, C, out=blend_out, packed=True, **kw) if world == 1 else None

    def blend_eval():
        gather_call()                                                        # K2 (this rank's tiles, packed, one launch)
        if world == 1:
            blend_call()
        elif not band.empty:
            E.blend(plan, method, [tile_out], N, C, out=partial, packed=True, partial=True,
                    tile_range=(band.tile_lo, band.tile_hi), row_range=(band.row_lo, band.row_hi), **kw)
            sharding.exchange_and_sum(partial, bands, rank)
            E.blend_finalize(plan, method, partial, weights=weights if args.method == "md" else None, out=blend_out,
                             row_range=(band.row_lo, band.row_hi))

    # ------------------------------------------------------------------ VAE state
    hook = None
    if not args.no_vae:
        dec = ld.make_decoder(0).to(dev)
        dec.original_forward = dec.forward
        hook = pl.tilevae.VAEHook(dec, args.vae_tile, is_decoder=True, fast_decoder=not args.slow_vae, fast_encoder=False, color_fix=False)
        hook.shard = (rank, world)
        hook.gather_to = 0 if world > 1 else None      # rank 0 returns the assembled image: the tile gather is part of the step
        z = torch.randn(1, 4, L, L, generator=torch.Generator(device="cpu").manual_seed(2)).to(dev)

    def step():
        for _ in range(args.evals):
            blend_eval()
        if hook is not None:
            return hook(z)

    # ------------------------------------------------------------------ timed region
    def sync_all():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    import builtins
    _print = builtins.print
    builtins.print = lambda *a, **k: None   # keep the plugin's progress chatter out of the JSON line
    try:
        for _ in range(args.warmup):
            step()
        sync_all()
        t0 = time.perf_counter()
        image = None
        for k in range(args.steps):
            image = step()
            if k + 1 < args.steps:
                image = None    # the previous step's image is not kept alive through the next one
        sync_all()
        elapsed = time.perf_counter() - t0
        if args.dump_outputs and rank == 0 and args.steps > 0:
            # what the caller of the timed path holds after its last step (rank 0 of N > 1: its own band of the blend output and
            # the assembled image); written before the untimed passes below reuse the buffers
            dump = {"blend_out" if world == 1 else f"blend_out_rows_{band.row_lo}_{band.row_hi}":
                    (blend_out if world == 1 else blend_out[:, :, band.row_lo:band.row_hi], DUMP_FULL_ELEMS)}
            if image is not None:
                dump["image"] = (image, DUMP_IMAGE_ELEMS)
            dump_outputs(args.dump_outputs, dump)
        image = None
        # per-stage split, untimed extras (same work, separate clocks)
        t_blend_eval = t_vae = None
        if args.full:
            sync_all()
            tb = time.perf_counter()
            for _ in range(args.evals):
                blend_eval()
            sync_all()
            t_blend_eval = (time.perf_counter() - tb) / args.evals
        if hook is not None and not args.no_profile_pass:
            tv = time.perf_counter()
            hook(z)
            sync_all()
            t_vae = time.perf_counter() - tv
    finally:
        builtins.print = _print
    debug_check = None
    if world > 1 and args.debug_single_device and hook is not None:
        # functional check of the N-rank flow (all ranks share cuda:0): rank 0's ASSEMBLED image (sequence-parallel estimator, tiles
        # dealt to the ranks, rectangles gathered) against the plain single-rank decode of the same latent on the same device
        img = hook(z)
        sync_all()
        if rank == 0:
            solo = pl.tilevae.VAEHook(dec, args.vae_tile, is_decoder=True, fast_decoder=not args.slow_vae, fast_encoder=False, color_fix=False)
            builtins.print = lambda *a, **k: None
            try:
                ref = solo(z)
            finally:
                builtins.print = _print
            den = ref.float().abs().max().item()
            debug_check = {"assembled_image_rel_err_vs_single_rank": float((img.float() - ref.float()).abs().max().item() / den),
                           "image_shape": list(img.shape)}
            # per tile: which rank decoded it and how far its rectangle is from the single-rank decode (a wrong tile names its owner)
            ins_, outs_ = hook.split_tiles(L, L)
            owner_ = sharding.deal_tiles(ins_, world)
            debug_check["per_tile"] = [{"tile": i, "owner": owner_[i], "in_bbox": list(ins_[i]),
                                        "rel_err": float((img[:, :, ob[2]:ob[3], ob[0]:ob[1]].float() - ref[:, :, ob[2]:ob[3], ob[0]:ob[1]].float()).abs().max().item() / den)}
                                       for i, ob in enumerate(outs_)]
            del ref
        del img
        sync_all()
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64)        # control plane (gloo)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()
    ms_per_step = elapsed / args.steps * 1e3
    value = L * L / (elapsed / args.steps)

    # ------------------------------------------------------------------ per-kernel roofline (instrumented extra pass)
    # (every rank runs it: with N > 1 the decode contains collectives -- sequence-parallel estimator -- that all ranks must enter;
    # only rank 0's figures are reported)
    roofline = roofline_blend = roofline_blend_f16 = None
    if not args.no_profile_pass:
        prof = Profile()
        s_bytes = 4
        T_local = plan.num_tiles if world == 1 else n_local
        blend_bytes = s_bytes * (T_local * N * C * plan.tile_h * plan.tile_w + N * C * L * (L if world == 1 else band.row_hi - band.row_lo)) \
            + 4 * L * (L if world == 1 else band.row_hi - band.row_lo) * (1 if args.method == "md" else 2)
        blend_extra = {}
        if world == 1:
            # 20 evaluations back to back between ONE pair of events: what the sampler loop's blend launches cost on the GPU
            # (an event pair per launch would also time the host's launch latency while the GPU sits idle); median of 5 rounds.
            def _median_round(call_list, bytes_each):
                for c in call_list[:3]:
                    c()
                rounds = []
                for _ in range(5):
                    p1 = Profile()

                    def _twenty():
                        for i in range(20):
                            call_list[i % len(call_list)]()
                    p1.wrap("blend", 20 * bytes_each, _twenty)
                    rounds.append(p1.summary()["blend"])
                rounds.sort(key=lambda r: r[2])
                return rounds[2]
            # (a) the bench's own buffers: 80 MB of tile outputs + canvas, static across evaluations -> resident in the 256 MiB
            #     Infinity Cache after the first launch ("warm"; this is the configuration the timed region runs)
            warm = _median_round([blend_call], blend_bytes)
            prof.add("blend", *warm)
            # (b) "cold": 8 rotating sets of tile outputs + canvases (8 x 76 MB = 610 MB > 256 MiB), so every launch reads its tiles
            #     from HBM -- what a sampler step sees when the UNet ran in between
            rot = []
            for i in range(8):
                t_i = torch.randn(plan.num_tiles * N, C, plan.tile_h, plan.tile_w, device=dev)
                o_i = torch.empty(N, C, L, L, device=dev)
                rot.append(E.BlendCall(plan, method, [t_i], N, C, out=o_i, packed=True, **kw))
            cold = _median_round(rot, blend_bytes)
            blend_extra["cold"] = {"avg_us": round(cold[2] / 20 * 1e6, 2), "achieved": round(cold[1] / cold[2] / 1e9, 1),
                                   "frac": round(cold[1] / cold[2] / 1e9 / HBM_PEAK_GBS, 4),
                                   "what": "8 rotating sets of tile outputs + canvases (610 MB > 256 MiB Infinity Cache): every read comes from HBM"}
            del rot
            # (b') the FLOOR beside it: a plain 16-byte-per-lane copy that moves the same number of bytes (half read, half written), cold the
            #      same way (8 rotating source / destination pairs, 20 back-to-back launches per event pair, median of 5 rounds) -- what this
            #      chip gives a single ~80 MB launch with no table hop, no tile walk, no arithmetic
            half = (blend_bytes // 2 + 4095) // 4096 * 4096
            cp = []
            for i in range(8):
                s_i = torch.randn(half // 4, device=dev)
                d_i = torch.empty(half // 4, device=dev)
                cp.append(E.StreamCopyCall(s_i, d_i))
            t_cp = time_launches(cp)
            blend_extra["copy_floor_us"] = round(t_cp * 1e6, 2)
            blend_extra["copy_floor_GBps"] = round(2 * half / t_cp / 1e9, 1)
            blend_extra["frac_of_copy_floor"] = round(t_cp / (cold[2] / 20), 4)
            blend_extra["copy_floor_what"] = (f"mdtile_stream_copy of {half} B -> {half} B (= the blend's {blend_bytes} algorithmic bytes), 8 rotating buffer pairs, timed like "
                                              "`achieved`; frac_of_copy_floor = copy time / blend time")
            del cp
            # (c) fp16 I/O (the webui's default dtype; fp32 accumulation inside the kernel): half the tile / canvas bytes
            th16 = tile_out.half()
            o16 = torch.empty(N, C, L, L, device=dev, dtype=torch.float16)
            call16 = E.BlendCall(plan, method, [th16], N, C, out=o16, packed=True, **kw)
            bytes16 = 2 * (plan.num_tiles * N * C * plan.tile_h * plan.tile_w + N * C * L * L) + 4 * L * L * (1 if args.method == "md" else 2)
            f16 = _median_round([call16], bytes16)
            blend_extra["f16"] = {"kernel": "k_blend<__half, ...>", "bound": "hbm", "achieved": round(f16[1] / f16[2] / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": round(f16[1] / f16[2] / 1e9 / HBM_PEAK_GBS, 4), "traffic": None, "avg_us": round(f16[2] / 20 * 1e6, 2),
                                  "bytes_per_launch": int(bytes16), "residency": "Infinity-Cache resident (static buffers)"}
            del th16, o16, call16
        if hook is not None:
            with Instrument(E, prof):
                _quiet(lambda: hook(z))
        agg = prof.summary()
        if "blend" in agg:
            n, work, secs = agg["blend"]
            n *= 20
            ach = work / secs / 1e9
            warm_d = {"avg_us": round(secs / n * 1e6, 2), "achieved": round(ach, 1), "frac": round(ach / HBM_PEAK_GBS, 4),
                      "what": "the bench's static buffers (80 MB): resident in the 256 MiB Infinity Cache after the first launch -- a cache-fed rate"}
            cold_d = blend_extra.pop("cold", None)
            head = cold_d or warm_d      # the HBM-fed figure is the one a sampler step sees (the UNet ran in between): it is `achieved`
            roofline_blend = {"kernel": "k_blend<float, 0, 8, 2, true>" if args.method == "md" else "k_blend<float, 1, ...>", "bound": "hbm",
                              "achieved": head["achieved"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                              "frac": head["frac"], "traffic": None, "launches": n,
                              "avg_us": head["avg_us"], "bytes_per_launch": int(work / n),
                              "timing": "median of 5 rounds of 20 back-to-back launches between one pair of HIP events",
                              "residency": "`achieved` = COLD: 8 rotating sets of tile outputs + canvases (610 MB > 256 MiB Infinity Cache), every read from HBM; "
                                           "`warm` = the static buffers of the timed region (Infinity-Cache resident)" if cold_d else warm_d["what"],
                              "warm": warm_d, **blend_extra}
            roofline_blend_f16 = roofline_blend.pop("f16", None)
        mm = {k: v for k, v in agg.items() if k.startswith("k_")}
        if mm:
            dom = max(mm, key=lambda k_: mm[k_][2])
            n, work, secs = mm[dom]
            ach = work / secs / 1e12
            bf16x3 = "bf16x3" in dom or "_rec" in dom
            peak = MFMA_BF16X3_PEAK_TFLOPS if bf16x3 else MFMA_F32_PEAK_TFLOPS
            # the 128-cout record convs are two symbols behind one dispatch (csrc/vae_conv_rec.hip: one 8-wave block per CU; vae_conv_rec2.hip:
            # two 4-wave blocks per CU on launches of few item rounds): the tag aggregates both, so the line names both and `traffic` sums both
            symbols = {"k_conv3x3_rec<2, 2, 4>": ["k_conv3x3_rec<2, 2, 4>", "k_conv3x3_rec2<2, 2, 4>"], "k_upconv_rec": ["k_upconv_rec(", "k_upconv_rec2("]}.get(dom, [dom])
            roofline = {"kernel": " + ".join(x.rstrip("(") for x in symbols), "kernel_symbols": symbols, "bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 1), "unit": "TFLOP/s",
                        "frac": round(ach / peak, 4), "traffic": None, "launches": n,
                        "mfma_path": "bf16x3 (3 bf16 MFMAs per fp32-class product; peak = 2500/3 algorithmic TFLOP/s)" if bf16x3 else "fp32 MFMA",
                        "avg_us": round(secs / n * 1e6, 1), "flops_per_launch": work / n,
                        "timing": "HIP events around every launch of this kernel symbol in one extra decode (same stream)",
                        "breakdown_s": {k: round(v[2], 4) for k, v in sorted(agg.items())},
                        "breakdown_tflops": {k: round(v[1] / v[2] / 1e12, 2) for k, v in sorted(mm.items())},
                        "breakdown_launches": {k: v[0] for k, v in sorted(mm.items())}}
        elif roofline_blend is not None:
            roofline = roofline_blend

    # HBM traffic per launch + the clock the kernel ran at, from a PREVIOUS set of rocprofv3 --pmc passes of this same command
    # (tools/gpu_pass.sh pmc -> tools/pmc_summary.py; counters cannot be read from inside the process).  The summary records the digest
    # of the libmdtile build it was taken on: a summary of another build is REJECTED (traffic stays null).
    pmc_path = os.environ.get("MDTILE_PMC_SUMMARY", "") or os.path.join(ROOT, "profiles", "pmc_hbm_summary_current.json")
    if rank == 0 and not args.no_profile_pass and pmc_path and os.path.exists(pmc_path):
        with open(pmc_path) as f:
            pmc = json.load(f)
        from mdtile import build as _mb
        running = open(_mb.STAMP).read().strip() if os.path.exists(_mb.STAMP) else ""
        same = bool(running) and pmc.get("libmdtile_digest", "") == running
        for rl in (roofline, roofline_blend):
            if rl is None:
                continue
            needles = rl.get("kernel_symbols") or [rl["kernel"].split("<*")[0].split(" (")[0]]
            needles = ["k_blend<"] if needles[0].startswith("k_blend") else needles
            hit = [v for k, v in pmc.get("kernels", {}).items() if any(nd_ in k for nd_ in needles)]
            if not hit:
                continue
            src = os.path.relpath(pmc_path, ROOT)
            if not same:
                rl["traffic_rejected"] = f"{src} was taken on libmdtile {pmc.get('libmdtile_digest', '?')[:12]}, this run is {running[:12]}: not comparable"
                continue
            nd = max(1, sum(h["dispatches"] for h in hit))
            rl["traffic"] = int(sum(h["hbm_bytes_per_launch"] * h["dispatches"] for h in hit) / nd)
            rl["traffic_unit"] = "HBM bytes per launch (rocprofv3 FETCH_SIZE x2 + WRITE_SIZE, separate passes)"
            rl["traffic_source"] = f"{src} (rocprofv3 --pmc passes of this command on libmdtile {running[:12]})"
            ck = [h for h in hit if h.get("clock_GHz") and h["clock_GHz"] <= 2.45]      # (summaries of older passes carry 3-17 "GHz" for us-scale kernels)
            if ck:
                rl["clock_GHz_measured"] = round(sum(h["clock_GHz"] * h["dispatches"] for h in ck) / max(1, sum(h["dispatches"] for h in ck)), 3)
                rl["clock_source"] = "GRBM_GUI_ACTIVE / 8 XCDs / kernel duration in the FETCH_SIZE pass; `peak` is quoted at 2.4 GHz"
                if rl.get("bound") == "mfma":
                    rl["frac_at_clock"] = round(rl["achieved"] / (rl["peak"] * rl["clock_GHz_measured"] / 2.4), 4)      # against the matrix-core peak at the clock the die granted

    # ------------------------------------------------------------------ whole-tile companion: the same step with the live-window narrowing OFF
    # (every padded tile decoded whole, as upstream does; untimed region of the headline, its own clock).  The two assembled images must be
    # the SAME numbers: the narrowing only leaves out pixels that crop_valid_region would throw away and that no kept pixel can see.
    whole = None
    if rank == 0 and world == 1 and hook is not None and not args.no_whole_tile_pass and pl.tilevae.LIVE_WINDOW and not args.slow_vae:
        builtins.print = lambda *a, **k: None
        try:
            img_live = hook(z)
            pl.tilevae.LIVE_WINDOW = False
            hook(z)                                  # warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.evals):
                blend_eval()
            img_whole = hook(z)
            torch.cuda.synchronize()
            ms_whole = (time.perf_counter() - t0) * 1e3
        finally:
            pl.tilevae.LIVE_WINDOW = True
            builtins.print = _print
        whole = {"ms_per_step": round(ms_whole, 2), "value": round(L * L / (ms_whole * 1e-3), 1), "bit_identical_image": bool(torch.equal(img_live, img_whole)),
                 "what": "same step with MDTILE_LIVE_WINDOW=0 (every padded decoder tile computed whole, like upstream) and torch.equal of the two 8K images"}
        del img_live, img_whole

    # ------------------------------------------------------------------ strict-fp32 companion: same decode on the exact-fp32 MFMA kernels
    # (untimed region of the headline; its own clock).  `parity.rel_err_vs_f32` = max |bf16x3 - f32| / max |f32| over the whole image.
    parity = value_f32 = ms_f32 = None
    if rank == 0 and world == 1 and hook is not None and not args.no_f32_pass and E.get_precision() == E.PRECISION_BF16X3:
        builtins.print = lambda *a, **k: None
        try:
            img = hook(z).float()
            E.set_precision(E.PRECISION_F32)
            hook(z)                                  # weights / workspaces of the exact kernels warm
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.evals):
                blend_eval()
            img32 = hook(z).float()
            torch.cuda.synchronize()
            ms_f32 = (time.perf_counter() - t0) * 1e3
        finally:
            E.set_precision(E.PRECISION_BF16X3)
            builtins.print = _print
        value_f32 = L * L / (ms_f32 * 1e-3)
        den = img32.abs().max().item()
        parity = {"rel_err_vs_f32": float((img - img32).abs().max().item() / den), "rms_err_vs_f32": float(((img - img32).pow(2).mean().sqrt() / den).item()),
                  "rel_l2_vs_f32": float(((img - img32).double().pow(2).sum().sqrt() / img32.double().pow(2).sum().sqrt()).item()),
                  "what": "whole 8K image of the timed configuration: default split-bf16 engine vs the engine's exact-fp32 MFMA kernels (mdtile_set_precision), same z and weights",
                  "tolerance": 1e-3}
        del img, img32

    # ------------------------------------------------------------------ parity against the ORACLE on an assembled decode (untimed)
    # BASELINE cfg3's decode: latent 512 x 512 at the bench's decoder tile (256 -> 2 x 2 tiles of all four tile shapes of the 8K decode:
    # 278x278, 256x278, 278x256, 256x256), estimator, crop and assembly = the whole result of upstream's vae_tile_forward
    # (scripts/tilevae.py:507-656).  The oracle (oracle/vae_oracle.py, pinned bit-exact to upstream) runs on this GPU through torch's
    # native fp32 conv / bmm (oracle/gpu_reference.py: an implementation independent of libmdtile.so) -- the 8K image itself would
    # take the oracle several minutes and 16 tiles' worth of resident activations.
    if rank == 0 and world == 1 and hook is not None and not args.no_oracle_pass:
        from oracle import gpu_reference as gr
        zc = torch.randn(1, 4, 512, 512, generator=torch.Generator(device="cpu").manual_seed(3))
        builtins.print = lambda *a, **k: None
        try:
            t0 = time.perf_counter()
            ref = gr.tiled_forward_gpu(dec, zc, args.vae_tile, fast=not args.slow_vae).cpu()
            t_oracle = time.perf_counter() - t0
            torch.cuda.empty_cache()
            out = hook(zc.to(dev)).float().cpu()
        finally:
            builtins.print = _print
        den = ref.abs().max().item()
        parity = parity or {"tolerance": 1e-3}
        parity.update({"rel_err_vs_oracle": float((out - ref).abs().max().item() / den),
                       "rms_err_vs_oracle": float(((out - ref).pow(2).mean().sqrt() / den).item()),
                       "rel_l2_vs_oracle": err_metrics(out, ref)[2],
                       "error_norms": "rel_err_* = max|d| / max|ref| (range-normalised), rms_err_* = rms(d) / max|ref|, rel_l2_* = ||d||_2 / ||ref||_2",
                       "oracle_what": f"assembled decode of a 512x512 latent (BASELINE cfg3) at decoder tile {args.vae_tile}, {'slow' if args.slow_vae else 'fast'} mode: "
                                      "engine (default precision) vs oracle/vae_oracle.py run on this GPU via torch fp32 conv / bmm (oracle/gpu_reference.py), "
                                      f"{t_oracle:.0f} s; the tile shapes are the four of the 8K decode; also tests/test_gpu_vae_large.py"})
        del ref, out
        # ---- the BENCHMARKED image itself against the oracle: single tiles of the 8K decode.  With every GroupNorm frozen by the
        # estimator (fast mode) a tile's pixels depend on no other tile, so the oracle can decode any one of upstream's 16 tiles of the 8K
        # latent alone (oracle/vae_oracle.py: only_tiles; the restriction equals the full sweep bit for bit, tests/test_oracle_golden.py)
        # with the statistics of its own estimator pass over the same latent.  Checked: an INTERIOR tile (278 x 278 latent px, padded on
        # all four sides -- the class the live-window narrowing changes most), a right-edge tile and the bottom-right corner tile.
        if L == 1024 and not args.slow_vae:
            from oracle import vae_oracle as vo8
            ins8, _ = vo8.split_tiles(L, L, args.vae_tile)
            cols = int(round(len(ins8) ** 0.5))
            picks = {"interior": cols + 1, "right_edge": 2 * cols - 1, "corner": len(ins8) - 1}
            builtins.print = lambda *a, **k: None
            try:
                img8 = hook(z).float()
                t0 = time.perf_counter()
                crops = gr.tiled_forward_gpu(dec, z, args.vae_tile, fast=True, only_tiles=list(picks.values()))
                t_or8 = time.perf_counter() - t0
            finally:
                builtins.print = _print
            den8 = img8.abs().max().item()
            per_tile = {}
            for (name, t), (ob, crop) in zip(picks.items(), crops):
                mine = img8[:, :, ob[2]:ob[3], ob[0]:ob[1]]
                d = (mine - crop.to(mine.device)).abs()
                per_tile[name] = {"tile": t, "latent_in_bbox": ins8[t], "image_out_bbox": ob, "rel_err": float(d.max().item() / den8),
                                  "rms_err": float((d.pow(2).mean().sqrt() / den8).item()), "rel_l2": err_metrics(mine, crop.to(mine.device))[2]}
            parity.update({"rel_err_vs_oracle_8k_interior": per_tile["interior"]["rel_err"], "rel_l2_vs_oracle_8k_interior": per_tile["interior"]["rel_l2"],
                           "rel_err_vs_oracle_8k_tiles": per_tile,
                           "oracle_8k_what": f"tiles of the TIMED 8192x8192 image (live windows {'on' if pl.tilevae.LIVE_WINDOW else 'off'}) against the oracle's decode of the same "
                                             f"tiles of the same latent with its own estimator statistics (torch fp32 on this GPU, {t_or8:.0f} s); "
                                             "errors relative to the image's absolute maximum"})
            del img8, crops

    # ------------------------------------------------------------------ parity on TRAINED-LIKE statistics (untimed)
    # Every number above is taken on default-init weights (activations ~ N(0,1), near-uniform softmax rows, no cancellation).  The
    # split-bf16 default precision has 16 significand bits per factor; its error grows with sum|a.w| / |sum a.w|.  Same cfg3 decode
    # with hostsim/ldm_decoder.py's committed "stress" recipe (conv gains 1..4, N(0,1) biases, zero-sum 3x3 filters on a third of the
    # output channels, GroupNorm gamma 0.2..3 / beta -2..2, 2 % of the residual stream x100 at mid.block_1, attention logits at
    # std 8): default precision AND the strict-fp32 engine against the oracle on this GPU.  tests/test_gpu_vae_stress.py holds the
    # same as tests (plus logit std 16 / 32, slow mode, the CPU oracle at tile 64).
    if rank == 0 and world == 1 and hook is not None and not args.no_stress_pass:
        from oracle import gpu_reference as gr
        dec_s = ld.make_decoder(0, stress=8).to(dev)
        dec_s.original_forward = dec_s.forward
        zs = torch.randn(1, 4, 512, 512, generator=torch.Generator(device="cpu").manual_seed(5))
        builtins.print = lambda *a, **k: None
        try:
            t0 = time.perf_counter()
            ref = gr.tiled_forward_gpu(dec_s, zs, args.vae_tile, fast=not args.slow_vae).cpu()
            t_oracle_s = time.perf_counter() - t0
            torch.cuda.empty_cache()
            hook_s = pl.tilevae.VAEHook(dec_s, args.vae_tile, is_decoder=True, fast_decoder=not args.slow_vae, fast_encoder=False, color_fix=False)
            out = hook_s(zs.to(dev)).float().cpu()
            try:
                E.set_precision(E.PRECISION_F32)
                out32 = hook_s(zs.to(dev)).float().cpu()
            finally:
                E.set_precision(E.PRECISION_BF16X3)
        finally:
            builtins.print = _print
        den = ref.abs().max().item()
        parity = parity or {"tolerance": 1e-3}
        parity.update({"rel_err_vs_oracle_stress": float((out - ref).abs().max().item() / den),
                       "rms_err_vs_oracle_stress": float(((out - ref).pow(2).mean().sqrt() / den).item()),
                       "rel_l2_vs_oracle_stress": err_metrics(out, ref)[2], "rel_l2_vs_oracle_stress_f32_engine": err_metrics(out32, ref)[2],
                       "rel_err_vs_oracle_stress_f32_engine": float((out32 - ref).abs().max().item() / den),
                       "stress_what": f"assembled decode of a 512x512 latent (BASELINE cfg3) at decoder tile {args.vae_tile}, {'slow' if args.slow_vae else 'fast'} mode, of the "
                                      "trained-like 'stress' decoder (hostsim/ldm_decoder.py: apply_stress): default precision and the strict-fp32 engine vs the oracle on "
                                      f"torch fp32 on this GPU ({t_oracle_s:.0f} s); output range {den:.2f}; bar 2e-4",
                       "stress_recipe": getattr(dec_s, "stress_info", None)})
        del ref, out, out32, hook_s, dec_s
        torch.cuda.empty_cache()

    # ------------------------------------------------------------------ the other configurations of SURVEY 8(d), untimed for the headline
    companions = None
    if rank == 0 and world == 1 and hook is not None and not args.no_companions and not args.slow_vae and L == 1024 and E.get_precision() == E.PRECISION_BF16X3:
        try:
            companions = run_companions(args, E, pl, ld, dev, dec, z, t_blend_eval)
        except Exception as e:      # noqa: BLE001 -- a companion figure must never cost the headline line
            companions = {"error": repr(e)}
            torch.cuda.empty_cache()

    # ------------------------------------------------------------------ CPU baseline (oracle = port of the reference), rank 0, N=1
    cpu_baseline = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        from oracle import blend_oracle as bo, vae_oracle as vo
        cores = os.cpu_count() or 1
        o = bo.BlendOracle(args.method, L, L, args.tile, args.tile, args.overlap, args.tile_bs)
        xc = x_in.cpu()
        pre = [t.cpu() for t in torch.split(tile_out, [len(b) * N for b in plan.batches])]
        it = iter(())

        def replay(_x):
            return next(it)

        # eager-torch sliced adds do not scale to hundreds of threads (the full pool is ~1000x slower than 8 threads on a
        # 256-core host): time a few pool sizes, report the fastest and the thread count it used
        best_blend = None
        for nt in sorted({min(cores, 8), min(cores, 32), cores}):
            torch.set_num_threads(nt)
            ts = []
            for _ in range(3):
                it = iter(pre)
                t0 = time.perf_counter()
                o.evaluate(xc, replay)
                ts.append(time.perf_counter() - t0)
                if ts[-1] > 5.0:
                    break
            med = sorted(ts)[len(ts) // 2]
            if best_blend is None or med < best_blend[0]:
                best_blend = (med, nt)
        cpu_blend, blend_threads = best_blend
        sample = f"blend: median of <=3 full {L}x{L} evaluations on {blend_threads} threads (best of 8/32/{cores})"
        cpu_val = L * L / (args.evals * cpu_blend)
        if hook is not None:
            # bounded sample: ONE tiled decode of a 64x88 latent at decoder tile 64 (the reference's own non-CUDA default,
            # tilevae.py:98) = 2 padded tiles; timed at two thread counts, the faster one is reported (a 256-thread pool
            # is slower than 32 threads on these small per-tile convs)
            ch, cw = 64, args.cpu_vae_latent
            dcpu = ld.make_decoder(0)
            zc = torch.randn(1, 4, ch, cw, generator=torch.Generator().manual_seed(2))
            best = None
            for nt in sorted({min(cores, 32), cores}):
                torch.set_num_threads(nt)
                t0 = time.perf_counter()
                vo.tiled_forward(dcpu, zc, 64, fast=not args.slow_vae)
                dt = time.perf_counter() - t0
                if best is None or dt < best[0]:
                    best = (dt, nt)
            cpu_vae, vae_threads = best
            per_px = args.evals * cpu_blend / (L * L) + cpu_vae / (ch * cw)
            cpu_val = 1.0 / per_px
            sample += (f"; VAE: one tiled decode of a {cw}x{ch} latent at decoder tile 64 (the reference's CPU default), "
                       f"{cpu_vae:.1f} s on {vae_threads} threads; rates combined per latent px")
        cpu_baseline = {"value": round(cpu_val, 1), "unit": "latent-px/s", "cores": max(blend_threads, vae_threads if hook is not None else 0), "host_cores": cores, "kind": "port", "sample": sample,
                        "blend_eval_ms": round(cpu_blend * 1e3, 2)}

    if rank == 0:
        out = {
            "metric": "latent-px/sec tile-blend+VAE-decode, 8K image", "value": round(value, 1), "unit": "latent-px/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f32" if E.get_precision() == E.PRECISION_F32 else "bf16x3+f32", "data": "synthetic",
            "config": {"workload": f"{'SDXL ' if L == 1024 else ''}{8 * L}x{8 * L} (latent {L}x{L}): {args.evals} x [tile gather + {'MultiDiffusion' if args.method == 'md' else 'Mixture-of-Diffusers'} "
                                   f"blend, {plan.num_tiles} tiles {plan.tile_w}x{plan.tile_h} overlap {plan.overlap}, N=2,C=4] + "
                                   + ("no VAE" if hook is None else f"tiled VAE decode (tile {args.vae_tile}, {'slow' if args.slow_vae else 'fast'} mode, SD decoder ch=128, random weights)"),
                       "latent": [L, L], "tile": [plan.tile_w, plan.tile_h], "overlap": plan.overlap, "evals": args.evals,
                       "vae_tile": None if hook is None else args.vae_tile,
                       "vae_live_window": None if hook is None else bool(pl.tilevae.LIVE_WINDOW and not args.slow_vae),   # padded border the remaining convs cannot carry into the valid rectangle is not computed (same pixels, bit for bit)
                       "sharding": "none" if world == 1 else f"tile-row bands x{world} + halo exchange; VAE tiles round-robin, estimator split by rows, image gathered to rank 0 inside the step"},
            "full": args.full,
            "stage_ms": None if t_blend_eval is None else {"blend_eval": round(t_blend_eval * 1e3, 4), "vae_decode": None if t_vae is None else round(t_vae * 1e3, 2)},
            "stage_px_per_s": None if t_blend_eval is None else {"blend_eval": round(L * L / t_blend_eval, 1), "vae_decode": None if t_vae is None else round(L * L / t_vae, 1)},
            "whole_tiles": whole,
            "value_f32": None if value_f32 is None else round(value_f32, 1), "ms_per_step_f32": None if ms_f32 is None else round(ms_f32, 2),
            "parity": parity,
            "roofline": roofline, "roofline_blend": roofline_blend, "roofline_blend_f16": roofline_blend_f16, "cpu_baseline": cpu_baseline,
            "companions": companions,
            "transport": transport, "debug_check": debug_check,
            "launcher": os.environ.get("MDTILE_BENCH_LAUNCHER", "torch.distributed.run" if world > 1 else "none (one process, one device)"),
            "process_model": "one process per GPU" if world > 1 else "single process", "devices_visible": devices_visible,
        }
        print(json.dumps(out))
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
