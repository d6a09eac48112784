#!/usr/bin/env python3
"""Operand-rounding model of the precision modes on the CPU: where does the error of a one-MFMA-per-product mode come from,
and what does MDTILE_PRECISION_F16 keep of it?

The nets are hostsim/ldm_decoder.py's (make_decoder(seed) / make_encoder(seed), default init and the "stress" recipe), run UNTILED in fp32 on a
24 x 24 latent (decoder) / 128 x 128 image (encoder).  A scheme names an operand format per class of matrix product; the inputs AND the weights of
every conv of the class are rounded to it before an fp32 conv, and inside the attention q, k, v and the probabilities P are rounded as well:
    norm   3x3 convs whose operand is silu(GroupNorm(x)): conv1 / conv2 of every ResnetBlock, conv_out
    raw    convs that read the raw residual stream: the upsample convs, nin_shortcut, the encoder's Downsample
    attn   q / k / v / proj_out and the two contractions of the attention
conv_in is never rounded (every mode keeps it exact fp32).  Formats: none (fp32: what the three-term kernels are to 2^-16), bf16 (round to nearest
even, 8 significand bits), f16 (clamped to +-65504, round to nearest even, 11 bits).  Schemes:
    mode2  all bf16                        -- MDTILE_PRECISION_BF16 as it is
    A      norm f16, raw none, attn bf16   -- MDTILE_PRECISION_F16
    B      as A with the attention in f16
    C      norm f16, raw bf16, attn bf16
    D      f16 everywhere
Printed per scheme and net: max|y - ref| / max|ref| against the unrounded fp32 forward (and the rel-L2 error with --l2).
    python tools/precision_model.py [--seed 7] [--latent 24] [--image 128] [--schemes mode2,A,B,C,D] [--stream-scale 1] [--l2]
--stream-scale s multiplies conv_in (weights and bias) by s: 3e4 drives the residual stream past fp16's range (65504) -- scheme D degrades, scheme A
does not (the GroupNorm behind the stream is scale-free).  CPU only; a full table takes a minute or two."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from hostsim import ldm_decoder as ld  # noqa: E402

SCHEMES = {
    "mode2": dict(norm="bf16", raw="bf16", attn="bf16"),
    "A": dict(norm="f16", raw="none", attn="bf16"),
    "B": dict(norm="f16", raw="none", attn="f16"),
    "C": dict(norm="f16", raw="bf16", attn="bf16"),
    "D": dict(norm="f16", raw="f16", attn="f16"),
}
TITLES = {
    "mode2": "all bf16 (MDTILE_PRECISION_BF16)",
    "A": "A: f16 behind norm+SiLU, raw-stream convs unrounded, attention bf16 (MDTILE_PRECISION_F16)",
    "B": "B: as A, attention in f16 too",
    "C": "C: f16 behind norm+SiLU, raw-stream convs bf16 one-term",
    "D": "D: f16 everywhere",
}


def rnd(x: torch.Tensor, fmt: str) -> torch.Tensor:
    if fmt == "none":
        return x
    if fmt == "bf16":
        return x.to(torch.bfloat16).float()
    if fmt == "f16":
        return x.clamp(-65504.0, 65504.0).to(torch.float16).float()
    raise ValueError(fmt)


def conv(m, x, fmt, **kw):
    return F.conv2d(rnd(x, fmt), rnd(m.weight, fmt), m.bias, **kw)


def resblock(b, x, s):
    h = conv(b.conv1, F.silu(b.norm1(x)), s["norm"], padding=1)
    h = conv(b.conv2, F.silu(b.norm2(h)), s["norm"], padding=1)
    if b.in_channels != b.out_channels:
        x = conv(b.nin_shortcut, x, s["raw"])
    return x + h


def attn(a, x, s):
    f = s["attn"]
    h = a.norm(x)
    b, c, hh, ww = h.shape
    q = rnd(conv(a.q, h, f).reshape(b, c, hh * ww).permute(0, 2, 1), f)
    k = rnd(conv(a.k, h, f).reshape(b, c, hh * ww), f)
    v = rnd(conv(a.v, h, f).reshape(b, c, hh * ww), f)
    w_ = rnd(torch.softmax(torch.bmm(q, k) * (int(c) ** -0.5), dim=2), f)
    h = torch.bmm(v, w_.permute(0, 2, 1)).reshape(b, c, hh, ww)
    return x + conv(a.proj_out, h, f)


def decoder(net, z, s):
    h = net.conv_in(z)
    h = resblock(net.mid.block_2, attn(net.mid.attn_1, resblock(net.mid.block_1, h, s), s), s)
    for lvl in reversed(range(net.num_resolutions)):
        for blk in net.up[lvl].block:
            h = resblock(blk, h, s)
        if lvl != 0:
            h = conv(net.up[lvl].upsample.conv, F.interpolate(h, scale_factor=2.0, mode="nearest"), s["raw"], padding=1)
    return conv(net.conv_out, F.silu(net.norm_out(h)), s["norm"], padding=1)


def encoder(net, x, s):
    h = net.conv_in(x)
    for lvl in range(net.num_resolutions):
        for blk in net.down[lvl].block:
            h = resblock(blk, h, s)
        if lvl != net.num_resolutions - 1:
            h = conv(net.down[lvl].downsample.conv, F.pad(h, (0, 1, 0, 1)), s["raw"], stride=2)
    h = resblock(net.mid.block_2, attn(net.mid.attn_1, resblock(net.mid.block_1, h, s), s), s)
    return conv(net.conv_out, F.silu(net.norm_out(h)), s["norm"], padding=1)


EXACT = dict(norm="none", raw="none", attn="none")


def nets(seed: int, latent: int, image: int, stream_scale: float = 1.0, small: bool = False):
    """[(column title, forward, net, input)] for the four columns of the table."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(1, 4, latent, latent, generator=g)
    x = torch.rand(1, 3, image, image, generator=g) * 2 - 1
    out = []
    for title, make, fwd, inp in (("dec", ld.make_decoder, decoder, z), ("enc", ld.make_encoder, encoder, x)):
        for stress in (False, 8):
            net = make(seed, small=small, stress=stress)
            if stream_scale != 1.0:
                with torch.no_grad():
                    net.conv_in.weight.mul_(stream_scale)
                    net.conv_in.bias.mul_(stream_scale)
            out.append((title + (" stress" if stress else ""), fwd, net, inp))
    return out


@torch.no_grad()
def table(seed=7, latent=24, image=128, schemes=("mode2", "A", "B", "C", "D"), stream_scale=1.0, small=False):
    """{scheme: {column: (max-abs error / max|ref|, rel-L2 error, finite)}}"""
    res = {k: {} for k in schemes}
    for title, fwd, net, inp in nets(seed, latent, image, stream_scale, small):
        ref = fwd(net, inp, EXACT).double()
        assert torch.isfinite(ref).all(), f"{title}: the fp32 forward is not finite"
        for k in schemes:
            y = fwd(net, inp, SCHEMES[k]).double()
            d = y - ref
            res[k][title] = (float(d.abs().max() / ref.abs().max()), float(d.norm() / ref.norm()), bool(torch.isfinite(y).all()))
    return res


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--latent", type=int, default=24)
    ap.add_argument("--image", type=int, default=128)
    ap.add_argument("--schemes", default="mode2,A,B,C,D")
    ap.add_argument("--stream-scale", type=float, default=1.0)
    ap.add_argument("--small", action="store_true", help="the ch=32 nets of the CPU tests (same topology; seconds instead of minutes)")
    ap.add_argument("--l2", action="store_true")
    a = ap.parse_args()
    schemes = [k for k in a.schemes.split(",") if k]
    res = table(a.seed, a.latent, a.image, schemes, a.stream_scale, a.small)
    cols = list(next(iter(res.values())))
    print("| which convs get which operands | " + " | ".join(cols) + " |")
    print("|---|" + "---|" * len(cols))
    for k in schemes:
        cells = []
        for c in cols:
            e, l2, fin = res[k][c]
            cells.append((f"{e:.2e}" + (f" ({l2:.2e})" if a.l2 else "")) if fin else "not finite")
        print(f"| {TITLES[k]} | " + " | ".join(cells) + " |")
    return 0


if __name__ == "__main__":
    sys.exit(main())
