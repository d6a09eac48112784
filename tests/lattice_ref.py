"""Operands on a lattice where every fp32 partial sum of a split-bf16 conv is exact, and the exact expected value of such a conv.

The kernels split x = hi + lo with hi = bf16_rn(x), lo = bf16_rn(x - hi) and accumulate hi*hi + hi*lo + lo*hi in fp32, in an order
of the hardware's choosing.  On the lattice
    hi in +-{1, 1.25, 1.5, 1.75} (or a subset),   lo = j * 2^-10, |j| <= 3   (|j| <= 1 where lo points towards zero from |hi| = 1)
|lo| < 2^-8 = half a bf16 ulp in [1, 2) -- and below 2^-9, half an ulp in [0.5, 1), where |x| < 1 -- so hi and lo are exactly what the
splitter produces (tests/test_lattice_host.py checks it against the numpy model), every product is a multiple of a grain g
and, while  sum |terms| + |bias| + |residual| < 2^24 g  holds for every output element, every partial sum in every order is a multiple
of g below 2^24 g: an fp32 number.  The kernel's result is then one bit pattern, the exact value of the expression, and torch.equal
against an fp64 evaluation is the whole test.  The condition is ASSERTED on the actual tensors (assert_exact_in_fp32), never assumed.

Hi sets by K = taps * cin (worst case per product: |ah bh| + |ah bl| + |al bh| <= H_x H_w + (H_x + H_w) * 3 * 2^-10):
    K <= 1152   +-{1, 1.25, 1.5, 1.75} on both operands    g = 2^-12    1152 * 3.0728 = 3540 < 4096
    K <= 2304   +-{1, 1.5} on both                          g = 2^-11    2304 * 2.2588 = 5205 < 8192
    K <= 4608   +-1 on x, +-{1, 1.5} on w                   g = 2^-11    4608 * 1.5074 = 6946 < 8192
(bias and residual together add less than 9).  The exact-fp32 kernels also form lo*lo, a multiple of 2^-20 with the full lo set: with
hi = +-1 and j in {-2, 0, 2} the grain is 2^-18 and K <= 36 (conv_in) fits: 36 * (1 + 2^-9)^2 + 9 < 64.  Nothing larger does, so those
kernels get the second class at every other K: small integers (lo = 0), exact in every precision mode.

The sub-pixel upsample kernels do not multiply the nine taps: they merge the taps that land on one input pixel into one weight (fp32
sum at pack time, 1, 2 or 4 taps) and split THAT.  Role "w_up" gives the nine taps of one (cout, cin) pair a common sign, so a merged
weight is hi = sum of the taps' hi (<= 7, a bf16 number) and lo = sum of their lo (<= 12 * 2^-10, below half a bf16 ulp of that hi):
still on a lattice of the same grain, and equal to what nearest-2x + 3x3 on the taps' own halves gives.  expected_conv models the merge;
tests/test_lattice_host.py checks that the two forms agree."""
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

TERMS = ("hh+hl+lh", "hh", "full")


class Plan(NamedTuple):
    x_hi: Tuple[float, ...]      # magnitudes of the hi half of the activation (signs are drawn)
    w_hi: Tuple[float, ...]      # ... of the weights
    js: Tuple[int, ...]          # lo = j * 2^-10
    g: float                     # grain of every term


_FULL_HI = (1.0, 1.25, 1.5, 1.75)
_FULL_J = (-3, -2, -1, 0, 1, 2, 3)


def lattice_plan(K: int, terms: str = "hh+hl+lh") -> Plan:
    """The richest hi sets for which the precondition holds at K products per output element (module docstring)."""
    assert terms in TERMS
    if terms == "full":
        if K <= 36:
            return Plan((1.0,), (1.0,), (-2, 0, 2), 2.0 ** -18)
        raise ValueError(f"no lattice keeps lo*lo exact at K = {K}: use integer_operands")
    if K <= 1152:
        return Plan(_FULL_HI, _FULL_HI, _FULL_J, 2.0 ** -12)
    if K <= 2304:
        return Plan((1.0, 1.5), (1.0, 1.5), _FULL_J, 2.0 ** -11)
    if K <= 4608:
        return Plan((1.0,), (1.0, 1.5), _FULL_J, 2.0 ** -11)
    raise ValueError(f"no lattice keeps the fp32 sums exact at K = {K}")


def _pick(values, shape, gen) -> torch.Tensor:
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(len(values), tuple(shape), generator=gen)]


def _offset(shape, g, gen) -> torch.Tensor:
    """bias / residual: a multiple of g, |v| < 4.01 (quarters plus a few grains)"""
    return torch.randint(-64, 65, tuple(shape), generator=gen).double() * 2.0 ** -4 + torch.randint(-7, 8, tuple(shape), generator=gen).double() * g


def lattice_operands(shape, K: int, seed: int, role: str, terms: str = "hh+hl+lh", halves: bool = False):
    """fp32 tensor of `shape` on the lattice of lattice_plan(K, terms).  role: "x" (activation), "w" (weights, OIHW), "w_up" (weights of a
    sub-pixel upsample conv: one sign per (cout, cin) pair), "bias", "residual".  halves=True: (x, hi, lo) as constructed."""
    plan = lattice_plan(K, terms)
    gen = torch.Generator().manual_seed(seed * 8 + ("x", "w", "w_up", "bias", "residual").index(role))
    if role in ("bias", "residual"):
        assert not halves
        return _offset(shape, plan.g, gen).float()
    mags = plan.x_hi if role == "x" else plan.w_hi
    sign_shape = tuple(shape[:2]) + (1,) * (len(shape) - 2) if role == "w_up" else tuple(shape)
    hi = _pick(mags, shape, gen) * _pick((-1.0, 1.0), sign_shape, gen)
    j = _pick(plan.js, shape, gen)
    if terms != "full":
        # below 1 a bf16 ulp halves: 1 - 3 * 2^-10 rounds to 1 - 2^-8 and 1 - 2 * 2^-10 is a tie.  Where lo points towards zero from
        # |hi| = 1, keep |j| = 1 (the exact-fp32 kernels never split, their plan needs no such care)
        toward_zero = (hi.abs() == 1.0) & (j * hi.sign() < -1)
        j = torch.where(toward_zero, -hi.sign(), j)
    lo = j * 2.0 ** -10
    x = (hi + lo).float()
    assert torch.equal(x.double(), hi + lo)
    return (x, hi.float(), lo.float()) if halves else x


def integer_operands(shape, seed: int, role: str) -> torch.Tensor:
    """The second class: small integers in [-4, 4] (lo = 0, grain 1), exact in every precision mode."""
    gen = torch.Generator().manual_seed(seed * 8 + 5 + ("x", "w", "w_up", "bias", "residual").index(role))
    return torch.randint(-4, 5, tuple(shape), generator=gen).float()


def split(t: torch.Tensor):
    """(hi, lo) of an fp32 tensor as the kernels' splitter forms them, in fp64 (tests/test_split_bf16_model.py::split is the numpy model)."""
    t = t.detach().float()
    hi = t.to(torch.bfloat16).float()
    lo = (t - hi).to(torch.bfloat16).float()
    return hi.double(), lo.double()


def expected_split(y: torch.Tensor) -> torch.Tensor:
    """hi + lo of an fp32 tensor: what a raw record image of y reads back as."""
    hi, lo = split(y)
    out = (hi + lo).float()
    assert torch.equal(out.double(), hi + lo)
    return out


_UP_TAPS = {(0, 0): (0, 1), (0, 1): (1, 3), (1, 0): (0, 2), (1, 1): (2, 3)}      # (output parity, merged tap) -> [lo, hi) over the 3x3 index


def merged_up_weights(w: torch.Tensor, a: int, b: int) -> torch.Tensor:
    """The 2x2 weights of output parity (row a, column b) of nearest-2x + 3x3: fp32 sums, in (dy, dx) order, of the taps that read the
    same input pixel (the packers' k_upconv_pack_bf16x3)."""
    w = w.detach().float()
    wm = torch.zeros(w.shape[0], w.shape[1], 2, 2)
    for u in (0, 1):
        for v in (0, 1):
            for dy in range(*_UP_TAPS[(a, u)]):
                for dx in range(*_UP_TAPS[(b, v)]):
                    wm[:, :, u, v] = wm[:, :, u, v] + w[:, :, dy, dx]
    return wm


def _halves(t, terms, absval):
    """the (left, right) factor choices of one operand as fp64 tensors: [hi, lo] or, for "full", [t]"""
    parts = [t.detach().double()] if terms == "full" else list(split(t))
    return [p.abs() for p in parts] if absval else parts


_TERM_IDX = {"full": [(0, 0)], "hh": [(0, 0)], "hh+hl+lh": [(0, 0), (0, 1), (1, 0)]}      # (x factor, w factor) of every product formed


def _products(x, w, *, terms, stride, up, k, absval=False):
    """(conv sum in fp64, list of (x factor, w factor) pairs that were multiplied).  absval: every factor by magnitude."""
    assert terms in TERMS and k in (1, 3) and stride in (1, 2) and not (up and (k != 3 or stride != 1))
    xs = _halves(x, terms, absval)
    if up and terms != "full":
        # sub-pixel form: four 2x2 convs on the input grid, weights merged then split
        B, _, H, W = x.shape
        out = torch.zeros(B, w.shape[0], 2 * H, 2 * W, dtype=torch.float64)
        pairs = []
        xp = [F.pad(p, (1, 1, 1, 1)) for p in xs]
        for a in (0, 1):
            for b in (0, 1):
                ws = _halves(merged_up_weights(w, a, b), terms, absval)
                for xi, wi in _TERM_IDX[terms]:
                    out[:, :, a::2, b::2] += F.conv2d(xp[xi][:, :, a:a + H + 1, b:b + W + 1], ws[wi])
                    pairs.append((xs[xi], ws[wi]))
        return out, pairs
    if up:
        xs = [F.interpolate(p, scale_factor=2.0, mode="nearest") for p in xs]
    ws = _halves(w, terms, absval)
    if stride == 2:      # ldm Downsample: pad right 1, bottom 1, no padding in the conv
        xs = [F.pad(p, (0, 1, 0, 1)) for p in xs]
    pairs = [(xs[xi], ws[wi]) for xi, wi in _TERM_IDX[terms]]
    out = sum(F.conv2d(a, b, stride=stride, padding=k // 2 if stride == 1 else 0) for a, b in pairs)
    return out, pairs


def _with_offsets(out, bias, residual, absval=False):
    for t, view in ((bias, (1, -1, 1, 1)), (residual, None)):
        if t is not None:
            t = t.detach().double()
            t = t.abs() if absval else t
            out = out + (t.view(view) if view else t)
    return out


def expected_conv(x, w, bias, residual, *, terms: str, stride: int = 1, up: bool = False, k: int) -> torch.Tensor:
    """Exact value of the conv the kernels compute, evaluated in fp64 on the split halves:
        "hh+hl+lh": sum (xh wh + xh wl + xl wh) + bias + residual   (MDTILE_PRECISION_BF16X3; lo*lo is not in it)
        "hh":       sum xh wh + bias + residual                     (MDTILE_PRECISION_BF16)
        "full":     sum x w + bias + residual                       (exact-fp32 kernels)
    x [B, cin, H, W], w [cout, cin, k, k] (k = 1 or 3, 'same' zero padding), bias [cout] or None, residual like the output or None.
    up: nearest-2x in front of the 3x3 conv, in the kernels' sub-pixel form (merged weights are split, not the taps).
    stride=2: ldm's Downsample (pad right 1, bottom 1, stride 2).  Returns fp32 after asserting that the cast loses nothing."""
    out, _ = _products(x, w, terms=terms, stride=stride, up=up, k=k)
    out = _with_offsets(out, bias, residual)
    y = out.float()
    assert torch.equal(y.double(), out), "expected value is not an fp32 number: the operands are off the lattice"
    return y


def _all_multiples(t: torch.Tensor, g: float) -> bool:
    q = t.double() / g
    return bool((q == q.round()).all())


def assert_exact_in_fp32(x, w, bias, residual, g: float, *, terms: str, stride: int = 1, up: bool = False, k: int) -> float:
    """The precondition, on the actual tensors: every product the kernel forms, bias and residual are multiples of g, and for every output
    element  sum |terms| + |bias| + |residual| < 2^24 g  (F.conv2d on absolute values).  Then every partial sum in any order is an fp32
    number.  Returns the largest sum / (2^24 g)."""
    _, pairs = _products(x, w, terms=terms, stride=stride, up=up, k=k)
    for a, b in pairs:
        prod = torch.unique(a).view(-1, 1) * torch.unique(b).view(1, -1)      # few distinct values on either side
        assert _all_multiples(prod, g), f"a product is no multiple of the grain {g}"
    for t in (bias, residual):
        assert t is None or _all_multiples(t, g), f"bias / residual is no multiple of the grain {g}"
    mag, _ = _products(x, w, terms=terms, stride=stride, up=up, k=k, absval=True)
    mag = _with_offsets(mag, bias, residual, absval=True)
    ratio = float(mag.max()) / (2.0 ** 24 * g)
    assert ratio < 1.0, f"sum |terms| reaches {ratio:.3f} of 2^24 g: partial sums need not be fp32 numbers"
    return ratio


def mismatch_report(got: torch.Tensor, want: torch.Tensor, g: float) -> str:
    """count of differing elements, index of the first one, its difference in units of g"""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = (got != want) | torch.isnan(got)
    n = int(bad.sum())
    if n == 0:
        return "equal"
    first = tuple(int(v) for v in bad.nonzero()[0])
    d = (float(got[first]) - float(want[first])) / g
    return f"{n} of {got.numel()} elements differ; first at {first}: got {float(got[first])!r}, want {float(want[first])!r}, difference {d:g} g (g = {g})"


# ---- the cases of tests/test_gpu_conv_lattice.py (here so that tests/test_lattice_host.py proves the instrument at the same K) -------------
# the smallest shapes that still reach every block variant and a ragged edge -- not the workload's shapes
HANDOVER_3X3 = [  # B, cin, cout, H, W (output), residual
    (1, 128, 128, 17, 45, True),       # ragged rows and columns
    (1, 64, 32, 9, 33, False),         # 64-cout block
    (1, 48, 160, 11, 33, False),       # couts padded 160 -> 256: the packing of the padded tail; cin % 32 != 0 (unpermuted K order)
    (2, 256, 128, 18, 20, True),       # batch stride
    (1, 512, 512, 8, 12, False),       # K = 4608, 4 cout blocks
]
HANDOVER_NARROW = (1, 128, 3, 10, 24, False)      # cout < 32: the exact-fp32 kernel takes it in every mode
HANDOVER_UP = [  # B, cin, cout, H, W (output), residual
    (1, 128, 128, 18, 26, False),      # from 9 x 13
    (1, 64, 64, 10, 34, True),         # 64-cout block, from 5 x 17
]
DOWN2 = [(1, 128, 128, 17, 23), (1, 128, 128, 16, 22)]      # B, cin, cout, Hin, Win: odd and even inputs
CONV_IN = [  # B, cin, cout, H, W, residual -- the fp32 few-cin kernel
    (1, 3, 128, 7, 131, False),
    (2, 4, 512, 5, 9, True),
    (1, 4, 128, 1, 1, False),
]
CONV1X1 = [  # B, cin, cout, H, W, residual
    (1, 96, 64, 17, 19, True),
    (1, 32, 160, 7, 29, False),
    (1, 160, 320, 5, 10, False),       # 5 phases
]
CONV1X1_TOKEN_MAJOR = (1, 128, 128, 13, 29, False)      # output [B, H W, cout]: the exact-fp32 kernel in every mode
CONV1X1_STREAM = [  # H W % 4 == 0, >= 2048 px, cout % 128 == 0
    (1, 64, 128, 48, 52, True),
    (2, 96, 256, 40, 52, False),
]
REC_DIRECT = [  # B, cin, cout, H, W, residual
    (1, 128, 128, 16, 32, False),      # exactly one block
    (1, 128, 128, 17, 45, True),
    (2, 256, 128, 12, 20, True),
    (1, 512, 512, 8, 12, False),
]
REC_UP = (1, 128, 128, 18, 26, False)
REC_NARROW = (1, 128, 3, 10, 24, False)
REC_WINDOW = (2, 128, 128, 12, 20, 7, 11, (0, 5), (3, 9))      # B, cin, cout, Hin, Win, h, w, y0 per image, x0 per image

KS_THREE_TERM = sorted({9 * c[1] for c in HANDOVER_3X3 + HANDOVER_UP + REC_DIRECT + [REC_UP, REC_NARROW, REC_WINDOW]} | {9 * c[1] for c in DOWN2} |
                       {c[1] for c in CONV1X1 + CONV1X1_STREAM})
KS_FP32_CHAIN = sorted({9 * c[1] for c in CONV_IN})
