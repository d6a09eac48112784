"""Operands on which the fp16 kernels of MDTILE_PRECISION_F16 have ONE expected bit pattern, and that pattern (tests/test_gpu_f16_exact.py).

The contract (csrc/f16_convert.h): an operand is h(v) = fp16_rn(clamp(v, +-65504)), a product h(x) h(w) is exact in fp32 (11 x 11 bits) and
the MFMA adds the products in fp32.  The lattice of lattice_ref.py already consists of fp16 numbers once it is made positive and scaled by 32
(32 |x| in [32 - 2^-5, 64) on multiples of 2^-5; weights in [1 - 2^-10, 2) on multiples of 2^-10), but the fp16 kernel forms the FULL product,
lo*lo included, and no lattice keeps that exact beyond K = 36.  So the fine bits (j 2^-10) go to ONE operand only and the other stays on the
coarse hi set: every product is again a multiple of the grain g of lattice_ref.lattice_plan(K).  Both operands also carry sub-ulp bits
r 2^-12, r in -2..2 -- a quarter or a half of an fp16 ulp in [1, 2), r = +-2 a tie -- which the conversion must round away, to nearest even:
    fine_x     activation target t = 32 (hi + j 2^-10 + r 2^-12), weights +-(hi_w + r 2^-12)
    fine_w     the mirror: j on the weights only
    integer    activation in {0, 32, 64}, integer weights: the fp16, the three-term and the one-term kernel must return one tensor
    subnormal  weights n 2^-25, |n| <= 2047 (half a subnormal fp16 ulp: odd n are ties, +-2047 rounds up to 2^-14, the smallest normal),
               activation in {0, 32, 40, 48, 56}, no bias: grain 2^-24 in units of activation / 8
Where hi == 1, j and r point away from zero (below 1 the fp16 ulp halves: 1 - 2^-11 is an fp16 number and would leave the coarse set).
The raw input is built backwards (gn_exact_ref.raw_for on exact_coeffs: fmaf(x, a, s) == t exactly, SiLU the identity on t >= 24 and at 0),
the expected value is lattice_ref.expected_conv on the ROUNDED operands h(t) / 32 and h(w), terms="full", and the precondition
(assert_exact_in_fp32) is asserted on those same tensors.  Per case the expected value must differ from the three-term and the one-term
bf16 value of the UNROUNDED operands in more than 0.9 of the elements: torch.equal then proves that the fp16 kernel ran, that it rounded to
nearest even and that every product reached the right accumulator.

What the GPU module supposes about the hardware and probes first: the fp16 MFMA's fp32 accumulation keeps every multiple of g below 2^24 g
(accumulation_probe).  The case builders are cached and shared with tests/test_f16_exact_host.py, which builds every row of every table."""
import functools
from types import SimpleNamespace

import numpy as np
import torch

import gn_exact_ref as gx
import lattice_ref as lr

F16_MAX = 65504.0
CLASSES = ("fine_x", "fine_w", "integer", "subnormal")
_RS = (-2, -1, 0, 1, 2)


# ---- the conversion --------------------------------------------------------------------------------------------------------------------------
def h(t: torch.Tensor) -> torch.Tensor:
    """cvt2h of csrc/f16_convert.h, widened again: clamp to +-65504, round to nearest even to fp16 (subnormals kept)."""
    return t.detach().float().clamp(-F16_MAX, F16_MAX).to(torch.float16).float()


def h_integer_model(t: torch.Tensor) -> torch.Tensor:
    """The same contract in integer arithmetic on the fp32 bit patterns -- no float16 cast of torch or numpy takes part.  Finite inputs."""
    bits = t.detach().float().contiguous().numpy().view(np.uint32).astype(np.int64)
    sign = np.where(bits >> 31 != 0, -1.0, 1.0)
    mag = np.minimum(bits & 0x7FFFFFFF, 0x477FE000)                  # clamp |t| to 65504 = 0x477FE000 (order of the bits = order of the values)
    e, m = mag >> 23, mag & 0x7FFFFF
    sig = np.where(e > 0, m | 0x800000, m)                           # |t| = sig 2^(ee - 150)
    ee = np.maximum(e, 1)
    normal = ee >= 113                                               # |t| >= 2^-14: fp16 ulp 2^(ee - 137); below: 2^-24
    shift = np.minimum(np.where(normal, 13, 126 - ee), 40)
    q, rem, half = sig >> shift, sig & ((np.int64(1) << shift) - 1), np.int64(1) << (shift - 1)
    q = q + ((rem > half) | ((rem == half) & (q & 1 == 1)))          # to nearest, ties to even
    val = sign * np.ldexp(q.astype(np.float64), np.where(normal, ee - 137, -24).astype(np.int64))
    out = torch.from_numpy(val.astype(np.float32)).view(t.shape)
    assert torch.equal(out.double(), torch.from_numpy(val).view(t.shape))
    return out


def ulp16(t: torch.Tensor) -> torch.Tensor:
    """spacing of fp16 at |t| (fp64): 2^(e - 10) for 2^e <= |t| < 2^(e + 1), 2^-24 below 2^-14"""
    _, e = torch.frexp(t.detach().double().abs().clamp_min(2.0 ** -14))
    return torch.ldexp(torch.ones(t.shape, dtype=torch.float64), e - 11)


def ties(t: torch.Tensor) -> torch.Tensor:
    """mask of the values exactly half way between two fp16 numbers (inside the range)"""
    t64 = t.detach().double()
    return ((h(t).double() - t64).abs() == ulp16(t) / 2.0) & (t64.abs() < F16_MAX)


def h_mutants(t: torch.Tensor):
    """wrong conversions a tolerance of half an ulp (plus a little) lets through, as fp32 tensors (Inf where the mutant makes one)"""
    t = t.detach().float()
    c = t.clamp(-F16_MAX, F16_MAX)
    u = ulp16(c)
    down = (torch.floor(c.double().abs() / u) * u * torch.sign(c.double())).float()                         # truncation
    away = ((torch.floor(c.double().abs() / u + 0.5)) * u * torch.sign(c.double())).float()                 # round half away from zero
    noclamp = t.to(torch.float16).float()                                                                   # conversion before the clamp: Inf from 65520 on
    short = t.clamp(-65472.0, 65472.0).to(torch.float16).float()                                            # a saturate one fp16 step short
    flushed = torch.where(h(t).abs() < 2.0 ** -14, torch.zeros_like(t), h(t))                               # subnormal results flushed
    return {"truncation": down, "round-half-away": away, "conversion before the clamp": noclamp, "wrong saturate": short, "subnormals flushed": flushed}


# ---- operands --------------------------------------------------------------------------------------------------------------------------------
def fine_operand(shape, mags, seed: int, slot: int, fine: bool, signed: bool) -> torch.Tensor:
    """fp32 tensor of +-(hi + j 2^-10 + r 2^-12): hi from `mags`, j in -3..3 (0 unless `fine`), r in -2..2; away from zero where hi == 1."""
    gen = torch.Generator().manual_seed(seed * 16 + slot)
    hi = lr._pick(mags, shape, gen)
    j = lr._pick(lr._FULL_J, shape, gen) if fine else torch.zeros(tuple(shape), dtype=torch.float64)
    r = lr._pick(_RS, shape, gen)
    at_one = hi == 1.0
    j = torch.where(at_one, j.abs(), j)
    r = torch.where(at_one & (j == 0), r.abs(), r)
    v = hi + j * 2.0 ** -10 + r * 2.0 ** -12
    if signed:
        v = v * lr._pick((-1.0, 1.0), shape, gen)
    out = v.float()
    assert torch.equal(out.double(), v) and float(out.abs().min()) >= 1.0 and float(out.abs().max()) < 2.0
    return out


def _other_arithmetic(x, w, bias, res, terms):
    """fp32-rounded value of another arithmetic on the same (unrounded) operands -- need not be exact, so no assertion on the cast"""
    out, _ = lr._products(x, w, terms=terms, stride=1, up=False, k=3)
    return lr._with_offsets(out, bias, res).float()


def record_output(y: torch.Tensor, gy: float, seed: int, grains: bool = True):
    """Coefficients of an activated record output on the exact conv value y (grain gy), on the pattern of gn_exact_ref.rec_act_case:
    a_c in {1, 2} 2^-m with 2 2^-m max|y| <= 448, s_c = 512 + 8 (c % 16) + f_c (+ a few grains of a gy), f_c cycling through
    {1/2, 1/4, 1/8, 1/16, 1/32, 0}: the half-ulp positions of the binades [1024, 2048) ... [64, 128) that t = a y + s lands in, so ties occur.
    Asserted: t is a multiple of its grain below 2^24 grains (the fma is exact) and t >= 32 (SiLU the identity).  The expected record is h(t)."""
    B, cout = y.shape[:2]
    top = float(y.abs().max())
    m = int(np.ceil(np.log2(max(top, 1e-30) / 224.0)))
    c = torch.arange(cout)
    a = torch.tensor([1.0, 2.0], dtype=torch.float64)[(c + torch.arange(B).view(B, 1)) % 2] * 2.0 ** -m                   # [B, cout]: neighbours differ
    frac = torch.tensor([0.5, 0.25, 0.125, 0.0625, 0.03125, 0.0], dtype=torch.float64)[c % 6].view(1, cout)
    s = 512.0 + 8.0 * (c % 16).double().view(1, cout) + frac + torch.zeros(B, cout, dtype=torch.float64)
    if grains:
        gen = torch.Generator().manual_seed(seed * 8 + 2)
        s = s + torch.randint(-7, 8, (B, cout), generator=gen).double() * a * gy
    t64 = y.double() * a.view(B, cout, 1, 1) + s.view(B, cout, 1, 1)
    gt = torch.minimum(a * gy, torch.tensor(2.0 ** -5, dtype=torch.float64)).view(B, cout, 1, 1)
    q = t64 / gt
    assert bool((q == q.round()).all()), "t is no multiple of its grain"
    assert float(t64.min()) >= 32.0 and bool((t64 < 2.0 ** 24 * gt).all()), f"t in [{float(t64.min())}, {float(t64.max())}] leaves [32, 2^24 grains)"
    t = t64.float()
    assert torch.equal(t.double(), t64)
    rec = h(t)
    changed, n_ties = float((rec != t).float().mean()), int(ties(t).sum())
    assert changed > 0.5, f"only {changed:.3f} of the record values change under h"
    assert n_ties > 0, "no tie among the record values"
    coef = torch.stack([a.float(), s.float()], dim=1).contiguous()
    assert torch.equal(coef[:, 0].double(), a) and torch.equal(coef[:, 1].double(), s)
    return SimpleNamespace(coef=coef, t=t, rec=rec, changed=changed, ties=n_ties, g=float(gt.min()))


@functools.lru_cache(maxsize=None)
def conv_case(case, cls: str):
    """One conv (B, cin, cout, H, W, residual) in one operand class: raw input x and coefficients (the activation is silu(fmaf(x, a, s)) = act),
    weights, bias, residual as the KERNEL gets them, the one expected fp32 output `want`, its grain g, and for the classes whose output can carry
    one the activated record output `out` (record_output)."""
    assert cls in CLASSES
    B, cin, cout, H, W, res = case
    seed, K = gx._seed(case) * 4 + CLASSES.index(cls), 9 * cin
    groups = 32 if cin % 32 == 0 else 16
    bias = r = None
    if cls in ("fine_x", "fine_w"):
        plan = lr.lattice_plan(K)
        g, scale = plan.g, 32.0
        unscaled = fine_operand((B, cin, H, W), plan.x_hi, seed, 0, cls == "fine_x", False)
        w = fine_operand((cout, cin, 3, 3), plan.w_hi, seed, 1, cls == "fine_w", True)
        bias = lr.lattice_operands((cout,), K, seed, "bias")
        r = lr.lattice_operands((B, cout, H, W), K, seed, "residual") if res else None
    elif cls == "integer":
        g, scale = 1.0, 32.0
        unscaled = gx.saturated_sparse((B, cin, H, W), seed) / 32.0
        w, bias = lr.integer_operands((cout, cin, 3, 3), seed, "w"), lr.integer_operands((cout,), seed, "bias")
        r = lr.integer_operands((B, cout, H, W), seed, "residual") if res else None
    else:
        g, scale = 2.0 ** -24, 8.0
        gen = torch.Generator().manual_seed(seed * 16 + 3)
        unscaled = lr._pick((0.0, 4.0, 5.0, 6.0, 7.0), (B, cin, H, W), gen).float()
        n = torch.randint(-2047, 2048, (cout, cin, 3, 3), generator=gen)
        n[0, 0, 0, 0], n[-1, -1, -1, -1] = 2047, -2047
        w = (n.double() * 2.0 ** -25).float()
        assert torch.equal(w.double(), n.double() * 2.0 ** -25) and float(w.abs().max()) < 2.0 ** -14
        assert float(h(w)[0, 0, 0, 0]) == 2.0 ** -14 and float(h(w)[-1, -1, -1, -1]) == -2.0 ** -14      # rounds up to the smallest normal
    act = unscaled * scale
    gx.assert_saturated(act)
    hx, hw = h(act) / scale, h(w)
    assert torch.equal(hx, h(unscaled))                       # the scaling by a power of two commutes with the rounding
    ratio = lr.assert_exact_in_fp32(hx, hw, bias, r, g, terms="full", k=3)
    want = lr.expected_conv(hx, hw, bias, r, terms="full", k=3) * scale
    changed = {"x": float((h(act) != act).float().mean()), "w": float((hw != w).float().mean())}
    differs = {t: float((want != _other_arithmetic(unscaled, w, bias, r, t) * scale).float().mean()) for t in ("hh+hl+lh", "hh")}
    if cls == "integer":
        assert changed == {"x": 0.0, "w": 0.0} and differs == {"hh+hl+lh": 0.0, "hh": 0.0}      # lo = 0: every arithmetic gives this tensor
    else:
        assert min(differs.values()) > 0.9, f"{case} {cls}: the expected value equals another arithmetic's too often: {differs}"
        if cls == "subnormal":
            assert changed["x"] == 0.0 and changed["w"] > 0.45
        else:
            assert changed["x"] > 0.7 and changed["w"] > 0.7, changed
            assert float(ties(act).float().mean()) > 0.3 and float(ties(w).float().mean()) > 0.3
    co = gx.exact_coeffs(B, cin, groups, seed)
    x = gx.raw_for(act, co.a, co.s)
    out = record_output(want, g * scale, seed, grains=cls != "integer") if cls != "subnormal" and cout % 128 == 0 else None
    return SimpleNamespace(x=x, act=act, h_act=h(act), co=co, w=w, h_w=hw, bias=None if bias is None else bias * scale, res=None if r is None else r * scale,
                           unscaled=unscaled, bias_u=bias, res_u=r, scale=scale, want=want, g=g * scale, ratio=ratio, changed=changed, differs=differs, out=out)


@functools.lru_cache(maxsize=None)
def both_fine_is_rejected(K: int = 1152) -> str:
    """fine bits on BOTH operands at K = 1152: lo*lo is a multiple of 2^-20 only -- the precondition must refuse it.  Returns its message."""
    plan = lr.lattice_plan(K)
    x = fine_operand((1, K // 9, 6, 6), plan.x_hi, 1, 0, True, False)
    w = fine_operand((8, K // 9, 3, 3), plan.w_hi, 1, 1, True, True)
    try:
        lr.assert_exact_in_fp32(h(x), h(w), None, None, plan.g, terms="full", k=3)
    except AssertionError as e:
        return str(e)
    raise RuntimeError("the precondition accepted fine bits on both operands")


# ---- the probe of the hardware supposition ---------------------------------------------------------------------------------------------------
PROBE_SHAPE = (1, 128, 128, 16, 32, False)


@functools.lru_cache(maxsize=None)
def accumulation_probe():
    """A conv whose per-output sum climbs, with every product positive, to about 0.9 of 2^24 g (g = 2^-12 in units of activation / 32):
    120 input channels carry 1.9375 + j 2^-10 against weights 1.75 (products 7 (1984 + j) g, odd and even multiples), 8 carry exactly 1
    against weights k 2^-12, k in 1..3: steps of one, two and three grains, which an accumulator that drops low bits near 2^24 g would lose."""
    B, cin, cout, H, W, _ = PROBE_SHAPE
    g = 2.0 ** -12
    gen = torch.Generator().manual_seed(55)
    small = torch.arange(cin) % 16 == 5
    u = 1.9375 + torch.randint(-3, 4, (B, cin, H, W), generator=gen).double() * 2.0 ** -10
    u[:, small] = 1.0
    w = torch.full((cout, cin, 3, 3), 1.75, dtype=torch.float64)
    w[:, small] = torch.randint(1, 4, (cout, int(small.sum()), 3, 3), generator=gen).double() * g
    u, w = u.float(), w.float()
    assert torch.equal(h(u), u) and torch.equal(h(w), w) and torch.equal(h(u * 32.0), u * 32.0)      # fp16 numbers already: only the accumulation is probed
    # the precondition per channel set (it multiplies every value of x with every value of w; the two sets never meet): the sum of the two
    # largest sums bounds the largest sum
    ratio = sum(lr.assert_exact_in_fp32(u[:, sel], w[:, sel], None, None, g, terms="full", k=3) for sel in (small, ~small))
    assert 0.88 <= ratio < 0.95, ratio
    want = lr.expected_conv(u, w, None, None, terms="full", k=3) * 32.0
    odd = float(((want.double() / (32.0 * g)) % 2 == 1).float().mean())
    assert odd > 0.3                                           # the last bit of a 24-bit sum is in use
    act = u * 32.0
    gx.assert_saturated(act)
    co = gx.exact_coeffs(B, cin, 32, 55)
    return SimpleNamespace(x=gx.raw_for(act, co.a, co.s), act=act, co=co, w=w, want=want, g=32.0 * g, ratio=ratio, unscaled=u)


# ---- conversion cases of the producers --------------------------------------------------------------------------------------------------------
_BELOW_65520 = float(np.nextafter(np.float32(65520.0), np.float32(0.0)))      # 65519.996: the largest fp32 that still rounds to 65504 without a clamp
CONVERSION_TABLE = [  # (group, targets, s of the group's channels): every target is 0 or >= 24 (SiLU the identity), an fp32 number
    ("exact fp16 values", (24.0, 32.0, 33.5, 48.03125, 1000.5, 2050.0, 40000.0, 65504.0), 16.0),
    ("a quarter ulp off", (32.0 + 2.0 ** -7, 48.0 - 2.0 ** -7, 1000.5 + 0.125, 1000.5 - 0.125, 3000.0 + 0.5, 3000.0 - 0.5, 50016.0 + 8.0, 50016.0 - 8.0), -16.0),
    ("ties", (40.0 + 2.0 ** -6, 40.0 + 3 * 2.0 ** -6, 1000.25, 1000.75, 2049.0, 2051.0, 40016.0, 40048.0), 8.0),      # lower neighbour even / odd, by turns
    ("ulp of 2 or more", (2049.5, 4097.0, 4099.0, 10001.25, 30000.69921875, 33333.0, 65503.0, 65487.99609375), -8.0),
    ("beyond the range", (65504.0, _BELOW_65520, 65520.0, 70000.0, 1e30, 3e38), 0.0),
    ("zero", (0.0,), 4.0),
]
CONVERSION_SHAPE = (2, 96, 5, 7)


@functools.lru_cache(maxsize=None)
def conversion_case():
    """[2, 96, 5, 7]: channel c holds the targets of group c % 6, cycling through the plane from a start that depends on c; a_c = +-2^m and
    the group's s make fmaf(x, a, s) == t exactly (asserted in fp64), so the one rounding under test is the conversion.  want = h(t)."""
    B, C, H, W = CONVERSION_SHAPE
    t = torch.zeros(CONVERSION_SHAPE, dtype=torch.float32)
    a, s = torch.zeros(B, C, dtype=torch.float64), torch.zeros(B, C, dtype=torch.float64)
    pos = torch.arange(H * W).view(H, W)
    for c in range(C):
        name, vals, s_g = CONVERSION_TABLE[c % len(CONVERSION_TABLE)]
        v = torch.tensor(vals, dtype=torch.float32)
        for b in range(B):
            t[b, c] = v[(pos + c // len(CONVERSION_TABLE) + 3 * b) % len(vals)]
            big = name == "beyond the range"
            a[b, c] = (-1.0 if (c + b) % 2 else 1.0) * 2.0 ** ((c // len(CONVERSION_TABLE)) % 2 if big else (c // len(CONVERSION_TABLE)) % 3 - 1)      # |a| >= 1 there: x stays finite
            s[b, c] = s_g * (1 + b)
    gx.assert_saturated(t)
    x64 = (t.double() - s.view(B, C, 1, 1)) / a.view(B, C, 1, 1)
    x = x64.float()
    assert torch.equal(x.double(), x64) and bool(torch.isfinite(x).all()), "the raw input is no fp32 number"
    assert torch.equal(x.double() * a.view(B, C, 1, 1) + s.view(B, C, 1, 1), t.double()), "round trip"
    small = (s != 0).view(B, C, 1, 1).expand_as(t)
    assert float((x.double() * a.view(B, C, 1, 1)).abs()[small].max()) < 2.0 ** 20      # fp64 holds these sums exactly; where s == 0 there is no sum
    want = h(t)
    beyond = t > F16_MAX
    assert int(beyond.sum()) > 0 and bool((want[beyond] == F16_MAX).all()) and bool((want[t == _BELOW_65520] == F16_MAX).all())
    assert len(torch.unique(t)) == len({v for _, vals, _ in CONVERSION_TABLE for v in vals})      # every target of the table is in the tensor
    assert torch.equal(want, h_integer_model(t))
    coef = torch.stack([a.float(), s.float()], dim=1).contiguous()
    return SimpleNamespace(x=x, t=t, coef=coef, want=want)


@functools.lru_cache(maxsize=None)
def rec_from_case(shape):
    """32 (|lattice| + r 2^-12) through rec_from_f32(x, coef): the record must read back as h(t)"""
    B, C = shape[:2]
    seed = gx._seed(shape) + 9
    co = gx.exact_coeffs(B, C, 32, seed)
    t = fine_operand(shape, lr._FULL_HI, seed, 2, True, False) * 32.0
    gx.assert_saturated(t)
    want = h(t)
    assert float((want != t).float().mean()) > 0.7 and float(ties(t).float().mean()) > 0.3
    return SimpleNamespace(x=gx.raw_for(t, co.a, co.s), co=co, t=t, want=want)


# ---- statistics epilogue ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rec_stats_case(case):
    """k_conv3x3_rec_f16_st: activated fp16 record in {0, 32, 64}, sparse integer weights: y = 32 x integers with |y| <= 255 grains"""
    B, cin, cout, H, W, res, up, _family = case
    assert not up
    seed, K = gx._seed(case) + 2, 9 * cin
    act = gx.saturated_sparse((B, cin, H, W), seed)
    gx.assert_saturated(act)
    assert torch.equal(h(act), act)
    co = gx.exact_coeffs(B, cin, 32, seed)
    w = gx.sparse_integer_operands((cout, cin, 3, 3), seed, "w", gx.density_for(K))
    bias = gx.sparse_integer_operands((cout,), seed, "bias")
    r = gx.sparse_integer_operands((B, cout, H, W), seed, "residual") if res else None
    ratio = lr.assert_exact_in_fp32(act / 32.0, w, bias, r, 1.0, terms="full", k=3)
    y = lr.expected_conv(act / 32.0, w, bias, r, terms="full", k=3) * 32.0
    top = gx.assert_lane_sums_exact(y, 32.0)
    var, mean = gx.expected_stats(y, 32, 32.0, f"fp16 record {case}")
    return SimpleNamespace(x=gx.raw_for(act, co.a, co.s), act=act, co=co, w=w, bias=bias * 32.0, res=None if r is None else r * 32.0, y=y, var=var, mean=mean,
                           g=32.0, ratio=ratio, top=top)


# ---- activated fp16 record output of the sub-pixel upsample convs -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def up_record_case(case):
    """(B, cin, cout, H, W (output), residual) of a sub-pixel upsample conv on a RAW lattice record: three-term arithmetic in every mode
    (lattice_ref, role "w_up"); its activated record output in mode 5 is h(a y + s) of that exact y (record_output)."""
    B, cin, cout, H, W, res = case
    assert not res
    seed, K = gx._seed(case) + 1, 9 * cin
    g = lr.lattice_plan(K).g
    x = lr.lattice_operands((B, cin, H // 2, W // 2), K, seed, "x")
    w = lr.lattice_operands((cout, cin, 3, 3), K, seed, "w_up")
    bias = lr.lattice_operands((cout,), K, seed, "bias")
    ratio = lr.assert_exact_in_fp32(x, w, bias, None, g, terms="hh+hl+lh", up=True, k=3)
    y = lr.expected_conv(x, w, bias, None, terms="hh+hl+lh", up=True, k=3)
    return SimpleNamespace(x=x, w=w, bias=bias, y=y, g=g, ratio=ratio, out=record_output(y, g, seed))


UP_WINDOW_WHOLE = lr.REC_WINDOW[:3] + (2 * lr.REC_WINDOW[3], 2 * lr.REC_WINDOW[4], False)      # the whole image the windows of lr.REC_WINDOW are cut from

# ---- case tables (shapes from lattice_ref / gn_exact_ref: the smallest that reach every block variant) -----------------------------------------
REC_CASES = lr.REC_DIRECT
NARROW_CASE = lr.REC_NARROW
HANDOVER_CASES = lr.HANDOVER_3X3                                   # the fp16 hand-over kernel takes every row (conv_bf16x3_gn_supported)
STATS_CASES = [c for c in gx.REC_STATS if not c[6]]                # the fp16 record kernels have no sub-pixel form
ALL_CONV_CASES = sorted(set(REC_CASES) | {NARROW_CASE} | set(HANDOVER_CASES))
