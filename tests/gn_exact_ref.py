"""Inputs on which every link of the GroupNorm chain has ONE expected bit pattern, and that pattern (tests/test_gpu_gn_exact.py).

Two observations carry it (tests/test_gn_exact_host.py proves both on the CPU):

1. Statistics are exact on small integers.  Above the lane every statistics route adds in fp64 (k_gn_partial, k_gn_partial_rows,
   k_conv_stats_partial, k_gn_final); only the two conv epilogues first add a lane's few values in fp32 (s1 += v; s2 = fmaf(v, v, s2)).
   If every y is an integer multiple of a power-of-two grain with |y| / grain <= 255 and a lane adds at most 256 values, every fp32
   partial stays below 2^24 grain (grain^2 for the squares) and is exact; the fp64 sums are then integers far below 2^53, exact in any
   order, and  mean = (float)(s1 / L),  var = (float)max(0, s2 / L - m m)  are single bit patterns -- up to whether the compiler contracts
   s2 / L - m m into an fma.  expected_stats evaluates both forms and REQUIRES that they round to the same fp32 in every group.

2. SiLU is the identity on a saturated set.  Every SiLU of the project is t * 1 / (1 + e^-t) (y / (1.0f + expf(-y)) in vae_norm.hip;
   t * rcp(1.0f + __expf(-t)) in the hand-over input stage, conv_rec_common.h::silu_f and act8).  For t >= SAT_MIN = 24, e^-t < 2^-34:
   1 + e^-t is 1.0f even if the exponential is several ulp off, and the result is t (given rcp(1.0f) == 1.0f, which the GPU module's
   first test probes); for t = 0 it is 0.  The lattice of lattice_ref.py made non-negative and multiplied by 32 (>= 32 - 2^-5) stays a
   lattice: a multiplication by 32 passes SiLU unchanged.  Coefficients a = +-2^m and dyadic s make fmaf(x, a, s) exact, and
   var = fl32(4^-k - 1e-6f) gives var + 1e-6f == 4^-k in fp32, so the production eps yields rstd = 2^k (given an exact sqrtf of a power
   of 4 and an exact 1.0f / 2^k: probed as well).

Every precondition is ASSERTED on the actual tensors.  The case builders below are cached and shared by the host and the GPU module: the
host module builds every row of every table, so a GPU run never meets a failed precondition."""
import functools
from fractions import Fraction
from types import SimpleNamespace

import numpy as np
import torch

import lattice_ref as lr

EPS = 1e-6                      # the production eps of every GroupNorm (mdtile.gn_apply / gn_coeffs default)
SAT_MIN = 24.0                  # from here on 1.0f + e^-t == 1.0f with room for a sloppy exponential (e^-24 = 2^-34.6; half an ulp of 1 is 2^-25)
LANE_VALUES_MAX = 256           # assert_lane_sums_exact: the most values one lane may add in fp32
PROBE_VALUES = (0.0, 32.0, 40.0, 48.0, 56.0, 32.0 + 2.0 ** -5, 63.96875, 4000.0)


# ---- operands -------------------------------------------------------------------------------------------------------------------------------
_ROLES = ("x", "w", "w_up", "bias", "residual")


def sparse_integer_operands(shape, seed: int, role: str, density: float = 0.25, offset: int = 0) -> torch.Tensor:
    """Small integers whose conv keeps |y| <= 255: x in {-1, 0, 1}; weights in {-1, 0, 1} masked to `density`; bias in [-8, 8] plus a constant
    `offset`; residual in [-8, 8].  On the pattern of lattice_ref.integer_operands (lo = 0, grain 1, exact in every precision mode)."""
    gen = torch.Generator().manual_seed(seed * 8 + 6 + _ROLES.index(role))
    if role == "x":
        return torch.randint(-1, 2, tuple(shape), generator=gen).float()
    if role in ("w", "w_up"):
        w = torch.randint(0, 2, tuple(shape), generator=gen).float() * 2.0 - 1.0
        return w * (torch.rand(tuple(shape), generator=gen) < density).float()
    return (torch.randint(-8, 9, tuple(shape), generator=gen) + (offset if role == "bias" else 0)).float()


def density_for(K: int) -> float:
    """weight density of the sparse integer class: 1/4 up to K = 1152, 1/8 above"""
    return 0.25 if K <= 1152 else 0.125


def saturated(x_lattice: torch.Tensor) -> torch.Tensor:
    """32 |x| of a lattice_ref.lattice_operands(..., role="x") tensor: on the saturated set, still a lattice (grain x 32)."""
    t = x_lattice.detach().float().abs() * 32.0
    assert float(t.min()) >= SAT_MIN
    return t


def saturated_sparse(shape, seed: int) -> torch.Tensor:
    """{0, 32, 64}: the saturated form of the integer class (32 x {0, 1, 2})"""
    gen = torch.Generator().manual_seed(seed * 8 + 3)
    return torch.randint(0, 3, tuple(shape), generator=gen).float() * 32.0


def assert_saturated(t: torch.Tensor) -> None:
    t = t.detach().double()
    assert bool(((t == 0.0) | (t >= SAT_MIN)).all()), "a value is neither 0 nor on the saturated set: SiLU is not the identity there"
    assert bool(torch.isfinite(t).all())


# ---- observation 1: statistics ------------------------------------------------------------------------------------------------------------
def assert_lane_sums_exact(y: torch.Tensor, grain: float) -> float:
    """Every element of y is a multiple of `grain` and max |y| / grain <= 255.  A lane that adds at most LANE_VALUES_MAX = 256 such values
    in fp32 then keeps  |sum v| <= 256 * 255 grain  and  sum v^2 <= 256 * 255^2 grain^2 < 2^24 grain^2:  every partial is an fp32 number.
    Lane counts actually used, as read from the kernel templates:
        hand-over ST epilogue (vae_conv_bf16x3_direct_body.h, `float s1[4], s2[4]` inside the loop over the wave's two 32-cout tiles; the
            launcher takes MT = 4 only, NROW = TH_ / WAVES_R = 8 / 4 = 2):                    NROW x 4 couts     =  8 values per sum
        record direct ST epilogue (conv_rec_common.h::epilogue_item `st1[m][q >> 2]`, vae_conv_rec_direct_body.h NROW = 4, NPX = 1):
                                                                                             NROW x NPX x 4     = 16 values per sum
        record sub-pixel ST epilogue (vae_conv_rec_upconv_body.h NROW = 2, NPX = 2):         NROW x NPX x 4     = 16 values per sum
    Returns max |y| / grain."""
    assert lr._all_multiples(y, grain), f"a value is no multiple of the grain {grain}"
    top = float(y.detach().double().abs().max()) / grain
    assert top <= 255.0, f"max |y| = {top:g} grains > 255: a lane's fp32 sum of squares may round"
    assert LANE_VALUES_MAX * 255 ** 2 < 2 ** 24
    return top


def _as_grains(y: torch.Tensor, grain: float) -> torch.Tensor:
    q = y.detach().double() / grain
    assert bool((q == q.round()).all()), f"a value is no multiple of the grain {grain}"
    return q.long()


def group_sums(y: torch.Tensor, groups: int, grain: float = 1.0, row_lo: int = 0, row_hi=None):
    """(s1, s2) per (sample, group) as lists of Python ints in units of grain / grain^2, over rows [row_lo, row_hi) of every plane."""
    B, C = y.shape[:2]
    assert C % groups == 0
    q = _as_grains(y, grain)
    if q.dim() == 4:
        q = q[:, :, row_lo:row_hi]
    else:
        assert row_lo == 0 and row_hi is None
    q = q.reshape(B * groups, -1)
    assert int(q.abs().max()) < 2 ** 20 and q.shape[1] < 2 ** 22      # int64 cannot overflow
    return [int(v) for v in q.sum(dim=1)], [int(v) for v in (q * q).sum(dim=1)], q.shape[1]


def var_mean_forms(S1: float, S2: float, L: float):
    """k_gn_final / k_gn_from_sums on fp64 sums: m = S1 / L, v = S2 / L - m m, clamped at 0 -> ((var, mean) plain, (var, mean) with the
    subtraction contracted into one fma), as numpy float32.  The fma is emulated with fractions.Fraction (one rounding of the exact value)."""
    m = S1 / L
    q = S2 / L
    plain = q - m * m
    fused = float(Fraction(q) - Fraction(m) * Fraction(m))
    return tuple((np.float32(max(v, 0.0)), np.float32(m)) for v in (plain, fused))


def assert_unambiguous(forms, what: str = ""):
    """both forms of every group round to the same fp32 -- no group may be left out"""
    for g, (plain, fused) in enumerate(forms):
        assert plain[0].tobytes() == fused[0].tobytes() and plain[1].tobytes() == fused[1].tobytes(), \
            f"{what} group {g}: var {plain[0]!r} without and {fused[0]!r} with fma contraction: pick another seed"


def stats_from_int_sums(s1, s2, L: int, grain: float = 1.0, what: str = ""):
    """(var, mean) fp32 tensors from exact integer sums in units of grain: the sums as the fp64 numbers the kernels hold, then var_mean_forms"""
    forms = []
    for a, b in zip(s1, s2):
        assert abs(a) < 2 ** 53 and b < 2 ** 53, "an fp64 sum would round"
        forms.append(var_mean_forms(float(a) * grain, float(b) * grain * grain, float(L)))
    assert_unambiguous(forms, what)
    return (torch.tensor([float(f[0][0]) for f in forms], dtype=torch.float32), torch.tensor([float(f[0][1]) for f in forms], dtype=torch.float32))


def expected_stats(y: torch.Tensor, groups: int = 32, grain: float = 1.0, what: str = ""):
    """(var, mean), each fp32 [B * groups]: get_var_mean of y as every statistics route of the project must return it, bit for bit."""
    s1, s2, L = group_sums(y, groups, grain)
    return stats_from_int_sums(s1, s2, L, grain, what)


def expected_sums(y: torch.Tensor, groups: int, row_lo: int, row_hi: int, grain: float = 1.0) -> torch.Tensor:
    """fp64 [B * groups, 2]: (sum, sum of squares) over rows [row_lo, row_hi) of every plane (mdtile.gn_sums)"""
    s1, s2, _ = group_sums(y, groups, grain, row_lo, row_hi)
    assert all(abs(a) < 2 ** 53 and b < 2 ** 53 for a, b in zip(s1, s2))
    return torch.tensor([[float(a) * grain, float(b) * grain * grain] for a, b in zip(s1, s2)], dtype=torch.float64)


# ---- observation 2: coefficients and raw inputs --------------------------------------------------------------------------------------------
def _representable(t: torch.Tensor) -> bool:
    return bool(torch.equal(t.double().float().double(), t.double()))


def _distinct_neighbours(idx: torch.Tensor, n: int) -> torch.Tensor:
    """a 1-D index tensor with idx[i] != idx[i - 1] (mod n)"""
    idx = idx.clone()
    for i in range(1, idx.numel()):
        if idx[i] == idx[i - 1]:
            idx[i] = (idx[i] + 1) % n
    return idx


def exact_coeffs(B: int, C: int, groups: int, seed: int, silu: bool = True, affine: bool = True):
    """(mean [B groups], var [B groups], gamma [C], beta [C], a [B, C], s [B, C]) as fp32 tensors with
        var = fl32(4^-k - 1e-6f), k in 0..5 distinct between neighbouring groups  ->  rstd = 2^k
        mean a multiple of 2^-4;  gamma = +-2^m (m in -1..1), or +-{1, 1.25, 1.5, 1.75} for the class without SiLU;  beta a multiple of 2^-4
    gamma and beta differ between neighbouring channels.  affine=False: gamma = beta = None (1 and 0).
    Asserted in numpy float32: var + eps == 4^-k;  a = 2^k gamma and s = -mean a + beta are fp32 numbers."""
    assert C % groups == 0
    gen = torch.Generator().manual_seed(seed * 8 + 1)
    k = _distinct_neighbours(torch.randint(0, 6, (B * groups,), generator=gen), 6)
    p4 = np.float32(4.0) ** (-k.numpy().astype(np.float32))
    var = (p4 - np.float32(EPS)).astype(np.float32)
    assert var.dtype == np.float32 and np.array_equal((var + np.float32(EPS)).astype(np.float32), p4), "var + eps is not 4^-k in fp32"
    assert np.array_equal(np.float32(1.0) / np.sqrt(p4), np.float32(2.0) ** k.numpy().astype(np.float32))
    mean = torch.randint(-32, 33, (B * groups,), generator=gen).double() * 2.0 ** -4
    mags = (0.5, 1.0, 2.0) if silu else (1.0, 1.25, 1.5, 1.75)
    cand = torch.tensor([sg * m for m in mags for sg in (1.0, -1.0)], dtype=torch.float64)      # signs alternate along the index
    if affine:
        gamma = cand[_distinct_neighbours(torch.randint(0, len(cand), (C,), generator=gen), len(cand))]
        beta = _distinct_neighbours(torch.randint(0, 65, (C,), generator=gen), 65).double() * 2.0 ** -4 - 2.0
        assert bool((gamma < 0).any()) and bool((gamma > 0).any())
    else:
        gamma, beta = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    cpg = C // groups
    rstd = (2.0 ** k.double()).view(B, groups, 1).expand(B, groups, cpg).reshape(B, C)
    mean_c = mean.view(B, groups, 1).expand(B, groups, cpg).reshape(B, C)
    a = rstd * gamma.view(1, C)
    s = -mean_c * a + beta.view(1, C)
    if affine:      # the s row differs between neighbouring channels in every sample: taking it from the neighbour must show
        for c in range(1, C):
            while bool((s[:, c] == s[:, c - 1]).any()) or beta[c] == beta[c - 1]:
                beta[c] += 2.0 ** -4
                s[:, c] = -mean_c[:, c] * a[:, c] + beta[c]
    assert _representable(a) and _representable(s), "a or s is no fp32 number"
    # the kernels' own arithmetic in numpy float32: a = rstd * gamma (one product), s = fmaf(-mean, a, beta) (the exact value, rounded once)
    a32 = (np.float32(2.0) ** k.numpy().astype(np.float32)).reshape(B, groups, 1) * gamma.numpy().astype(np.float32).reshape(1, groups, cpg)
    assert np.array_equal(a32.reshape(B, C).astype(np.float64), a.numpy())
    out = SimpleNamespace(mean=mean.float(), var=torch.from_numpy(var.copy()), gamma=gamma.float() if affine else None, beta=beta.float() if affine else None,
                          a=a.float(), s=s.float(), k=k, groups=groups)
    out.coef = torch.stack([out.a, out.s], dim=1).contiguous()      # [B, 2, C]: the layout of mdtile.gn_coeffs
    return out


def unit_coef(B: int, C: int) -> torch.Tensor:
    """[B, 2, C] with a = 1, s = 0"""
    return torch.stack([torch.ones(B, C), torch.zeros(B, C)], dim=1).contiguous()


def raw_for(target: torch.Tensor, a: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """The fp32 x [B, C, H, W] with fmaf(x, a, s) == target for per-(sample, channel) a = +-2^m and dyadic s [B, C].  The round trip is
    asserted in fp64, where a product by a power of two and a sum of small dyadic numbers are exact: the fp32 fma then returns the exact
    value, which is `target`.  A negative a makes x negative where the target is positive: a sign or absolute-value slip shows."""
    B, C = target.shape[:2]
    a64, s64 = a.double().view(B, C, 1, 1), s.double().view(B, C, 1, 1)
    m = torch.log2(a64.abs())
    assert bool((m == m.round()).all()), "a is no power of two"
    x64 = (target.double() - s64) / a64
    x = x64.float()
    assert torch.equal(x.double(), x64), "the raw input is no fp32 number"
    assert torch.equal(x.double() * a64 + s64, target.double()), "round trip"
    assert float((x.double() * a64).abs().max()) < 2.0 ** 20 and float(s64.abs().max()) < 2.0 ** 20      # fp64 holds the sum exactly
    return x


def affine_exact(x: torch.Tensor, a: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """x a + s in fp64, asserted to be an fp32 number: what fmaf(x, a, s) returns"""
    B, C = x.shape[:2]
    t = x.double() * a.double().view(B, C, 1, 1) + s.double().view(B, C, 1, 1)
    assert float(t.abs().max()) < 2.0 ** 20
    out = t.float()
    assert torch.equal(out.double(), t), "x a + s is no fp32 number"
    return out


# ---- the numpy float32 model of the three SiLU forms (the reciprocal modelled as correctly rounded) ----------------------------------------
def silu_models(t):
    t = np.asarray(t, dtype=np.float32)
    one = np.float32(1.0)
    with np.errstate(over="ignore", under="ignore"):
        e = np.exp(-t.astype(np.float64)).astype(np.float32)                                        # expf(-t), correctly rounded
        div = (t / (one + e)).astype(np.float32)                                                    # vae_norm.hip: y / (1.0f + expf(-y))
        rcp = (t * (one / (one + e)).astype(np.float32)).astype(np.float32)                         # silu_f / the hand-over input stage
        arg = (t * np.float32(-1.44269504088896340736)).astype(np.float32)
        e2 = np.exp2(arg.astype(np.float64)).astype(np.float32)                                     # act8: exp2(t * -log2(e))
        act = (t * (one / (one + e2)).astype(np.float32)).astype(np.float32)
    return {"y / (1 + expf(-y))": div, "t * rcp(1 + __expf(-t))": rcp, "act8": act}


# ---- case tables: the smallest shapes that reach every variant ------------------------------------------------------------------------------
STATS_SHAPES = [  # mdtile_gn_stats, 32 groups
    (2, 64, 9, 13),        # L = 234: odd groups start 8 bytes off -- the scalar path and the vector path in one launch
    (1, 128, 5, 7),        # aligned, no tail
    (1, 32, 5, 7),         # L = 35, one plane per group
    (1, 96, 3, 3),         # 3 channels per group, tail of 3
    (3, 32, 1, 1),         # L = 1: var exactly 0
    (1, 32, 260, 260),     # L = 67600 > 64 x 256 x 4: the grid-stride loop wraps
]
STATS_OFFSETS = (0, 1000)
BAND_SHAPE = (2, 64, 12, 10)
BANDS = [(0, 12), (0, 5), (5, 12), (3, 4)]
POOL_CASES = [  # pixel counts of the tiles: four equal tiles, (2, 1, 1) x k
    (100, 100, 100, 100),
    (2, 1, 1),
    (2 * 4096, 4096, 4096),
]
HANDOVER_STATS = [  # B, cin, cout, H, W, residual, bias offset (in grains)
    (1, 128, 128, 17, 45, True, 0),        # ragged
    (2, 256, 256, 9, 40, True, 0),         # batch, 8 couts per group
    (1, 512, 512, 8, 33, False, 0),        # 16 per group, four cout blocks
    (1, 256, 128, 11, 34, False, 100),     # mean >> std
]
REC_STATS = [  # B, cin, cout, H, W (output), residual, upsample, family (1 = one block per CU: the epilogue computes them; 0 = the launcher's choice)
    (1, 128, 128, 16, 32, False, False, 1),      # one item
    (1, 256, 256, 19, 45, True, False, 1),
    (2, 128, 128, 10, 40, True, False, 1),
    (1, 512, 512, 9, 33, False, False, 1),
    (1, 128, 128, 18, 26, False, True, 1),       # sub-pixel
    (2, 256, 256, 14, 70, False, True, 1),       # ragged input tiles, both row parities
    (1, 256, 256, 19, 45, True, False, 0),       # the launcher takes the statistics pass
]
ROUTES_CASE = REC_STATS[1]
APPLY_SHAPES = [
    (2, 64, 9, 13),        # planes with plane * HW % 4 != 0 take the scalar path, the others the vector path plus tail
    (1, 128, 8, 8),
    (1, 32, 1, 3),
    (1, 32, 260, 260),     # a plane larger than the 64-block grid
]
APPLY_CLASSES = ("affine", "plain", "silu")      # lattice x with gamma in +-{1 .. 1.75}; gamma = beta = None; raw_for(saturated lattice) with SiLU
FUSED_CASES = lr.HANDOVER_3X3
REC_ACT_CASES = [(c, False) for c in lr.REC_DIRECT] + [(lr.REC_UP, True)]
REC_ACT_S0 = 1024.0      # see rec_act_case
COEFF_PROBES = [(B, C, groups, affine, silu) for B, C, groups, affine in ((2, 64, 32, True), (1, 512, 32, True), (1, 48, 16, True), (2, 128, 32, False))
                for silu in (True, False)]      # B, C, groups, with gamma and beta, gamma = +-2^m (else +-{1 .. 1.75})
REC_FROM_SHAPES = [(2, 64, 9, 13), (1, 128, 17, 45), (1, 32, 1, 3)]


def _seed(case) -> int:
    return sum(int(v) * (i + 1) for i, v in enumerate(case[:5]))


@functools.lru_cache(maxsize=None)
def stats_case(shape, offset: int):
    """integers in [-40, 40] + offset (no fp32 lane sums on this route: only the fp64 sums must be exact) and their (var, mean)"""
    gen = torch.Generator().manual_seed(_seed(shape) + offset)
    x = (torch.randint(-40, 41, tuple(shape), generator=gen) + offset).float()
    var, mean = expected_stats(x, 32, 1.0, f"stats {shape} +{offset}")
    return SimpleNamespace(x=x, var=var, mean=mean)


@functools.lru_cache(maxsize=None)
def handover_stats_case(case):
    """item 5: raw input whose activation is the sparse saturated set, sparse integer weights: y = 32 x integers"""
    B, cin, cout, H, W, res, boff = case
    seed, K = _seed(case), 9 * cin
    act = saturated_sparse((B, cin, H, W), seed)
    assert_saturated(act)
    co = exact_coeffs(B, cin, 32, seed)
    x = raw_for(act, co.a, co.s)
    w = sparse_integer_operands((cout, cin, 3, 3), seed, "w", density_for(K))
    bias = sparse_integer_operands((cout,), seed, "bias", offset=boff)
    r = sparse_integer_operands((B, cout, H, W), seed, "residual") if res else None
    ratio = lr.assert_exact_in_fp32(act / 32.0, w, bias, r, 1.0, terms="full", k=3)
    y = lr.expected_conv(act / 32.0, w, bias, r, terms="full", k=3) * 32.0
    top = assert_lane_sums_exact(y, 32.0)
    var, mean = expected_stats(y, 32, 32.0, f"hand-over {case}")
    return SimpleNamespace(x=x, act=act, co=co, w=w, bias=bias * 32.0, res=None if r is None else r * 32.0, y=y, var=var, mean=mean, g=32.0, ratio=ratio, top=top)


@functools.lru_cache(maxsize=None)
def rec_stats_case(case):
    """item 6: raw record input of sparse integers"""
    B, cin, cout, H, W, res, up, _family = case
    seed, K = _seed(case) + int(up), 9 * cin
    hin, win = (H // 2, W // 2) if up else (H, W)
    x = sparse_integer_operands((B, cin, hin, win), seed, "x")
    w = sparse_integer_operands((cout, cin, 3, 3), seed, "w", density_for(K))
    bias = sparse_integer_operands((cout,), seed, "bias")
    r = sparse_integer_operands((B, cout, H, W), seed, "residual") if res else None
    ratio = lr.assert_exact_in_fp32(x, w, bias, r, 1.0, terms="full", up=up, k=3)
    y = lr.expected_conv(x, w, bias, r, terms="full", up=up, k=3)
    assert torch.equal(y, lr.expected_conv(x, w, bias, r, terms="hh", up=up, k=3))      # lo = 0: every mode computes the same value
    top = assert_lane_sums_exact(y, 1.0)
    var, mean = expected_stats(y, 32, 1.0, f"record {case}")
    return SimpleNamespace(x=x, w=w, bias=bias, res=r, y=y, var=var, mean=mean, g=1.0, ratio=ratio, top=top, up=up)


@functools.lru_cache(maxsize=None)
def apply_case(shape, cls: str):
    """item 7: (x, coefficients, expected output) of one class of APPLY_CLASSES"""
    B, C, H, W = shape
    seed = _seed(shape) + APPLY_CLASSES.index(cls)
    lat = lr.lattice_operands(shape, 1152, seed, "x")
    co = exact_coeffs(B, C, 32, seed, silu=cls == "silu", affine=cls != "plain")
    if cls == "silu":
        want = saturated(lat)
        assert_saturated(want)
        x = raw_for(want, co.a, co.s)
    else:
        x = lat
        want = affine_exact(x, co.a, co.s)
    return SimpleNamespace(x=x, co=co, want=want, g=2.0 ** -16)


@functools.lru_cache(maxsize=None)
def unsaturated_case():
    """item 7's one tolerance class: lattice x, exact t = a x + s with |t| <= 16, SiLU of that t in fp64"""
    shape = (2, 64, 9, 13)
    B, C = shape[:2]
    x = lr.lattice_operands(shape, 1152, 77, "x")
    co = exact_coeffs(B, C, 32, 77, silu=True)
    # shrink the coefficients by powers of two until |t| <= 16: they stay exact
    scale = 2.0 ** -4
    a, s = co.a * scale, co.s * scale
    t = affine_exact(x, a, s)
    assert float(t.abs().max()) <= 16.0 and float(t.abs().max()) > 4.0 and bool((t < 0).any())
    mean, var = co.mean, co.var                     # a = 2^k gamma: put the scale into gamma and beta
    gamma, beta = co.gamma * scale, co.beta * scale
    assert torch.equal((co.s.double() * scale).float().double(), co.s.double() * scale)
    t64 = t.double()
    want = t64 / (1.0 + torch.exp(-t64))
    return SimpleNamespace(x=x, mean=mean, var=var, gamma=gamma, beta=beta, a=a, s=s, t=t, want=want)


@functools.lru_cache(maxsize=None)
def fused_case(case, cls: str):
    """item 8: activation 32 |lattice x| (or {0, 32, 64}), bias and residual x 32: expected 32 x the conv of the unscaled operands"""
    B, cin, cout, H, W, res = case
    seed, K = _seed(case), 9 * cin
    groups = 32 if cin % 32 == 0 else 16
    if cls == "lattice":
        g = lr.lattice_plan(K).g
        unscaled = lr.lattice_operands((B, cin, H, W), K, seed, "x").abs()
        act = saturated(unscaled)
        w = lr.lattice_operands((cout, cin, 3, 3), K, seed, "w")
        bias = lr.lattice_operands((cout,), K, seed, "bias")
        r = lr.lattice_operands((B, cout, H, W), K, seed, "residual") if res else None
        pre_terms = "hh+hl+lh"
    else:
        g = 1.0
        act = saturated_sparse((B, cin, H, W), seed)
        unscaled = act / 32.0
        w, bias = lr.integer_operands((cout, cin, 3, 3), seed, "w"), lr.integer_operands((cout,), seed, "bias")
        r = lr.integer_operands((B, cout, H, W), seed, "residual") if res else None
        pre_terms = "full"
    assert_saturated(act)
    ratio = lr.assert_exact_in_fp32(unscaled, w, bias, r, g, terms=pre_terms, k=3)
    co = exact_coeffs(B, cin, groups, seed)
    x = raw_for(act, co.a, co.s)
    want = {t: lr.expected_conv(unscaled, w, bias, r, terms=t, k=3) * 32.0 for t in ("hh+hl+lh", "hh")}
    if cls == "lattice":
        assert (want["hh+hl+lh"] != want["hh"]).float().mean() > 0.9
    return SimpleNamespace(x=x, act=act, co=co, w=w, bias=bias * 32.0, res=None if r is None else r * 32.0, want=want, g=32.0 * g, ratio=ratio)


@functools.lru_cache(maxsize=None)
def rec_act_case(case, up: bool):
    """item 9: a lattice record conv whose record output is activated with a_c in {0.5, 1, 2}, s_c = REC_ACT_S0 + 8 (c % 16) + a few grains.
    On the expected y (per mode): t = a y + s is a multiple of the grain of t and SAT_MIN <= 32 <= t < 2^24 grains, so the fma is exact and
    SiLU the identity: the record output is split(t).  REC_ACT_S0 = 1024: with 512 a y of -350 under a = 2 (K = 4608) would leave the
    saturated set; the larger shift asks the same of the kernel."""
    B, cin, cout, H, W, res = case
    seed, K = _seed(case) + int(up), 9 * cin
    g = lr.lattice_plan(K).g
    hin, win = (H // 2, W // 2) if up else (H, W)
    x = lr.lattice_operands((B, cin, hin, win), K, seed, "x")
    w = lr.lattice_operands((cout, cin, 3, 3), K, seed, "w_up" if up else "w")
    bias = lr.lattice_operands((cout,), K, seed, "bias")
    r = lr.lattice_operands((B, cout, H, W), K, seed, "residual") if res else None
    ratio = lr.assert_exact_in_fp32(x, w, bias, r, g, terms="hh+hl+lh", up=up, k=3)
    gen = torch.Generator().manual_seed(seed * 8 + 2)
    c = torch.arange(cout)
    a = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[(c + torch.arange(B).view(B, 1)) % 3]                        # [B, cout]: neighbours differ
    s = REC_ACT_S0 + 8.0 * (c % 16).double().view(1, cout) + torch.randint(-7, 8, (B, cout), generator=gen).double() * g
    gt = g / 2.0                                                                                                        # a = 0.5 halves the grain
    y, t, rec = {}, {}, {}
    for terms in ("hh+hl+lh", "hh"):
        y[terms] = lr.expected_conv(x, w, bias, r, terms=terms, up=up, k=3)
        tt = y[terms].double() * a.view(B, cout, 1, 1) + s.view(B, cout, 1, 1)
        assert lr._all_multiples(tt, gt), "t is no multiple of its grain"
        assert float(tt.min()) >= 32.0 and float(tt.max()) < 2.0 ** 24 * gt, f"t in [{float(tt.min())}, {float(tt.max())}] leaves [32, 2^24 grains)"
        t[terms] = tt.float()
        assert torch.equal(t[terms].double(), tt)
        rec[terms] = lr.expected_split(t[terms])
    assert (rec["hh+hl+lh"] != t["hh+hl+lh"]).float().mean() > 0.5      # 16 bits of a 24-bit t: the split is not the identity here
    coef = torch.stack([a.float(), s.float()], dim=1).contiguous()
    assert torch.equal(coef[:, 1].double(), s)
    return SimpleNamespace(x=x, w=w, bias=bias, res=r, coef=coef, y=y, t=t, rec=rec, g=g, gt=gt, ratio=ratio)


@functools.lru_cache(maxsize=None)
def coeff_probe(B: int, C: int, groups: int, affine: bool, silu: bool):
    """item 1's second probe: one set of exact coefficients"""
    return exact_coeffs(B, C, groups, 11 + C, silu=silu, affine=affine)


@functools.lru_cache(maxsize=None)
def rec_from_case(shape):
    """item 9: raw input whose activation is 32 |lattice x|: the activated record image holds it whole (both halves survive the scaling)"""
    B, C = shape[:2]
    seed = _seed(shape) + 4
    co = exact_coeffs(B, C, 32, seed)
    want = saturated(lr.lattice_operands(shape, 1152, seed, "x"))
    assert_saturated(want)
    assert torch.equal(lr.expected_split(want), want)
    return SimpleNamespace(x=raw_for(want, co.a, co.s), co=co, want=want)


@functools.lru_cache(maxsize=None)
def routes_case():
    """item 10: the record conv's integer y of ROUTES_CASE, and operands from which the hand-over kernel computes 32 y: activation 32 (x + 1)
    in {0, 32, 64}, the same weights, 32 x the bias and a residual that takes 32 conv(ones) off again -- all integers.  (var, mean) of 32 y
    are (1024 var, 32 mean): scalings by powers of two commute with every rounding."""
    case = ROUTES_CASE
    B, cin, cout, H, W, res, up, _family = case
    assert res and not up
    c = rec_stats_case(case)
    co = exact_coeffs(B, cin, 32, 5)
    act = (c.x + 1.0) * 32.0
    assert_saturated(act)
    ones = lr.expected_conv(torch.ones_like(c.x), c.w, None, None, terms="full", k=3)
    res2 = c.res - ones
    lr.assert_exact_in_fp32(act / 32.0, c.w, c.bias, res2, 1.0, terms="full", k=3)
    assert torch.equal(lr.expected_conv(act / 32.0, c.w, c.bias, res2, terms="full", k=3), c.y)
    assert_lane_sums_exact(c.y * 32.0, 32.0)
    var32, mean32 = expected_stats(c.y * 32.0, 32, 32.0, "routes, hand-over")
    assert torch.equal(var32 / 1024.0, c.var) and torch.equal(mean32 / 32.0, c.mean)
    return SimpleNamespace(rec=c, co=co, x_hand=raw_for(act, co.a, co.s), bias_hand=c.bias * 32.0, res_hand=res2 * 32.0, y_hand=c.y * 32.0,
                           var_hand=var32, mean_hand=mean32)


def pool_case(pixels, BG: int = 64, seed: int = 9):
    """item 4: dyadic means and vars with pixel counts whose fractions are dyadic: every product and every partial sum of k_gn_pool is exact
    (in any order, with or without fma contraction), asserted in fp64."""
    T = len(pixels)
    gen = torch.Generator().manual_seed(seed + T + int(pixels[0]))
    means = torch.randint(-256, 257, (T, BG), generator=gen).double() * 2.0 ** -5
    vars_ = torch.randint(0, 1025, (T, BG), generator=gen).double() * 2.0 ** -7
    px = torch.tensor([int(p) for p in pixels], dtype=torch.float32) / max(pixels)      # the wrapper's own fp32 arithmetic (mdtile.gn_pool)
    frac = px / torch.sum(px)
    m = torch.log2(frac.double())
    assert bool((m == m.round()).all()), "a pixel fraction is no power of two"
    assert float(frac.double().sum()) == 1.0
    want_m, want_v = (means * frac.double().view(T, 1)).sum(0), (vars_ * frac.double().view(T, 1)).sum(0)
    for t in (want_m, want_v):      # multiples of 2^-7 2^-2 below 2^5: every partial sum is an fp32 number
        assert lr._all_multiples(t, 2.0 ** -12) and float(t.abs().max()) < 2.0 ** 10 and _representable(t)
    return SimpleNamespace(means=means.float(), vars=vars_.float(), pixels=tuple(int(p) for p in pixels), mean=want_m.float(), var=want_v.float())
