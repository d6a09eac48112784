"""Attention inputs whose softmax is exact in fp32, their expected values, and a CPU model of the flash schedule with wrong kernels.

If the live keys of a query all have exactly the same logit and every other key lies at least 160 below in the log2 domain, then
exp2(0) = 1, exp2(x <= -160) = 0 (2^-160 is below half the smallest fp32 denormal), P is 0 or 1 with P_lo = 0, the denominator is the
live-key count (a power of two) and the output is the mean of the mode's V value over the live keys: ONE bit pattern in every
accumulation order, for k_attn_bf16x3, k_attn_bf16x1, k_attn (expf, scale) and k_attn_combine (w = 1 for a part with a live key, 0 for
every other part).  The V value is v_hi + v_lo in the three-term mode, v_hi in the one-term modes, v in the exact mode.

One code scheme: a token group has a code id (16 bits, distinct within an image), channel c of a code is +-1 from bit (r mod 16) of the
id, r the rank of c among the code channels.  Key j is its code, query i is A = 4096 times the code of its target.  Two codes differ in
at least floor(code channels / 16) >= 7 channels, a gap of 2 * 7 * 4096 * scale * log2 e > 3000 in the log2 domain.

Classes (q [B, C, Tq], k [B, C, Tk], v [B, Tk, C]; V from lattice_ref.lattice_operands(K=1) with every lo made positive, see _values;
twin: the odd key's value is derived from the even key's, see _twin_values):
  selector   every key its own code, one live key per query.
  group      a code shared by n = 1, 2 or 4 keys, "spread" (members Tk // n keys apart: other 16-key steps, key tiles, 128-key blocks and
             key-range parts) or "packed" (n neighbouring keys of one 16-key step); keys left over keep a code of their own.
             selector and group take one or two SHIFT channels out of the code (q = -A * code channels, k = 1 on every real key): the
             live logit is exactly 0, which is the logit of a padded key (k = 0) -- a padded key let in ties with the live key.
  twin       keys 2m and 2m + 1 share a code, targets are even keys, tie-break channels are taken out of the code (M = tie_mag(C)):
               "lh"    q[c1] = 1 + 3 * 2^-10, q[c2] = 1; the even key has M on c1, the odd key M on c2: only Q_lo x K_hi separates them
               "hl"    q[c3] = M; the even key has 1 + 3 * 2^-10 on c3, the odd key 1: only Q_hi x K_lo separates them
               "both"  all three channels
               "ll"    q[c1] = m (1 + 3 * 2^-10), q[c2] = m, m = M / 32; the even key has m (1 + 3 * 2^-10) on c1 and 0 on c2, the odd
                       key m on c1 and 3 m 2^-10 on c2: the three terms tie (live count 2), only lo x lo separates the pair (exact mode)
             M = 2^19 at C = 128 and 2^20 above: 3 * 2^-10 * M * C^-0.5 * log2 e must pass 160 (196 at C = 128 and 512, 277 at 256).
  graded     (section "graded" below) sign codes with lattice magnitudes: P is no power of two, the one class that sees P_lo x V_hi;
             compared with an fp64 softmax under a derived bound, not bit for bit.

Preconditions, asserted on the actual tensors by ExactCase before any value is expected: (a) q, k, v equal hi + lo of the splitter,
(b) the logits of every term set a kernel forms are exact in fp32 (lattice_ref.assert_exact_in_fp32, q as a 1x1 conv's input, k as its
weights, the grain taken from the products formed), (c) per query and term set the keys within 161 of the row maximum all equal it and
their count is 1, 2, 4 or 8, (d) the expected value is an fp32 number, (e) the expectations of the term sets differ (check_discrimination).
tests/test_attn_exact_host.py proves the instrument with flash_model; tests/test_gpu_attn_exact.py runs the kernels."""
import functools
import math

import torch
import torch.nn.functional as F

import lattice_ref as lr

A = 4096.0
EPS = 3 * 2.0 ** -10
GAP = 160.0
LOG2E = 1.4426950408889634
# term sets of the logits: the three kernels' own, and the three-term kernel that lost Q_lo x K_hi ("hh+hl") or Q_hi x K_lo ("hh+lh")
TERMS = ("hh+hl+lh", "hh", "full", "hh+hl", "hh+lh")
_QK_IDX = {"hh+hl+lh": [(0, 0), (0, 1), (1, 0)], "hh": [(0, 0)], "hh+hl": [(0, 0), (0, 1)], "hh+lh": [(0, 0), (1, 0)]}      # (q half, k half)
BK = 128


def tie_mag(C: int) -> float:
    return 2.0 ** 19 if C <= 128 else 2.0 ** 20


def scale_of(C: int) -> float:
    return float(C ** -0.5)


def scale2_f32(scale: float) -> float:
    """the split-bf16 kernels' fp32 constant scale * log2(e), as they round it"""
    return float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))


def _ids(groups: torch.Tensor, b: int) -> torch.Tensor:
    return (groups * 40503 + 12345 + 7919 * b) % 65536      # odd multiplier: a bijection of 16-bit ids


def _signs(ids: torch.Tensor, n_code: int) -> torch.Tensor:
    """[n_code, len(ids)] of +-1: bit (r mod 16) of the id for the code channel of rank r"""
    r = torch.arange(n_code).view(-1, 1) % 16
    return (((ids.view(1, -1) >> r) & 1) * 2 - 1).double()


def _targets(Tq: int, n_groups: int, b: int) -> torch.Tensor:
    return (torch.arange(Tq) * 7 + 3 + 11 * b) % n_groups


def group_of_key(Tk: int, n: int, placement: str) -> torch.Tensor:
    """group id per key: G = Tk // n groups of n members, the keys left over one group each"""
    j = torch.arange(Tk)
    G = Tk // n
    if n == 1 or G == 0:
        return j
    member = j % G if placement == "spread" else j // n
    return torch.where(j < n * G, member, G + j - n * G)


def shift_channels(C: int):
    """[(channel, weight)]: the weights sum to the number of code channels and are bf16 numbers after * A"""
    return [(C // 2 + 3, float(C - 1))] if C <= 256 else [(C // 2 + 3, 256.0), (C - 6, float(C - 2 - 256))]


def twin_positions(C: int):
    """(c1, c2, c3) so that over the list a tie-break channel falls in every 64-channel slab, in both halves of a 16-channel k-step, in
    the first and the last k-step of a slab and, at the top, on the last channel"""
    out = []
    for s in range(C // 64):
        out.append((64 * s, 64 * s + 1, 64 * s + 2))             # first k-step, channels 0..7 of it
        out.append((64 * s + 61, 64 * s + 62, 64 * s + 63))      # last k-step, channels 8..15 of it
    return out


def decode_key(j: int, nkb: int, nsplit: int) -> str:
    blk = j // BK
    part = next(s for s in range(nsplit) if nkb * (s + 1) // nsplit > blk)
    return f"key {j}: block {blk}, tile {(j % BK) // 32}, step {(j % BK) // 16}, lane half {((j % 16) >> 2) & 1}, part {part}"


def _grain(pairs) -> float:
    g = 2.0 ** 40
    for a, b in pairs:
        prod = torch.unique(a).view(-1, 1) * torch.unique(b).view(1, -1)
        while not lr._all_multiples(prod, g):
            g /= 2
    return g


class ExactCase:
    """q, k, v of one case on the CPU with the preconditions asserted; logits, live keys and expected values per term set"""

    def __init__(self, name, q, k, v, check_terms=("hh+hl+lh", "hh", "full"), exact=True):
        self.name, self.q, self.k, self.v = name, q, k, v
        self.B, self.C, self.Tq = q.shape
        self.Tk = k.shape[2]
        self.scale = scale_of(self.C)
        self.nkb = (self.Tk + BK - 1) // BK
        self._qs, self._ks, self._vs = lr.split(q), lr.split(k), lr.split(v)
        for t, (hi, lo) in ((q, self._qs), (k, self._ks), (v, self._vs)):
            assert torch.equal(t.double(), hi + lo), f"{name}: an operand is not hi + lo of the splitter"              # (a)
        self.ratio, self.grain = {}, {}
        # (b): assert_exact_in_fp32 takes every value of x times every value of w for a product.  Here a product is formed within one
        # channel only (2^20 meets 1 + 3 * 2^-10, never 4096 * that), so the channels go in by sets of equal values, all with the one
        # grain of the products really formed; the sets' sums add up to the whole logit's, and it is their total that must stay below 1.
        for b in range(self.B):
            x = q[b].t().reshape(1, self.Tq, self.C, 1).permute(0, 2, 1, 3)
            w = k[b].t().reshape(self.Tk, self.C, 1, 1)
            sets = {}
            for c in range(self.C):
                sig = (tuple(torch.unique(q[b, c]).tolist()), tuple(torch.unique(k[b, c]).tolist()))
                sets.setdefault(sig, []).append(c)
            for terms in check_terms:
                g = min(_grain(lr._products(x[:, ch], w[:, ch], terms=terms, stride=1, up=False, k=1)[1]) for ch in sets.values())
                r = sum(lr.assert_exact_in_fp32(x[:, ch], w[:, ch], None, None, g, terms=terms, k=1) for ch in sets.values())
                assert r < 1.0, f"{name} [{terms}]: sum |terms| reaches {r:.3f} of 2^24 g"
                self.ratio[terms] = max(r, self.ratio.get(terms, 0.0))
                self.grain[terms] = min(g, self.grain.get(terms, g))
        self._live, self._want, self.gap, self.counts = {}, {}, {}, {}
        if exact:
            for terms in TERMS:                                                                                         # (c), (d)
                self.want(terms)

    def logits(self, terms):
        """[B, Tq, Tk] in fp64, unscaled: exact, every product of the term set is a few bits wide"""
        if terms == "full":
            return torch.bmm(self.q.double().transpose(1, 2), self.k.double())
        return sum(torch.bmm(self._qs[a].transpose(1, 2), self._ks[b]) for a, b in _QK_IDX[terms])

    def live(self, terms):
        if terms not in self._live:
            S = self.logits(terms)
            mx = S.max(dim=2, keepdim=True).values
            below = (mx - S) * (self.scale * LOG2E)
            live = S == mx
            assert torch.equal(below < GAP + 1.0, live), f"{self.name} [{terms}]: a key within {GAP + 1} of the row maximum does not equal it"
            n = live.sum(2)
            counts = sorted(int(c) for c in torch.unique(n))
            assert set(counts) <= {1, 2, 4, 8}, f"{self.name} [{terms}]: live-key counts {counts}"
            self._live[terms], self.counts[terms] = live, counts
            self.gap[terms] = float(below[~live].min()) if bool((~live).any()) else math.inf
        return self._live[terms]

    def v_of(self, terms):
        return self._vs[0] if terms == "hh" else self._vs[0] + self._vs[1]

    def want(self, terms):
        """[B, C, Tq] fp32: the mean of the term set's V value over the live keys"""
        if terms not in self._want:
            live = self.live(terms).double()
            out = (torch.bmm(live, self.v_of(terms)) / live.sum(2, keepdim=True)).transpose(1, 2).contiguous()
            y = out.float()
            assert torch.equal(y.double(), out), f"{self.name} [{terms}]: the expected value is not an fp32 number"
            self._want[terms] = y
        return self._want[terms]

    def differ(self, a, b) -> float:
        return float((self.want(a) != self.want(b)).float().mean())

    def describe(self) -> str:
        per = ", ".join(f"{t}: live {self.counts[t]} gap {self.gap[t]:.0f}" for t in TERMS if t in self.counts)
        pre = ", ".join(f"{t}: grain {self.grain[t]:g} sum/(2^24 g) {self.ratio[t]:.2e}" for t in self.ratio)
        return f"precondition {self.name} C={self.C} Tq={self.Tq} Tk={self.Tk} B={self.B}: {per}; {pre}"

    def report(self, got, terms, nsplit=1) -> str:
        return attn_mismatch_report(got, self.want(terms), self.live(terms), nsplit)

    def image(self, b):
        """the case of image b alone (same tensors, so the same expectation)"""
        return self.q[b:b + 1], self.k[b:b + 1], self.v[b:b + 1]


def attn_mismatch_report(got, want, live, nsplit=1) -> str:
    """count of differing elements, the first (b, c, query), that query's live keys decoded to 128-key block, key tile, 16-key step, lane
    half and key-range part, got / want / difference"""
    got, want = got.detach().cpu(), want.detach().cpu()
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = (got != want) | torch.isnan(got)
    n = int(bad.sum())
    if n == 0:
        return "equal"
    b, c, i = (int(x) for x in bad.nonzero()[0])
    Tk = live.shape[2]
    nkb = (Tk + BK - 1) // BK
    keys = "; ".join(decode_key(int(j), nkb, nsplit) for j in live[b, i].nonzero().flatten())
    g, w = float(got[b, c, i]), float(want[b, c, i])
    return (f"{n} of {got.numel()} elements differ; first at (b, c, query) = ({b}, {c}, {i}); live keys of that query (nsplit {nsplit}): [{keys}]; "
            f"got {g!r}, want {w!r}, difference {g - w!r}")


def _values(B, Tk, C, seed):
    """V on the K = 1 lattice with every lo made positive (j = 0 -> 1; j = 1 where hi = -1, the one place where a larger lo towards zero
    would change hi): as drawn, lo = 0 in one element of seven and the lo halves of a group cancel in one of six, which would leave (e)
    below its 90 %.  So v_lo != 0 everywhere and no mean of lo halves vanishes."""
    _, hi, lo = lr.lattice_operands((B, Tk, C), 1, seed, "x", halves=True)
    j = (lo.double() * 2.0 ** 10).abs().clamp(min=1.0)
    j = torch.where(hi == -1.0, torch.ones_like(j), j)
    v = hi.double() + j * 2.0 ** -10
    assert torch.equal(v.float().double(), v)
    return v.float()


@functools.lru_cache(maxsize=None)
def group_case(C, Tq, Tk, B=1, n=1, placement="spread", seed=0) -> ExactCase:
    """selector (n = 1) and group.  Computed once, shared, never changed."""
    shifts = shift_channels(C)
    code_ch = [c for c in range(C) if c not in {s[0] for s in shifts}]
    assert sum(w for _, w in shifts) == len(code_ch)
    gid = group_of_key(Tk, n, placement)
    n_groups = int(gid.max()) + 1
    q, k = torch.zeros(B, C, Tq, dtype=torch.float64), torch.zeros(B, C, Tk, dtype=torch.float64)
    for b in range(B):
        k[b, code_ch] = _signs(_ids(gid, b), len(code_ch))
        q[b, code_ch] = A * _signs(_ids(_targets(Tq, n_groups, b), b), len(code_ch))
        for c, w in shifts:
            k[b, c] = 1.0
            q[b, c] = -A * w
    name = "selector" if n == 1 else f"group-{n}-{placement}"
    case = ExactCase(name, q.float(), k.float(), _values(B, Tk, C, seed + C + Tk))
    print(case.describe())
    return case


def _twin_values(B, Tk, C, seed):
    """_values with the odd key of a pair derived from the even one: |hi| one lattice step on (1.75 -> 1), same sign, same lo.  No element
    of a pair's mean then equals the even key's value (drawn independently, one element in twenty would)."""
    v = _values(B, Tk, C, seed).double()
    n = Tk // 2
    hi, lo = lr.split(v[:, 0:2 * n:2].float())
    hi_o = hi.sign() * (1.0 + (hi.abs() - 0.75) % 1.0)
    v[:, 1:2 * n:2] = hi_o + torch.where(hi_o == -1.0, torch.full_like(lo, 2.0 ** -10), lo)
    assert torch.equal(v.float().double(), v)
    return v.float()


@functools.lru_cache(maxsize=None)
def twin_case(C, Tq, Tk, B=1, variant="both", pos=None, seed=0) -> ExactCase:
    c1, c2, c3 = pos if pos is not None else twin_positions(C)[0]
    used = {"both": (c1, c2, c3), "lh": (c1, c2), "hl": (c3,), "ll": (c1, c2)}[variant]
    code_ch = [c for c in range(C) if c not in used]
    M = tie_mag(C)
    j = torch.arange(Tk)
    even = (j % 2 == 0).double()
    q, k = torch.zeros(B, C, Tq, dtype=torch.float64), torch.zeros(B, C, Tk, dtype=torch.float64)
    for b in range(B):
        k[b, code_ch] = _signs(_ids(j // 2, b), len(code_ch))
        q[b, code_ch] = A * _signs(_ids(_targets(Tq, (Tk + 1) // 2, b), b), len(code_ch))
        if variant in ("both", "lh"):
            q[b, c1], q[b, c2] = 1.0 + EPS, 1.0
            k[b, c1], k[b, c2] = M * even, M * (1 - even)
        if variant in ("both", "hl"):
            q[b, c3] = M
            k[b, c3] = 1.0 + EPS * even
        if variant == "ll":
            m = M / 32
            q[b, c1], q[b, c2] = m * (1.0 + EPS), m
            k[b, c1], k[b, c2] = m * (1.0 + EPS * even), m * EPS * (1 - even)
    case = ExactCase(f"twin-{variant}@{c1},{c2},{c3}", q.float(), k.float(), _twin_values(B, Tk, C, seed + C + Tk + 1))
    print(case.describe())
    return case


def check_discrimination(case: ExactCase) -> dict:
    """(e): the lo terms are in nearly every expected value.  Returns the fractions of differing elements."""
    three = "hh+hl+lh"
    fr = {"hh": case.differ("hh", three)}
    if case.name.startswith("twin"):
        variant = case.name.split("@")[0].split("-")[1]
        if variant == "lh":
            fr["hh+hl"] = case.differ("hh+hl", three)       # without Q_lo x K_hi the twins tie
        elif variant == "hl":
            fr["hh+lh"] = case.differ("hh+lh", three)       # without Q_hi x K_lo the twins tie
        elif variant == "ll":
            fr["full"] = case.differ("full", three)         # lo x lo is all that separates them
    for terms, f in fr.items():
        assert f > 0.9, f"{case.name}: the {terms} expectation differs from the three-term one in only {f:.3f} of the elements"
    return fr


# ---- the graded class -------------------------------------------------------------------------------------------------------------------
TOL_THREE, TOL_ONE = 2.0 ** -15, 2.0 ** -7


class GradedCase(ExactCase):
    """Sign codes with magnitudes from the lattice hi set {1, 1.25, 1.5, 1.75} and lo = j 2^-10, q scaled by a power of two: one Hamming
    step is ~3 in the log2 domain, |s'| <= ~40, the three-term and one-term logits are still exact in fp32 (b) -- what is left is exp2, the
    split of P and the accumulation.  reference(terms) is an fp64 softmax on the term set with the kernel's own fp32 scale constant."""

    def __init__(self, C, T, B, seed):
        q, k = torch.zeros(B, C, T, dtype=torch.float64), torch.zeros(B, C, T, dtype=torch.float64)
        mq = lr.lattice_operands((B, C, T), C, seed, "x").double().abs()
        mk = lr.lattice_operands((B, C, T), C, seed, "w").double().abs()
        sq = 1.0 if C <= 128 else 0.5
        for b in range(B):
            k[b] = _signs(_ids(torch.arange(T), b), C) * mk[b]
            q[b] = sq * _signs(_ids(_targets(T, T, b), b), C) * mq[b]
        super().__init__("graded", q.float(), k.float(), _values(B, T, C, seed + 1), check_terms=("hh+hl+lh", "hh"), exact=False)

    def reference(self, terms):
        """(out [B, C, T] fp64, sum_j p_j |v_j| [B, C, T] fp64)"""
        S = self.logits(terms)
        if terms == "full":       # k_attn: expf((s - m) * scale) with the fp32 scale
            p = torch.softmax(S * float(torch.tensor(self.scale, dtype=torch.float32)), dim=2)
        else:
            p = torch.softmax(S * (scale2_f32(self.scale) * math.log(2.0)), dim=2)
        v = self.v_of(terms)
        return torch.bmm(p, v).transpose(1, 2), torch.bmm(p, v.abs()).transpose(1, 2)

    def s2_range(self, terms):
        S = self.logits(terms) * (self.scale * LOG2E)
        return float(S.min()), float(S.max())


@functools.lru_cache(maxsize=None)
def graded_case(C, T, B=1, seed=0) -> GradedCase:
    case = GradedCase(C, T, B, seed)
    lo, hi = case.s2_range("hh+hl+lh")
    print(f"precondition graded C={C} T={T}: s' in [{lo:.1f}, {hi:.1f}]; " + ", ".join(f"{t}: grain {case.grain[t]:g} sum/(2^24 g) {case.ratio[t]:.2e}"
                                                                                          for t in case.ratio))
    return case


# ---- CPU model of the flash schedule ----------------------------------------------------------------------------------------------------
def _bsplit(t):
    hi = t.to(torch.bfloat16).float()
    return hi, (t - hi).to(torch.bfloat16).float()


_NAT_OF_REC = [0] * 16      # V record order: element i of lane half kg holds key (i & 3) + 8 (i >> 2) + 4 kg of the 16-key step
for _kg in range(2):
    for _i in range(8):
        _NAT_OF_REC[(_i & 3) + 8 * (_i >> 2) + 4 * _kg] = 8 * _kg + _i

# wrong kernel -> (what it does, the class that catches it)
MUTANTS = {
    "drop_hl": ("K_lo x Q_hi dropped in k-step `arg`", "twin-hl"),
    "drop_lh": ("Q_lo x K_hi dropped in k-step `arg`", "twin-lh"),
    "drop_vlo": ("V_lo x P_hi dropped in 16-key step `arg` of every block", "selector"),
    "add_lolo": ("lo x lo added to both contractions", "twin-ll"),
    "lo_other_half": ("the K_lo record of k-step `arg` taken from the other lane half", "twin-hl"),
    "v_natural": ("keys of a 16-key V group in natural order, not the record order", "selector"),
    "mask_gt": ("mask bound off by one: key > Tk for key >= Tk", "selector"),
    "pad_logit0": ("padded keys of key tile `arg` let in with logit 0", "selector"),
    "no_alpha_acc": ("alpha not applied to acc_o", "selector"),
    "no_l_rescale": ("l_run not rescaled by alpha", "selector"),
    "combine_drop": ("part `arg` dropped in the combine", "selector"),
    "combine_wrong_w": ("the combine's weights taken from the next part", "selector"),
    "store_lt": ("query bound on the store off by one: q < T - 1", "selector"),
    "store_le": ("query bound on the store off by one: q <= T", "selector"),
    "drop_plo": ("V_hi x P_lo dropped", "graded"),
}


def _order(n, order, gen):
    if order == "forward":
        return list(range(n))
    if order == "reversed":
        return list(range(n - 1, -1, -1))
    assert order == "shuffled"
    return [int(x) for x in torch.randperm(n, generator=gen)]


def flash_model(q, k, v, scale, *, terms=3, nsplit=1, order="forward", mutant=None, arg=None, seed=0):
    """One image through the schedule of k_attn_bf16x3 / k_attn_bf16x1 (terms = 3 / 1) and k_attn_combine, in fp32: q [C, Tq], k [C, Tk],
    v [Tk, C] -> [C, Tq].  128-key blocks, four key tiles, running max / sum / alpha, P split to hi / lo, `nsplit` key ranges.  `order`
    ("forward", "reversed", "shuffled") is the order of the k-steps, the terms, the keys of a tile sum, the 16-key steps and the parts.
    mutant: a key of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    gen = torch.Generator().manual_seed(seed)
    C, Tq = q.shape
    Tk = k.shape[1]
    Tq128, Tk128 = (Tq + 127) // 128 * 128, (Tk + 127) // 128 * 128
    nkb = Tk128 // BK
    assert 1 <= nsplit <= nkb
    qh, ql = _bsplit(F.pad(q.float(), (0, Tq128 - Tq)))
    kh, kl = _bsplit(F.pad(k.float(), (0, Tk128 - Tk)))
    vh, vl = _bsplit(F.pad(v.float(), (0, 0, 0, Tk128 - Tk)))
    scale2 = torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    ninf = torch.tensor(-math.inf)
    parts = []
    for s in range(nsplit):
        acc = torch.zeros(C, Tq128)
        m_run, l_run = torch.full((Tq128,), -math.inf), torch.zeros(Tq128)
        for kb in range(nkb * s // nsplit, nkb * (s + 1) // nsplit):
            k0 = kb * BK
            st = torch.zeros(BK, Tq128)
            for ks in _order(C // 16, order, gen):
                ch = slice(16 * ks, 16 * ks + 16)
                Kh, Kl, Qh, Ql = kh[ch, k0:k0 + BK], kl[ch, k0:k0 + BK], qh[ch], ql[ch]
                if mutant == "lo_other_half" and ks == arg:
                    Kl = torch.cat([Kl[8:], Kl[:8]])
                prods = [(Kh, Qh)]
                if terms == 3:
                    if not (mutant == "drop_hl" and ks == arg):
                        prods.append((Kl, Qh))
                    if not (mutant == "drop_lh" and ks == arg):
                        prods.append((Kh, Ql))
                    if mutant == "add_lolo":
                        prods.append((Kl, Ql))
                for i in _order(len(prods), order, gen):
                    st = st + prods[i][0].t() @ prods[i][1]
            sv = st * scale2
            key = k0 + torch.arange(BK)
            masked = key >= (Tk + 1 if mutant == "mask_gt" else Tk)
            if mutant == "pad_logit0":
                masked = masked & ((key - k0) // 32 != arg)
            sv = torch.where(masked.view(-1, 1), ninf, sv)
            m_blk = sv.view(4, 32, Tq128).amax(1).amax(0)
            m_new = torch.maximum(m_run, m_blk)
            alpha = torch.exp2(m_run - m_new)
            p = torch.exp2(sv - m_new)
            tsum = torch.zeros(4, Tq128)
            p4 = p.view(4, 32, Tq128)
            for i in _order(32, order, gen):
                tsum = tsum + p4[:, i]
            l_run = l_run * (1.0 if mutant == "no_l_rescale" else alpha) + ((tsum[0] + tsum[1]) + (tsum[2] + tsum[3]))
            m_run = m_new
            ph, pl = _bsplit(p)
            if mutant != "no_alpha_acc":
                acc = acc * alpha
            for g in _order(8, order, gen):
                rows = slice(k0 + 16 * g, k0 + 16 * g + 16)
                Vh, Vl, Ph, Pl = vh[rows], vl[rows], ph[16 * g:16 * g + 16], pl[16 * g:16 * g + 16]
                if mutant == "v_natural":
                    Vh, Vl = Vh[_NAT_OF_REC], Vl[_NAT_OF_REC]
                prods = [(Vh, Ph)]
                if terms == 3:
                    if not (mutant == "drop_vlo" and g == arg):
                        prods.append((Vl, Ph))
                    if mutant != "drop_plo":
                        prods.append((Vh, Pl))
                    if mutant == "add_lolo":
                        prods.append((Vl, Pl))
                for i in _order(len(prods), order, gen):
                    acc = acc + prods[i][0].t() @ prods[i][1]
        parts.append((acc, m_run, l_run))
    if nsplit == 1:
        acc, _, l_run = parts[0]
        out = acc * (1.0 / l_run)
    else:
        m = functools.reduce(torch.maximum, [p_[1] for p_ in parts])
        src = (lambda s_: (s_ + 1) % nsplit) if mutant == "combine_wrong_w" else (lambda s_: s_)
        w = [torch.exp2(parts[src(s_)][1] - m) for s_ in range(nsplit)]
        den, o = torch.zeros(Tq128), torch.zeros(C, Tq128)
        for s_ in _order(nsplit, order, gen):
            if mutant == "combine_drop" and s_ == arg:
                continue
            den = den + parts[s_][2] * w[s_]
            o = o + parts[s_][0] * w[s_]
        out = o * (1.0 / den)
    # the store: rows of [C][Tq] for q < Tq; `store_le` also writes q == Tq, which is element (c + 1, 0) -- the row written last wins
    flat = torch.full((C * Tq + 1,), math.nan)
    n = Tq - 1 if mutant == "store_lt" else Tq + 1 if (mutant == "store_le" and Tq < Tq128) else Tq
    for c in range(C - 1, -1, -1):
        flat[c * Tq:c * Tq + n] = out[c, :n]
    return flat[:C * Tq].view(C, Tq).clone()


def model_case(case: ExactCase, **kw):
    """flash_model over the images of a case -> [B, C, Tq]"""
    return torch.stack([flash_model(case.q[b], case.k[b], case.v[b], case.scale, **kw) for b in range(case.B)])


# ---- case tables of tests/test_gpu_attn_exact.py (here so that the host test proves the instrument on the same constructions) -----------
T_SWEEP = (1, 31, 33, 77, 127, 128, 129, 300, 450, 1000)                      # vae_attn at C = 128
T_EDGE = {256: (33, 129, 450), 512: (1, 127, 300, 1000)}                     # the edge sizes at the wider C
QK_SHAPES = ((64, 200), (300, 1100), (1000, 130), (1000, 200), (1000, 300), (129, 1))
SPLIT_EXPECTED = {("attn", 300): 1, ("attn", 450): 3, ("attn", 1000): 4, ("qk", (1000, 200)): 2, ("qk", (1000, 300)): 3}      # at 256 CUs
GRADED_SHAPES = [(C, T) for C in (128, 512) for T in (129, 450, 1000)]
