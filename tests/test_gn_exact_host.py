"""The instrument of tests/test_gpu_gn_exact.py, proven on the CPU before any kernel is trusted to it (tests/gn_exact_ref.py).

  * the expected statistics do not depend on the summation order: shuffled, per-block partials in the shapes of k_gn_partial and of the
    conv epilogues + k_conv_stats_partial (fp32 lane sums below, fp64 above), and a two-band split all give the same fp64 sums and the
    same fp32 (var, mean);
  * wrong statistics kernels change bits: a pixel dropped at a ragged edge, a pixel counted twice, a lane partial credited to the
    neighbouring quad, the unbiased variance, one block's sum of squares kept in fp32.  The sixth candidate, a missing clamp of
    E[x^2] - mean^2, has NO witness on this class of inputs: a negative difference needs a constant group (any spread of integers leaves
    var >= (L - 1) / L^2, ten orders above the rounding of m m), and on a constant group c L / L = c and c^2 L / L = c^2 are exact, so the
    difference is exactly 0 in both forms (test_no_input_of_this_class_needs_the_clamp): that mutant is dropped;
  * the numpy float32 model of the three SiLU forms (reciprocal correctly rounded) returns t on the saturated set and 0 at 0;
  * every precondition holds for every row of every case table -- the builders of gn_exact_ref assert lane sums, unambiguity,
    lattice_ref.assert_exact_in_fp32 and the coefficient identities, and are cached: the GPU module gets the very same objects;
  * wrong apply / fused-input / record-activation kernels change bits: coefficients of the neighbouring channel, of the neighbouring
    group, of the other half of a record, a pad pixel contributing silu(s), the lo half of the activated value dropped."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gn_exact_ref as gx
import lattice_ref as lr


def _f32_stats(S1, S2, L):
    """(var, mean) bits of fp64 sums through both forms, which must agree"""
    plain, fused = gx.var_mean_forms(float(S1), float(S2), float(L))
    assert plain[0].tobytes() == fused[0].tobytes() and plain[1].tobytes() == fused[1].tobytes()
    return plain[0].tobytes() + plain[1].tobytes()


def _group_values(y, groups, g):
    """[B groups, cpg, H, W] float64 view of group g's values"""
    B, C, H, W = y.shape
    return y.double().reshape(B * groups, C // groups, H, W)[g].numpy()


def _seq_sum_f64(values):
    s = 0.0
    for v in values:
        s += float(v)
    return s


def _lane_sums_f32(vals):
    """s1 += v; s2 = fmaf(v, v, s2) over a lane's values, in numpy float32 (v v + s2 is exact in fp64: one rounding)"""
    s1, s2 = np.float32(0.0), np.float32(0.0)
    for v in vals:
        v = np.float32(v)
        s1 = np.float32(s1 + v)
        s2 = np.float32(np.float64(v) * np.float64(v) + np.float64(s2))
    return float(s1), float(s2)


def _epilogue_sums(vg, rows_per_lane):
    """(S1, S2) of one group [cpg = 4 k, H, W] the way a conv epilogue and k_conv_stats_partial add them: a lane's rows_per_lane x 4 couts
    in fp32, everything above in fp64 (here: sequentially, in the order of the loops)"""
    cpg, H, W = vg.shape
    S1 = S2 = 0.0
    for q in range(0, cpg, 4):
        for y0 in range(0, H, rows_per_lane):
            for x in range(W):
                a, b = _lane_sums_f32(vg[q:q + 4, y0:y0 + rows_per_lane, x].reshape(-1))
                S1 += a
                S2 += b
    return S1, S2


ORDER_INPUTS = [("hand-over y", lambda: (gx.handover_stats_case(gx.HANDOVER_STATS[0]).y, 32.0)),
                ("mean >> std", lambda: (gx.handover_stats_case(gx.HANDOVER_STATS[3]).y, 32.0)),
                ("record y", lambda: (gx.rec_stats_case(gx.REC_STATS[2]).y, 1.0)),
                ("offset 1000", lambda: (gx.stats_case(gx.STATS_SHAPES[0], 1000).x, 1.0))]


@pytest.mark.parametrize("name,make", ORDER_INPUTS, ids=[n for n, _ in ORDER_INPUTS])
def test_expected_stats_do_not_depend_on_the_summation_order(name, make):
    y, grain = make()
    B, C, H, W = y.shape
    groups = 32
    want_v, want_m = gx.expected_stats(y, groups, grain)
    want_sums = gx.expected_sums(y, groups, 0, H, grain)
    rng = np.random.default_rng(5)
    for g in (0, 1, B * groups - 1):
        vg = _group_values(y, groups, g)
        flat = vg.reshape(-1)
        L = flat.size
        want_bits = np.float32(float(want_v[g])).tobytes() + np.float32(float(want_m[g])).tobytes()
        routes = {}
        routes["in order"] = (_seq_sum_f64(flat), _seq_sum_f64(flat * flat))
        p = rng.permutation(L)
        routes["shuffled"] = (_seq_sum_f64(flat[p]), _seq_sum_f64((flat * flat)[p]))
        # k_gn_partial: 64 blocks x 256 threads, thread t of block b takes elements b 256 + t + k 64 256; block tree; blocks in order
        idx = np.arange(L)
        parts = [(flat[(idx // 256) % 64 == b].sum(), (flat * flat)[(idx // 256) % 64 == b].sum()) for b in range(64)]
        routes["k_gn_partial"] = (_seq_sum_f64([a for a, _ in parts]), _seq_sum_f64([b for _, b in parts]))
        if name != "offset 1000":      # the epilogue routes: fp32 lane sums need |y| <= 255 grains
            gx.assert_lane_sums_exact(y, grain)
            routes["hand-over epilogue (2 rows x 4 couts per lane)"] = _epilogue_sums(vg, 2)
            routes["record epilogue (4 rows x 4 couts per lane)"] = _epilogue_sums(vg, 4)
        r0 = H // 2 - 1
        a, b = gx.expected_sums(y, groups, 0, r0, grain)[g], gx.expected_sums(y, groups, r0, H, grain)[g]
        routes["two bands"] = (float(a[0] + b[0]), float(a[1] + b[1]))
        for what, (S1, S2) in routes.items():
            assert S1 == float(want_sums[g, 0]) and S2 == float(want_sums[g, 1]), f"{name} group {g} {what}: fp64 sums differ"
            assert _f32_stats(S1, S2, L) == want_bits, f"{name} group {g} {what}"


def _stats_of(s1, s2, L, grain):
    """bits per group, WITHOUT the unambiguity requirement (a mutant's sums may be anything)"""
    out = []
    for a, b in zip(s1, s2):
        plain, _ = gx.var_mean_forms(float(a) * grain, float(b) * grain * grain, float(L))
        out.append(plain[0].tobytes() + plain[1].tobytes())
    return out


def test_wrong_statistics_kernels_change_bits():
    c = gx.handover_stats_case(gx.HANDOVER_STATS[0])      # 128 couts, 4 per group: a quad is a group; 17 x 45: ragged
    y, grain, groups = c.y, c.g, 32
    q = (y.double() / grain).long()
    s1, s2, L = gx.group_sums(y, groups, grain)
    want = _stats_of(s1, s2, L, grain)
    H, W = y.shape[2:]
    # 1. / 2. one pixel of the ragged corner (a cout where it is not 0) dropped / counted twice
    ch = next(ch for ch in range(y.shape[1]) if int(q[0, ch, H - 1, W - 1]) != 0)
    v, g = int(q[0, ch, H - 1, W - 1]), ch // 4
    for sign, what in ((-1, "dropped"), (1, "counted twice")):
        m1, m2 = list(s1), list(s2)
        m1[g] += sign * v
        m2[g] += sign * v * v
        got = _stats_of(m1, m2, L, grain)
        assert got[g] != want[g], what
        assert [i for i in range(groups) if got[i] != want[i]] == [g]
    # 3. one lane partial (2 rows x 4 couts at one column) credited to the neighbouring quad: on random data the two groups' statistics
    #    are nearly the same, which is why a tolerance cannot see it
    lane = q[0, 8:12, 4:6, 7].reshape(-1)
    p1, p2 = int(lane.sum()), int((lane * lane).sum())
    assert p2 != 0
    m1, m2 = list(s1), list(s2)
    m1[2] -= p1; m2[2] -= p2; m1[3] += p1; m2[3] += p2      # noqa: E702
    got = _stats_of(m1, m2, L, grain)
    assert got[2] != want[2] and got[3] != want[3]
    rel = abs(np.frombuffer(got[2][:4], np.float32)[0] / np.frombuffer(want[2][:4], np.float32)[0] - 1.0)
    assert rel < 1e-2, "the mutant is supposed to be a small one"
    # 4. unbiased variance
    for gi in range(groups):
        S1, S2 = float(s1[gi]) * grain, float(s2[gi]) * grain * grain
        m = S1 / L
        unb = np.float32(max((S2 - L * m * m) / (L - 1), 0.0))
        assert unb.tobytes() != want[gi][:4]


def test_a_block_sum_of_squares_kept_in_fp32_changes_bits():
    """Not visible on the conv outputs of this class (|y| <= 255 grains: a 1024-value block stays below 2^24 grains^2 and fp32 holds it) --
    which is the point of that bound.  On the statistics pass's inputs with an offset of 1000 one block's share exceeds 2^24 by far."""
    shape = gx.STATS_SHAPES[5]
    x = gx.stats_case(shape, 1000).x
    s1, s2, L = gx.group_sums(x, 32, 1.0)
    want = _stats_of(s1, s2, L, 1.0)
    changed = 0
    for g in range(32):
        flat = x.double().reshape(32, -1)[g].numpy()
        idx = np.arange(L)
        mine = flat[(idx // 1024) % 64 == 0]           # block 0 of k_gn_partial's vector path: float4 i = b 256 + t + k 64 256
        acc = np.float32(0.0)
        for v in mine:
            acc = np.float32(np.float64(v) * v + np.float64(acc))
        m2 = s2[g] - int((mine * mine).sum()) + int(acc)
        changed += _stats_of([s1[g]], [m2], L, 1.0)[0] != want[g]
    assert changed >= 1, "an fp32 block sum of squares went unseen in all 32 groups"
    print(f"fp32 block sum of squares: {changed} of 32 groups change")


def test_no_input_of_this_class_needs_the_clamp():
    """The missing-clamp mutant has no witness here (module docstring): on a constant group the difference is exactly 0 in both forms, for
    every value and every group length the tables use; with any spread it is positive."""
    lengths = sorted({(s[1] // 32) * s[2] * s[3] for s in gx.STATS_SHAPES} | {4 * 17 * 45, 16 * 8 * 33, 8 * 9 * 40})
    for L in lengths:
        for c in (1, 3, 40, 255, 1000, 1040, -7, -1040):
            for grain in (1.0, 32.0):
                S1, S2 = float(c * L) * grain, float(c * c * L) * grain * grain
                m, q = S1 / L, S2 / L
                assert q - m * m == 0.0
                plain, fused = gx.var_mean_forms(S1, S2, float(L))
                assert float(plain[0]) == 0.0 and float(fused[0]) == 0.0
        if L > 1:      # one element off by one grain: var = (L - 1) / L^2, far above the rounding of m m
            c = 1040
            S1, S2 = float(c * L + 1), float(c * c * L + 2 * c + 1)
            m, q = S1 / L, S2 / L
            assert q - m * m > 0.0


def test_silu_models_are_the_identity_on_the_saturated_set():
    lat = gx.saturated(lr.lattice_operands((64, 64), 1152, 3, "x")).numpy().reshape(-1)
    vals = np.concatenate([np.array(gx.PROBE_VALUES, dtype=np.float32), lat, gx.saturated_sparse((64,), 3).numpy(), np.float32([gx.SAT_MIN])])
    gx.assert_saturated(torch.from_numpy(vals))
    for form, out in gx.silu_models(vals).items():
        assert np.array_equal(out, vals), form
    assert lat.min() < 32.0 and lat.min() >= 32.0 - 2.0 ** -5      # 32 |x| dips just under 32 where lo points towards zero
    # and the model is no identity in general: it would not pass a value that SiLU changes
    for form, out in gx.silu_models(np.float32([8.0, -3.0, 0.5])).items():
        assert (out != np.float32([8.0, -3.0, 0.5])).all(), form
    with pytest.raises(AssertionError):
        gx.assert_saturated(torch.tensor([8.0]))


def test_var_plus_eps_is_a_power_of_four():
    for k in range(6):
        var = np.float32(np.float32(4.0 ** -k) - np.float32(gx.EPS))
        assert np.float32(var + np.float32(gx.EPS)) == np.float32(4.0 ** -k)
        assert np.float32(1.0) / np.sqrt(np.float32(var + np.float32(gx.EPS))) == np.float32(2.0 ** k)
    co = gx.exact_coeffs(2, 64, 32, 4)
    assert bool((co.k[1:] != co.k[:-1]).all()) and bool((co.gamma[1:] != co.gamma[:-1]).all()) and bool((co.beta[1:] != co.beta[:-1]).all())
    assert bool((co.a < 0).any()) and bool((co.a > 0).any())


# ---- every precondition, for every row of every table -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", gx.STATS_SHAPES, ids=str)
def test_preconditions_statistics_pass(shape):
    for off in gx.STATS_OFFSETS:
        c = gx.stats_case(shape, off)
        assert c.var.shape == (shape[0] * 32,) and c.var.dtype == torch.float32
        if shape[2] * shape[3] * (shape[1] // 32) == 1:
            assert not c.var.any()
    bands = gx.stats_case(gx.BAND_SHAPE, 0)
    for lo, hi in gx.BANDS:
        assert gx.expected_sums(bands.x, 32, lo, hi).shape == (gx.BAND_SHAPE[0] * 32, 2)
    for px in gx.POOL_CASES:
        gx.pool_case(px)


@pytest.mark.parametrize("case", gx.HANDOVER_STATS, ids=str)
def test_preconditions_handover_statistics(case):
    c = gx.handover_stats_case(case)
    assert c.top <= 255 and c.ratio < 1.0
    assert set(torch.unique(c.act).tolist()) == {0.0, 32.0, 64.0}
    assert torch.equal(gx.affine_exact(c.x, c.co.a, c.co.s), c.act)
    assert bool((c.x < 0).any())      # negative a: the raw input is no copy of the activation


@pytest.mark.parametrize("case", gx.REC_STATS, ids=str)
def test_preconditions_record_statistics(case):
    c = gx.rec_stats_case(case)
    assert c.top <= 255 and c.ratio < 1.0
    assert torch.equal(lr.expected_split(c.x), c.x)      # integers: lo = 0, the record image holds them whole


@pytest.mark.parametrize("shape", gx.APPLY_SHAPES, ids=str)
def test_preconditions_apply(shape):
    for cls in gx.APPLY_CLASSES:
        c = gx.apply_case(shape, cls)
        assert c.want.shape == shape and torch.isfinite(c.want).all()
        if cls == "silu":
            gx.assert_saturated(c.want)
    u = gx.unsaturated_case()
    assert torch.equal(gx.affine_exact(u.x, u.a, u.s), u.t)


@pytest.mark.parametrize("case", gx.FUSED_CASES, ids=str)
def test_preconditions_fused_input(case):
    for cls in ("lattice", "integer"):
        c = gx.fused_case(case, cls)
        assert 0.0 < c.ratio < 1.0
        assert torch.equal(gx.affine_exact(c.x, c.co.a, c.co.s), c.act)
        hi, lo = lr.split(c.act)
        assert torch.equal((hi + lo).float(), c.act)      # the activation is a split-bf16 number: the kernel's operand is the activation itself


@pytest.mark.parametrize("case,up", gx.REC_ACT_CASES, ids=str)
def test_preconditions_activated_records(case, up):
    c = gx.rec_act_case(case, up)
    for terms in ("hh+hl+lh", "hh"):
        assert float(c.t[terms].min()) >= 32.0
        for form, out in gx.silu_models(c.t[terms].numpy().reshape(-1)[:4096]).items():
            assert np.array_equal(out, c.t[terms].numpy().reshape(-1)[:4096]), form


def test_preconditions_probes_record_inputs_and_routes():
    for row in gx.COEFF_PROBES:
        co = gx.coeff_probe(*row)
        assert co.coef.shape == (row[0], 2, row[1]) and (co.gamma is None) == (not row[3])
    for shape in gx.REC_FROM_SHAPES:
        c = gx.rec_from_case(shape)
        assert torch.equal(gx.affine_exact(c.x, c.co.a, c.co.s), c.want)
    rc = gx.routes_case()
    assert set(torch.unique(gx.affine_exact(rc.x_hand, rc.co.a, rc.co.s)).tolist()) == {0.0, 32.0, 64.0}
    assert torch.equal(rc.y_hand, rc.rec.y * 32.0)


# ---- mutants of the apply, the fused input and the activated record ----------------------------------------------------------------------------
@pytest.mark.parametrize("cls", gx.APPLY_CLASSES)
def test_wrong_coefficients_change_bits_in_the_apply(cls):
    shape = gx.APPLY_SHAPES[0]
    c = gx.apply_case(shape, cls)
    B, C = shape[:2]
    cpg = C // 32

    def planes_changed(a, s):
        t = c.x.double() * a.double().view(B, C, 1, 1) + s.double().view(B, C, 1, 1)
        if cls == "silu":
            t = t / (1.0 + torch.exp(-t))
        return (t.float() != c.want).flatten(2).any(dim=2)

    if cls != "plain":      # (without gamma and beta all channels of a group share their coefficients)
        assert bool(planes_changed(c.co.a.roll(1, dims=1), c.co.s.roll(1, dims=1)).all()), "neighbouring channel"
        assert bool(planes_changed(c.co.a, c.co.s.roll(1, dims=1)).all()), "the s row of the neighbouring channel"
    assert bool(planes_changed(c.co.a.roll(cpg, dims=1), c.co.s.roll(cpg, dims=1)).all()), "neighbouring group"


@pytest.mark.parametrize("cls", ["lattice", "integer"])
def test_a_pad_pixel_that_contributes_silu_s_changes_bits(cls):
    case = gx.FUSED_CASES[1]
    c = gx.fused_case(case, cls)
    B, cin, cout, H, W, _ = case
    s = c.co.s.double()
    pad_value = s / (1.0 + torch.exp(-s))                                                       # what a pad pixel with x = 0 would contribute
    assert bool((pad_value.abs() > 0).any()) and float(pad_value.abs().min()) < 1.0           # some s are small: the tolerance tests pass these
    ring = pad_value.view(B, cin, 1, 1).expand(B, cin, H + 2, W + 2).clone()
    ring[:, :, 1:-1, 1:-1] = 0.0
    delta = F.conv2d(ring, c.w.double())
    assert not delta[:, :, 1:-1, 1:-1].any()
    edge = torch.ones(H, W, dtype=torch.bool)
    edge[1:-1, 1:-1] = False
    got = (c.want["hh+hl+lh"].double() + delta).float()
    assert bool((got != c.want["hh+hl+lh"])[:, :, edge].float().mean() > 0.9)
    # coefficients of the neighbouring channel in the fused input
    act_wrong = gx.affine_exact(c.x, c.co.a.roll(1, dims=1), c.co.s.roll(1, dims=1))
    assert bool((act_wrong != c.act).flatten(2).any(dim=2).all())


def test_wrong_record_activations_change_bits():
    case, up = gx.REC_ACT_CASES[1]
    c = gx.rec_act_case(case, up)
    t, want = c.t["hh+hl+lh"], c.rec["hh+hl+lh"]
    hi, lo = lr.split(t)
    assert bool((hi.float() != want).float().mean() > 0.5), "lo of the activated value dropped"
    B, cout = t.shape[:2]
    y = c.y["hh+hl+lh"].double()
    a, s = c.coef[:, 0].double(), c.coef[:, 1].double()
    for shift, what in ((8, "the other record of the pair"), (16, "the other half of the 32-cout tile"), (1, "neighbouring channel")):
        tw = y * a.roll(shift, dims=1).view(B, cout, 1, 1) + s.roll(shift, dims=1).view(B, cout, 1, 1)
        assert bool((lr.expected_split(tw.float()) != want).flatten(2).any(dim=2).all()), what
    # an unactivated record (the raw y) is something else entirely
    assert bool((lr.expected_split(c.y["hh+hl+lh"]) != want).all())
