"""The instrument of tests/test_gpu_conv_lattice.py, proven on the CPU before any kernel is trusted to it (tests/lattice_ref.py).

On the lattice every fp32 partial sum of the three-term products is exact, so the accumulation order cannot matter and the result is one
bit pattern.  Checked here with the numpy model of the kernels' arithmetic (tests/test_split_bf16_model.py: split, _dot3), at every K
the GPU file uses:
  * the model's splitter returns the lattice's own hi and lo;
  * four accumulation orders give identical bits, equal to lattice_ref.expected_conv;
  * four ways a kernel can be subtly wrong (a dropped lo*hi k-step, an added lo*lo, two swapped lo values, a truncating splitter) each
    change output bits -- without that the GPU test's power would only be a claim;
  * the sub-pixel (merged-weight) form of the upsample conv equals nearest-2x + 3x3 on the taps' own halves, and the Downsample padding
    is torch's;
  * the precondition check refuses operands whose sums outgrow fp32."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lattice_ref as lr
import test_split_bf16_model as sm

M, N = 16, 8      # rows of a, rows of b: every (m, n) pair is one dot product of the model


def _operands(K, seed=3, terms="hh+hl+lh"):
    a, ah, al = lr.lattice_operands((M, K), K, seed, "x", terms, halves=True)
    b, bh, bl = lr.lattice_operands((N, K), K, seed, "w", terms, halves=True)
    return (a, ah, al), (b, bh, bl)


def _pairs(a, b):
    """[M, K], [N, K] numpy -> the [M N, K] operand rows of every (m, n) dot product"""
    return np.repeat(a, b.shape[0], axis=0), np.tile(b, (a.shape[0], 1))


def _expected(a, b, terms):
    """the same dot products through expected_conv: a as M one-pixel images of K channels, b as N 1x1 filters"""
    y = lr.expected_conv(a.view(M, -1, 1, 1), b.view(N, -1, 1, 1), None, None, terms=terms, k=1)
    return y.reshape(-1).numpy()


def _acc(steps):
    """fp32 accumulation of a sequence of [rows, <= 16] product blocks: each block is summed exactly, as one MFMA does, then rounded"""
    acc = None
    for p, q in steps:
        s = np.sum(p.astype(np.float64) * q, axis=1)
        acc = s.astype(np.float32) if acc is None else (acc + s).astype(np.float32)
    return acc


def _steps(ah, al, bh, bl, K, drop=None, extra_lolo=False):
    """(k-step, term) blocks in the model's order: lo*hi, hi*lo, [lo*lo], hi*hi per 16-deep k-step.  drop = (k-step, term index)."""
    out = []
    for i, k in enumerate(range(0, K, 16)):
        sl = slice(k, k + 16)
        terms = [(al, bh), (ah, bl)] + ([(al, bl)] if extra_lolo else []) + [(ah, bh)]
        out += [(t, (p[:, sl], q[:, sl])) for t, (p, q) in enumerate(terms) if drop != (i, t)]
    return out


@pytest.mark.parametrize("K", lr.KS_THREE_TERM)
def test_model_splitter_reproduces_the_lattice(K):
    for role in ("x", "w", "w_up"):
        x, hi, lo = lr.lattice_operands((64, K), K, 11, role, halves=True)
        mh, ml = sm.split(x.numpy())
        assert np.array_equal(mh, hi.numpy()) and np.array_equal(ml, lo.numpy()), role
        th, tl = lr.split(x)
        assert torch.equal(th, hi.double()) and torch.equal(tl, lo.double())
        assert np.array_equal(sm.bf16_round(lo.numpy()), lo.numpy())      # lo is itself a bf16 number
    assert (lo != 0).any() and (lo < 0).any() and (lo > 0).any()


@pytest.mark.parametrize("K", lr.KS_THREE_TERM)
def test_three_term_sum_is_one_bit_pattern_in_every_order(K):
    (a, _, _), (b, _, _) = _operands(K)
    A, B = _pairs(a.numpy(), b.numpy())
    (ah, al), (bh, bl) = sm.split(A), sm.split(B)
    want = _expected(a, b, "hh+hl+lh")
    ratio = lr.assert_exact_in_fp32(a.view(M, K, 1, 1), b.view(N, K, 1, 1), None, None, lr.lattice_plan(K).g, terms="hh+hl+lh", k=1)
    assert 0.0 < ratio < 1.0
    steps = _steps(ah, al, bh, bl, K)
    forward = sm._dot3(A, B)
    assert np.array_equal(forward, _acc([s for _, s in steps]))       # _acc is the model's accumulation
    orders = {
        "reversed": [s for _, s in reversed(steps)],
        "term-major": [s for t in (0, 1, 2) for tt, s in steps if tt == t],
        "permuted k-steps": [steps[3 * i + t][1] for i in np.random.default_rng(K).permutation(len(steps) // 3) for t in (0, 1, 2)],
    }
    for name, order in orders.items():
        assert np.array_equal(_acc(order), forward), name
    assert np.array_equal(forward, want)
    # the one-term mode's value is exact under the same condition
    assert np.array_equal(_acc([s for t, s in steps if t == 2]), _expected(a, b, "hh"))


@pytest.mark.parametrize("K", lr.KS_FP32_CHAIN)
def test_fp32_chain_is_one_bit_pattern_in_every_order(K):
    """conv_in's kernel is a chain of fp32 FMAs on the unsplit operands: lo*lo is in every product, the plan's grain is 2^-18."""
    (a, _, _), (b, _, _) = _operands(K, terms="full")
    A, B = _pairs(a.numpy(), b.numpy())
    want = _expected(a, b, "full")
    assert lr.assert_exact_in_fp32(a.view(M, K, 1, 1), b.view(N, K, 1, 1), None, None, lr.lattice_plan(K, "full").g, terms="full", k=1) < 1.0
    for order in (np.arange(K), np.arange(K)[::-1], np.random.default_rng(K).permutation(K)):
        acc = np.zeros(A.shape[0], dtype=np.float32)
        for k in order:
            acc = (acc + A[:, k].astype(np.float64) * B[:, k]).astype(np.float32)      # one FMA: exact product, one rounding
        assert np.array_equal(acc, want)
    # a kernel that split its operands and dropped lo*lo would not pass
    assert (sm._dot3(np.pad(A, ((0, 0), (0, -K % 16))), np.pad(B, ((0, 0), (0, -K % 16)))) != want).any()


@pytest.mark.parametrize("K", lr.KS_THREE_TERM)
def test_subtly_wrong_kernels_change_bits(K):
    (a, _, _), (b, _, _) = _operands(K, seed=5)
    A, B = _pairs(a.numpy(), b.numpy())
    (ah, al), (bh, bl) = sm.split(A), sm.split(B)
    want = _expected(a, b, "hh+hl+lh")
    nk = (K + 15) // 16
    # 1. lo*hi missing in one 16-deep k-step (the last but one, or the only one)
    step = max(nk - 2, 0)
    got = _acc([s for _, s in _steps(ah, al, bh, bl, K, drop=(step, 0))])
    missing = np.sum(al[:, 16 * step:16 * step + 16].astype(np.float64) * bh[:, 16 * step:16 * step + 16], axis=1)
    assert np.array_equal(got.astype(np.float64), want - missing) and (got != want).any()
    # 2. lo*lo added where the contract drops it
    assert (sm._dot3(A, B, terms=4) != want).any()
    # 3. the lo of two adjacent k-positions swapped in one operand
    al2 = al.copy()
    al2[:, [4, 5]] = al[:, [5, 4]]
    assert (_acc([s for _, s in _steps(ah, al2, bh, bl, K)]) != want).any()
    # 4. a splitter that truncates hi instead of rounding it to nearest
    at_h = (A.view(np.uint32) & 0xFFFF0000).view(np.float32)
    at_l = sm.bf16_round(A - at_h)
    assert np.array_equal(at_h.astype(np.float64) + at_l, A.astype(np.float64)) and (at_h != ah).any()      # still a split of a
    assert (_acc([s for _, s in _steps(at_h, at_l, bh, bl, K)]) != want).any()


@pytest.mark.parametrize("cls", ["lattice", "integer"])
def test_subpixel_form_equals_nearest_upsample_then_conv(cls):
    """expected_conv(up=True) splits the MERGED weights as the packers do.  With one sign per (cout, cin) pair ("w_up") the merged
    weight's split is the sum of the taps' splits, so the value equals nearest-2x + 3x3 on the taps' own halves; with free signs it need
    not (a merged weight near zero rounds differently), and the helper's grain check says so."""
    B, cin, cout, h, w = 2, 32, 8, 5, 7
    K = 9 * cin
    if cls == "lattice":
        x, wt = lr.lattice_operands((B, cin, h, w), K, 2, "x"), lr.lattice_operands((cout, cin, 3, 3), K, 2, "w_up")
        bias, res, g = lr.lattice_operands((cout,), K, 2, "bias"), lr.lattice_operands((B, cout, 2 * h, 2 * w), K, 2, "residual"), lr.lattice_plan(K).g
    else:
        x, wt = lr.integer_operands((B, cin, h, w), 2, "x"), lr.integer_operands((cout, cin, 3, 3), 2, "w")
        bias, res, g = lr.integer_operands((cout,), 2, "bias"), lr.integer_operands((B, cout, 2 * h, 2 * w), 2, "residual"), 1.0
    lr.assert_exact_in_fp32(x, wt, bias, res, g, terms="hh+hl+lh", up=True, k=3)
    xu = F.interpolate(x, scale_factor=2.0, mode="nearest")
    for terms in ("hh+hl+lh", "hh"):
        assert torch.equal(lr.expected_conv(x, wt, bias, res, terms=terms, up=True, k=3), lr.expected_conv(xu, wt, bias, res, terms=terms, k=3)), terms
    if cls == "integer":      # (lo*lo leaves the three-term lattice's grain: "full" is for integers)
        full = lr.expected_conv(x, wt, bias, res, terms="full", up=True, k=3)
        assert torch.equal(full, (F.conv2d(xu.double(), wt.double(), bias.double(), padding=1) + res).float())
    else:
        free = lr.lattice_operands((cout, cin, 3, 3), K, 2, "w")
        with pytest.raises(AssertionError, match="grain"):
            lr.assert_exact_in_fp32(x, free, bias, res, g, terms="hh+hl+lh", up=True, k=3)


@pytest.mark.parametrize("hw", [(9, 11), (8, 10)])
def test_downsample_padding_is_ldms(hw):
    """stride=2: pad right 1, bottom 1, then a stride-2 conv without padding -- ldm's Downsample, (H - 2) // 2 + 1 output rows."""
    x, wt, bias = lr.integer_operands((1, 4, *hw), 3, "x"), lr.integer_operands((5, 4, 3, 3), 3, "w"), lr.integer_operands((5,), 3, "bias")
    want = F.conv2d(F.pad(x, (0, 1, 0, 1), mode="constant", value=0.0), wt, bias, stride=2, padding=0)
    got = lr.expected_conv(x, wt, bias, None, terms="full", stride=2, k=3)
    assert got.shape == (1, 5, (hw[0] - 2) // 2 + 1, (hw[1] - 2) // 2 + 1) and torch.equal(got, want)
    assert torch.equal(lr.expected_conv(x, wt, bias, None, terms="hh+hl+lh", stride=2, k=3), want)      # integers: lo = 0, every mode alike


def test_integer_class_is_the_same_in_every_mode():
    x, wt = lr.integer_operands((1, 64, 6, 7), 4, "x"), lr.integer_operands((16, 64, 3, 3), 4, "w")
    bias, res = lr.integer_operands((16,), 4, "bias"), lr.integer_operands((1, 16, 6, 7), 4, "residual")
    assert lr.assert_exact_in_fp32(x, wt, bias, res, 1.0, terms="full", k=3) < 1e-3
    ys = [lr.expected_conv(x, wt, bias, res, terms=t, k=3) for t in lr.TERMS]
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[0], ys[2])
    assert torch.equal(ys[0], (F.conv2d(x, wt, bias, padding=1) + res))
    assert x.min() == -4 and x.max() == 4


def test_precondition_rejects_a_k_too_large_for_its_hi_sets():
    with pytest.raises(ValueError):
        lr.lattice_plan(4609)
    with pytest.raises(ValueError):
        lr.lattice_plan(37, "full")
    # the full hi sets (the plan of K <= 1152) at K = 4608: sums reach ~2 x 2^24 g
    plan = lr.lattice_plan(1152)
    x, wt = lr.lattice_operands((1, 4608, 1, 4), 1152, 6, "x"), lr.lattice_operands((8, 4608, 1, 1), 1152, 6, "w")
    with pytest.raises(AssertionError, match="2\\^24 g"):
        lr.assert_exact_in_fp32(x, wt, None, None, plan.g, terms="hh+hl+lh", k=1)
    # and operands of a coarser plan do not pass for a finer grain than their products have
    with pytest.raises(AssertionError, match="grain"):
        lr.assert_exact_in_fp32(x[:, :64], wt[:, :64], None, None, 2.0 ** -8, terms="hh+hl+lh", k=1)
    # lo*lo of the three-term lattice has a 2^-20 grain: the exact-fp32 expectation is refused at the three-term grain
    with pytest.raises(AssertionError, match="grain"):
        lr.assert_exact_in_fp32(x[:, :64], wt[:, :64], None, None, plan.g, terms="full", k=1)


def test_mismatch_report_names_count_index_and_grains():
    want = torch.zeros(2, 3, 4, 5)
    got = want.clone()
    got[1, 2, 0, 3] = 3 * 2.0 ** -12
    got[1, 2, 3, 4] = 1.0
    msg = lr.mismatch_report(got, want, 2.0 ** -12)
    assert "2 of 120" in msg and "(1, 2, 0, 3)" in msg and "difference 3 g" in msg
