"""The instrument of tests/test_gpu_f16_exact.py, proven on the CPU before any kernel is trusted to it (tests/f16_exact_ref.py).

  * h(t), the conversion contract of csrc/f16_convert.h, agrees with an integer-arithmetic model that uses no float16 cast, on every fp16
    number, on quarter-ulp neighbours and ties of every binade, on subnormals and beyond the range;
  * every precondition holds for every row of every case table (the builders assert them and are cached: the GPU module gets the very same
    objects); the ratios sum |terms| / (2^24 g) are printed;
  * the products of a few output elements, added in fp32 in random orders and in blocks of 4, 8 and 16 (as an MFMA would), give one bit
    pattern, which is the fp64 value;
  * wrong kernels change bits on the case aimed at them: truncation, round-half-away, conversion before the clamp, subnormals flushed, three
    bf16 terms on the unrounded operands, one bf16 term, one k-step from the neighbouring output channel, a record output rounded from a
    value first cut to 16 bits;
  * the precondition rejects fine bits on both operands at K = 1152."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import f16_exact_ref as fx
import gn_exact_ref as gx
import lattice_ref as lr


# ---- the conversion ---------------------------------------------------------------------------------------------------------------------------
def _all_fp16_numbers():
    bits = np.arange(0, 0x7C00, dtype=np.uint16)                     # every finite non-negative fp16
    return torch.from_numpy(bits.view(np.float16).astype(np.float32))


def test_h_is_the_integer_model_of_the_contract():
    f16 = _all_fp16_numbers()
    assert float(f16[-1]) == fx.F16_MAX and float(f16[1]) == 2.0 ** -24
    assert torch.equal(fx.h(f16), f16) and torch.equal(fx.h_integer_model(f16), f16)
    nxt = torch.cat([f16[1:], torch.tensor([65536.0])])
    gap = (nxt - f16).double()
    vals = [f16.double() + gap * q for q in (0.25, 0.5, 0.75, 0.5 - 2.0 ** -12, 0.5 + 2.0 ** -12)]
    vals.append(torch.tensor([65520.0, 70000.0, 1e30, 3e38, fx._BELOW_65520, 2.0 ** -26, 2.0 ** -25, 3 * 2.0 ** -26, 1e-40, 0.0], dtype=torch.float64))
    t = torch.cat(vals).float()
    t = torch.cat([t, -t])
    gen = torch.Generator().manual_seed(3)
    t = torch.cat([t, torch.randn(1 << 16, generator=gen) * torch.exp2(torch.randint(-30, 20, (1 << 16,), generator=gen).float())])
    got, model = fx.h(t), fx.h_integer_model(t)
    assert torch.equal(got, model), lr.mismatch_report(got, model, 2.0 ** -24)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) == fx.F16_MAX
    # the ties of the first block (q = 0.5) go to the even neighbour: the fp16 number with an even bit pattern
    tie = (f16.double() + gap * 0.5).float()
    lower_even = (torch.arange(len(f16)) % 2 == 0)
    want = torch.where(lower_even, f16, nxt).clamp(max=fx.F16_MAX)
    assert torch.equal(fx.h(tie), want)
    assert bool(fx.ties(tie[:-1]).all()) and not bool(fx.ties(f16).any())


def test_conversion_table_holds_what_the_issue_lists():
    c = fx.conversion_case()
    t, want = c.t, c.want
    for v in (65520.0, 70000.0, 1e30, 3e38, fx._BELOW_65520):
        sel = t == torch.tensor(v, dtype=torch.float32)
        assert bool(sel.any()) and bool((want[sel] == fx.F16_MAX).all()), v
    assert bool(fx.ties(t).any()) and bool((t == 0).any()) and bool(((t >= 2048) & (t < fx.F16_MAX) & (want != t)).any())
    even_odd = {float(v): float(fx.h(torch.tensor([v]))) for v in (2049.0, 2051.0, 40016.0, 40048.0)}
    assert even_odd == {2049.0: 2048.0, 2051.0: 2052.0, 40016.0: 40000.0, 40048.0: 40064.0}      # both directions: to the even neighbour
    assert bool((c.coef[:, 0] < 0).any()) and bool((c.x < 0).any())


# ---- every precondition, for every row of every table -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fx.ALL_CONV_CASES, ids=str)
def test_preconditions_conv_cases(case):
    for cls in fx.CLASSES:
        c = fx.conv_case(case, cls)
        print(f"precondition {case} {cls}: sum|terms| / (2^24 g) = {c.ratio:.3f}; h changes x {c.changed['x']:.3f} w {c.changed['w']:.3f}; "
              f"differs from three terms {c.differs['hh+hl+lh']:.4f}, from one term {c.differs['hh']:.4f}")
        assert 0.0 <= c.ratio < 1.0
        assert torch.equal(gx.affine_exact(c.x, c.co.a, c.co.s), c.act)
        assert torch.equal(fx.h_integer_model(c.act), c.h_act) and torch.equal(fx.h_integer_model(c.w), c.h_w)
        if cls != "integer":
            assert bool((c.x < 0).any())
        if c.out is not None:
            assert c.out.changed > 0.5 and c.out.ties > 0
            for form, out in gx.silu_models(c.out.t.numpy().reshape(-1)[:4096]).items():
                assert np.array_equal(out, c.out.t.numpy().reshape(-1)[:4096]), form
    assert (fx.conv_case(case, "fine_x").out is not None) == (case[2] % 128 == 0)


def test_precondition_ratios_at_the_three_k():
    """the table of the module's design: fine bits on x / on w at K = 1152, 2304, 4608"""
    rows = {1152: lr.REC_DIRECT[0], 2304: lr.REC_DIRECT[2], 4608: lr.REC_DIRECT[3]}
    for K, case in rows.items():
        assert 9 * case[1] == K
        rx, rw = fx.conv_case(case, "fine_x").ratio, fx.conv_case(case, "fine_w").ratio
        print(f"K = {K}: fine x {rx:.3f}, fine w {rw:.3f} of 2^24 g")
        assert rx < 1.0 and rw < 1.0
    print(f"subnormal class at K = 1152: {fx.conv_case(rows[1152], 'subnormal').ratio:.3f}")


def test_preconditions_probe_producers_statistics_and_upsample():
    p = fx.accumulation_probe()
    print(f"accumulation probe: the largest sum is {p.ratio:.3f} of 2^24 g")
    assert torch.equal(gx.affine_exact(p.x, p.co.a, p.co.s), p.act)
    for shape in gx.REC_FROM_SHAPES:
        c = fx.rec_from_case(shape)
        assert torch.equal(gx.affine_exact(c.x, c.co.a, c.co.s), c.t) and torch.equal(fx.h_integer_model(c.t), c.want)
    for case in fx.STATS_CASES:
        c = fx.rec_stats_case(case)
        assert c.top <= 255 and c.ratio < 1.0 and set(torch.unique(c.act).tolist()) == {0.0, 32.0, 64.0}
    assert len(fx.STATS_CASES) == 5 and any(c[7] == 0 for c in fx.STATS_CASES)
    for case in (lr.REC_UP, fx.UP_WINDOW_WHOLE):
        c = fx.up_record_case(case)
        assert c.ratio < 1.0 and c.out.changed > 0.5 and c.out.ties > 0
    for v in gx.PROBE_VALUES:
        assert float(fx.h(torch.tensor([v]))) == v      # the identity probe's values are fp16 numbers


def test_fine_bits_on_both_operands_are_rejected():
    assert "no multiple of the grain" in fx.both_fine_is_rejected(1152)


# ---- summation orders -------------------------------------------------------------------------------------------------------------------------
def _terms_of(c, b, co, y, x):
    """every term of output element (b, co, y, x) in units of the kernel's values: products h(act) h(w), bias, residual (fp64, exact)"""
    xp = F.pad(c.h_act.double(), (1, 1, 1, 1))[b, :, y:y + 3, x:x + 3]
    terms = (xp * c.h_w[co].double()).reshape(-1).numpy()
    extra = [float(t) for t in ([] if c.bias is None else [c.bias[co]]) + ([] if c.res is None else [c.res[b, co, y, x]])]
    return terms, extra


def _f32_sum(values, start=0.0):
    acc = np.float32(start)
    for v in values:
        acc = np.float32(acc + np.float32(v))
    return acc


@pytest.mark.parametrize("case,cls", [(lr.REC_DIRECT[1], "fine_x"), (lr.REC_DIRECT[1], "fine_w"), (lr.REC_DIRECT[3], "fine_x"), (lr.REC_DIRECT[0], "subnormal"),
                                      (lr.HANDOVER_3X3[2], "fine_w")], ids=str)
def test_every_summation_order_gives_the_fp64_value(case, cls):
    c = fx.conv_case(case, cls)
    B, cin, cout, H, W, _ = case
    rng = np.random.default_rng(7)
    for b, co, y, x in ((0, 0, 0, 0), (B - 1, cout - 1, H - 1, W - 1), (0, cout // 2, H // 2, W // 2), (0, 1, 1, W - 2)):
        terms, extra = _terms_of(c, b, co, y, x)
        assert all(np.float32(v) == v for v in terms)                                   # a product of two fp16 numbers is an fp32 number
        exact = float(np.sum(terms.astype(np.float64)) + sum(extra))
        want_bits = np.float32(float(c.want[b, co, y, x])).tobytes()
        assert np.float32(exact).tobytes() == want_bits and float(np.float32(exact)) == exact
        got = {"in order, offsets last": _f32_sum(extra, _f32_sum(terms)), "offsets first": _f32_sum(terms, _f32_sum(extra))}
        for i in range(3):
            got[f"shuffled {i}"] = _f32_sum(extra, _f32_sum(terms[rng.permutation(len(terms))]))
        for blk in (4, 8, 16):      # a block's products are added first, then the block joins the accumulator
            p = terms[rng.permutation(len(terms))]
            acc = _f32_sum(extra)
            for i in range(0, len(p), blk):
                acc = np.float32(acc + _f32_sum(p[i:i + blk]))
            got[f"blocks of {blk}"] = acc
        for what, v in got.items():
            assert np.float32(v).tobytes() == want_bits, f"{case} {cls} element {(b, co, y, x)} {what}: {float(v)!r} != {exact!r}"


# ---- wrong kernels change bits ------------------------------------------------------------------------------------------------------------------
def _conv_with(c, act=None, w=None):
    act = c.h_act if act is None else act
    w = c.h_w if w is None else w
    y = F.conv2d(act.double(), w.double(), padding=1)
    y = lr._with_offsets(y, None if c.bias is None else c.bias, c.res)
    return y.float()


def test_wrong_conversions_change_bits():
    conv = fx.conversion_case()
    mut = fx.h_mutants(conv.t)
    for name in ("truncation", "round-half-away", "conversion before the clamp", "wrong saturate"):
        assert not torch.equal(mut[name], conv.want), name
    assert bool(torch.isinf(mut["conversion before the clamp"]).any())
    tie = fx.ties(conv.t)
    assert bool((mut["round-half-away"][tie] != conv.want[tie]).any()) and bool((mut["round-half-away"][tie] == conv.want[tie]).any())      # odd and even neighbours
    assert torch.equal(mut["round-half-away"][~tie], conv.want[~tie])                  # ... and only the ties tell the two roundings apart
    # in a conv: on either operand, in more than 0.9 of the output elements
    for cls in ("fine_x", "fine_w"):
        c = fx.conv_case(lr.REC_DIRECT[1], cls)
        assert torch.equal(_conv_with(c), c.want)
        for name in ("truncation", "round-half-away"):
            for which in ("act", "w"):
                kw = {which: fx.h_mutants(c.act if which == "act" else c.w)[name]}
                changed = float((_conv_with(c, **kw) != c.want).float().mean())
                assert changed > 0.9, f"{cls}: {name} of {which} changes only {changed:.3f}"
    s = fx.conv_case(lr.REC_DIRECT[0], "subnormal")
    assert torch.equal(_conv_with(s), s.want)
    flushed = fx.h_mutants(s.w)["subnormals flushed"]
    assert bool((flushed[flushed != 0].abs() == 2.0 ** -14).all()) and int((flushed != 0).sum()) >= 2      # only the weights that round up to 2^-14 survive a flush
    assert float((_conv_with(s, w=flushed) != s.want).float().mean()) > 0.9
    for name in ("truncation", "round-half-away"):
        assert float((_conv_with(s, w=fx.h_mutants(s.w)[name]) != s.want).float().mean()) > 0.9, name


@pytest.mark.parametrize("case", [lr.REC_DIRECT[1], lr.HANDOVER_3X3[2], lr.REC_DIRECT[3]], ids=str)
def test_other_arithmetic_and_a_misplaced_k_step_change_bits(case):
    B, cin, cout, H, W, _ = case
    for cls in ("fine_x", "fine_w", "subnormal"):
        c = fx.conv_case(case, cls)
        assert c.differs["hh+hl+lh"] > 0.9 and c.differs["hh"] > 0.9                   # three terms on the unrounded operands; one bf16 term
        # one k-step -- 32 consecutive K indices: one tap, cins [32, 64) (the whole of a short cin) -- read from the neighbouring output channel
        w = c.h_w.clone()
        hi = min(64, cin)
        w[:, 32:hi, 1, 1] = c.h_w.roll(-1, dims=0)[:, 32:hi, 1, 1]
        changed = (_conv_with(c, w=w) != c.want).flatten(2).float().mean(dim=2)
        assert float(changed.min()) > 0.8, f"{case} {cls}: a plane changes in only {float(changed.min()):.3f} of its elements"
    i = fx.conv_case(case, "integer")
    assert i.differs == {"hh+hl+lh": 0.0, "hh": 0.0}


def test_a_record_output_rounded_twice_changes_bits():
    for c in (fx.conv_case(lr.REC_DIRECT[1], "fine_x").out, fx.conv_case(lr.REC_DIRECT[3], "fine_w").out, fx.up_record_case(lr.REC_UP).out):
        twice = fx.h(lr.expected_split(c.t))                                           # cut to 16 bits (hi + lo) first, then to fp16
        n = int((twice != c.rec).sum())
        print(f"double rounding changes {n} of {c.rec.numel()} record values")
        assert n > 0
        assert not torch.equal(lr.expected_split(c.t), c.rec)                          # a bf16 split read as the record is something else
