"""The instrument of tests/test_gpu_attn_exact.py, proved without a GPU (tests/attn_exact_ref.py holds constructions and model).

1. The preconditions hold on the actual tensors of every class, at the shapes the construction was first checked at, and print their gaps,
   grains and live-key counts.  The term-set expectations differ in more than 90 % of the elements (e).
2. flash_model -- 128-key blocks, four key tiles, running max / sum / alpha, P split to hi / lo, three- or one-term products, 1..4 key
   ranges merged by k_attn_combine's formula -- returns the expected bits in every accumulation order and for every split.
3. Every wrong kernel of attn_exact_ref.MUTANTS changes bits on the class named for it.
4. The mismatch report names the query's live keys by block, tile, step, lane half and part.
5. The graded class: the model stays inside the derived bound, the model without V_hi x P_lo does not."""
import pytest
import torch

import attn_exact_ref as ar

THREE, ONE = "hh+hl+lh", "hh"
C, TQ, TK = 128, 130, 450          # two query blocks, four key blocks with a ragged last one: every split 1..4 exists
POS = ar.twin_positions(C)[1]      # (61, 62, 63): last k-step of slab 0, upper lane half


def _class(name):
    if name == "selector":
        return ar.group_case(C, TQ, TK)
    if name.startswith("group"):
        _, n, placement = name.split("-")
        return ar.group_case(C, TQ, TK, 1, int(n), placement)
    return ar.twin_case(C, TQ, TK, 1, name.split("-")[1], POS)


CLASSES = ["selector", "group-2-spread", "group-2-packed", "group-4-spread", "group-4-packed", "twin-both", "twin-lh", "twin-hl", "twin-ll"]


@pytest.mark.parametrize("shape", [(128, 300, 300), (512, 1000, 333), (256, 77, 77)], ids=lambda s: "x".join(map(str, s)))
def test_preconditions_and_discrimination(shape):
    c, tq, tk = shape
    cases = [ar.group_case(c, tq, tk, 1, n, pl) for n, pl in ((1, "spread"), (2, "spread"), (2, "packed"), (4, "spread"), (4, "packed"))]
    cases += [ar.twin_case(c, tq, tk, 1, variant, pos) for variant in ("both", "lh", "hl", "ll") for pos in (ar.twin_positions(c)[0], ar.twin_positions(c)[-1])]
    for case in cases:
        print(case.name, ar.check_discrimination(case))
        assert min(case.gap[t] for t in ar.TERMS) >= ar.GAP + 1
        if case.name.startswith("twin"):
            tied = THREE if case.name.startswith("twin-ll") else ONE       # 2 live keys, 1 where an odd Tk leaves the last key alone
            assert case.counts[tied] == ([1, 2] if tk % 2 else [2]) and case.counts["full"] == [1]
        elif case.name.startswith("group"):
            n = int(case.name.split("-")[1])
            assert n in case.counts[THREE] and set(case.counts[THREE]) <= {1, n}
        else:
            assert case.counts[THREE] == [1]
        assert torch.equal(case.want(THREE), case.want("full")) or case.name.startswith("twin-ll")


def test_group_placements():
    spread, packed = ar.group_of_key(450, 4, "spread"), ar.group_of_key(450, 4, "packed")
    members = (spread == 5).nonzero().flatten().tolist()
    assert members == [5, 117, 229, 341]
    assert len({m // 16 for m in members}) == 4 and len({m // 128 for m in members}) >= 3      # other steps, other blocks
    assert {ar.decode_key(m, 4, 3)[-1] for m in members} == set("012")                                   # every part of a three-way split
    members = (packed == 5).nonzero().flatten().tolist()
    assert members == [20, 21, 22, 23] and len({m // 16 for m in members}) == 1
    assert torch.equal(spread[448:], torch.tensor([112, 113])) and torch.equal(packed[448:], torch.tensor([112, 113]))      # left over: alone


def test_twin_positions_cover_the_schedule():
    for c in (128, 256, 512):
        pos = ar.twin_positions(c)
        chans = [ch for p in pos for ch in p]
        assert {ch // 64 for ch in chans} == set(range(c // 64))               # every 64-channel slab
        assert {(ch % 16) // 8 for ch in chans} == {0, 1}                      # both halves of a k-step
        assert {(ch % 64) // 16 for ch in chans} >= {0, 3}                     # first and last k-step of a slab
        assert c - 1 in chans


@pytest.mark.parametrize("name", CLASSES)
def test_model_returns_the_expected_bits_in_every_order_and_split(name):
    case = _class(name)
    for terms, ts in ((3, THREE), (1, ONE)):
        for nsplit in (1, 2, 3, 4):
            for order in ("forward", "reversed", "shuffled"):
                out = ar.model_case(case, terms=terms, nsplit=nsplit, order=order, seed=nsplit)
                assert torch.equal(out, case.want(ts)), f"{name} terms={terms} nsplit={nsplit} {order}: {case.report(out, ts, nsplit)}"


def test_model_on_a_stacked_batch_and_a_key_band():
    case = ar.group_case(C, 300, 130, 2, 2, "spread")      # Tq != Tk, two images with different targets
    assert not torch.equal(case.want(THREE)[0], case.want(THREE)[1])
    out = ar.model_case(case, terms=3, nsplit=2, order="shuffled")
    assert torch.equal(out, case.want(THREE)), case.report(out, THREE, 2)


# mutant -> (arguments of flash_model); the class comes from attn_exact_ref.MUTANTS
MUTANT_RUNS = {
    "drop_hl": dict(arg=POS[2] // 16),
    "drop_lh": dict(arg=POS[0] // 16),
    "drop_vlo": dict(arg=5),
    "add_lolo": dict(),
    "lo_other_half": dict(arg=POS[2] // 16),
    "v_natural": dict(),
    "mask_gt": dict(),
    "pad_logit0": dict(arg=2),                 # key tile 2 of the last block is all padding (keys 448, 449 are the last real ones)
    "no_alpha_acc": dict(),
    "no_l_rescale": dict(),
    "combine_drop": dict(arg=1, nsplit=3),
    "combine_wrong_w": dict(nsplit=2),
    "store_lt": dict(),
    "store_le": dict(),
}


@pytest.mark.parametrize("mutant", sorted(MUTANT_RUNS))
def test_wrong_kernel_changes_bits(mutant):
    what, cls = ar.MUTANTS[mutant]
    case = _class(cls)
    kw = MUTANT_RUNS[mutant]
    intact = ar.model_case(case, terms=3, nsplit=kw.get("nsplit", 1))
    assert torch.equal(intact, case.want(THREE))
    out = ar.model_case(case, terms=3, mutant=mutant, **kw)
    report = case.report(out, THREE, kw.get("nsplit", 1))
    print(f"{mutant} ({what}) on {cls}: {report}")
    assert not torch.equal(out, case.want(THREE)), f"{mutant} ({what}) is not caught by {cls}"


def test_every_listed_mutant_is_run():
    assert set(MUTANT_RUNS) | {"drop_plo"} == set(ar.MUTANTS)


def test_the_full_twin_alone_would_miss_a_single_lo_term():
    """why the single-channel variants exist: with both tie-breaks in, the other lo term still separates the pair"""
    case = _class("twin-both")
    for mutant, ch in (("drop_hl", POS[2]), ("drop_lh", POS[0])):
        assert torch.equal(ar.model_case(case, terms=3, mutant=mutant, arg=ch // 16), case.want(THREE))


def test_mismatch_report():
    case = ar.group_case(C, TQ, TK, 1, 2, "spread")
    want = case.want(THREE)
    assert case.report(want.clone(), THREE, 3) == "equal"
    got = want.clone()
    got[0, 7, 100] += 0.5
    got[0, 9, 101] = float("nan")
    keys = case.live(THREE)[0, 100].nonzero().flatten().tolist()
    assert keys == [28, 253]          # target group (7 * 100 + 3) % 225, members 225 apart
    text = case.report(got, THREE, 3)
    print(text)
    assert text.startswith(f"2 of {want.numel()} elements differ; first at (b, c, query) = (0, 7, 100)")
    assert "key 28: block 0, tile 0, step 1, lane half 1, part 0" in text
    assert "key 253: block 1, tile 3, step 7, lane half 1, part 1" in text
    w = float(want[0, 7, 100])
    assert f"got {w + 0.5!r}, want {w!r}, difference 0.5" in text
    assert "shape" in ar.attn_mismatch_report(got[:, :5], want, case.live(THREE))


def test_decode_key_parts_follow_the_kernels_ranges():
    # nkb = 8, nsplit = 3: blocks [0, 2), [2, 5), [5, 8)
    assert [ar.decode_key(128 * blk, 8, 3).rsplit(" ", 1)[1] for blk in range(8)] == ["0", "0", "1", "1", "1", "2", "2", "2"]
    assert ar.decode_key(128 + 32 + 16 + 12, 4, 1) == "key 188: block 1, tile 1, step 3, lane half 1, part 0"


def test_graded_model_inside_the_bound_and_p_lo_is_seen():
    case = ar.graded_case(128, 450)      # at 129 keys too few lie within a few Hamming steps of a target for P_lo to pass the bound
    lo, hi = case.s2_range(THREE)
    assert -60 < lo and 20 < hi < 45
    for terms, ts, tol in ((3, THREE, ar.TOL_THREE), (1, ONE, ar.TOL_ONE)):
        ref, mag = case.reference(ts)
        out = ar.model_case(case, terms=terms).double()
        ratio = float(((out - ref).abs() / (tol * mag)).max())
        print(f"graded model terms={terms}: max error / bound = {ratio:.3f}")
        assert ratio < 1.0
    ref, mag = case.reference(THREE)
    out = ar.model_case(case, terms=3, mutant="drop_plo").double()
    ratio = float(((out - ref).abs() / (ar.TOL_THREE * mag)).max())
    print(f"graded model without V_hi x P_lo: max error / bound = {ratio:.1f}")
    assert ratio > 1.0
