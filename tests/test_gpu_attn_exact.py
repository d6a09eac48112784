"""Bit-exact tests of the VAE attention: inputs whose softmax is exact in fp32 (tests/attn_exact_ref.py).

On randn logits every output row averages hundreds of keys, and a product missing in one k-step or one output MFMA site, a lo fragment
of the neighbouring lane half, a padded key let into one key tile or a key-range part merged with the wrong weight moves the result by a
fraction of the 5e-5 tolerance.  Here every query has 1, 2 or 4 live keys of exactly equal logit and every other key at least 160 below
in the log2 domain: exp2(0) = 1, exp2(<= -160) = 0, P is 0 or 1, the denominator is a power of two and the kernel's result is ONE bit
pattern, the mean of the mode's V value over the live keys:
    MDTILE_PRECISION_BF16X3                       v_hi + v_lo of the keys live under hh + hl + lh     k_attn_bf16x3 (+ k_attn_combine)
    MDTILE_PRECISION_BF16, MDTILE_PRECISION_F16   v_hi of the keys live under hh                      k_attn_bf16x1 (+ k_attn_combine)
    exact=True, MDTILE_PRECISION_F32              v of the keys live under the full products          k_attn (token-major v only)
Classes selector, group (1, 2, 4 live keys, spread over blocks and parts or packed into one 16-key step) and twin (pairs of keys that only
Q_lo x K_hi, only Q_hi x K_lo, both, or only lo x lo tell apart); every assertion of the value tests is torch.equal, and a mismatch
message names the first (b, c, query) and that query's live keys by 128-key block, key tile, 16-key step, lane half and key-range part.
tests/test_attn_exact_host.py proves the instrument on a CPU model of the schedule: every order and split agrees, 14 wrong kernels change
bits.  The key-range split a case gets is read from the workspace size and printed; the table reaches 1, 2, 3 and 4 by shape alone.

What the construction supposes of the hardware -- v_exp_f32 returns exactly 1.0 at 0 and exactly 0 at <= -160, and so do expf / exp2f as
hipcc compiles them in k_attn / k_attn_combine -- is settled by these tests themselves: they can only pass if it holds.
The first run on an MI355X settled it: every value test of this module passed bit for bit, in every mode and at every split.

The graded class (sign codes with lattice magnitudes, |s'| <= ~40) is the one that sees P_lo x V_hi: it is compared with an fp64
softmax on the mode's term set under the per-element bound tol * sum_j p_j |v_j|, tol = 2^-15 (three-term, exact) or 2^-7 (one-term).
Measured max error / bound on an MI355X (token- and channel-major v give the same bits), T = 129 / 450 / 1000:
    three-term   C = 128: 0.025 / 0.029 / 0.030    C = 512: 0.023 / 0.029 / 0.034
    one-term     C = 128: 0.001 / 0.022 / 0.013    C = 512: 0.001 / 0.003 / 0.008      (BF16 and F16 alike)
    exact        C = 128: 0.026 / 0.054 / 0.081    C = 512: 0.024 / 0.043 / 0.063      (exact=True and PRECISION_F32 alike)
The CPU model of the schedule without V_hi x P_lo reaches 3.2 at C = 128, T = 450 (tests/test_attn_exact_host.py).
Every test leaves the default precision mode behind."""
import pytest
import torch

import attn_exact_ref as ar

pytestmark = pytest.mark.gpu

TERMS_OF_MODE = {"bf16x3": "hh+hl+lh", "bf16": "hh", "f16": "hh", "f32": "full", "exact": "full"}
SPLIT_MODES, ALL_MODES = ("bf16x3", "bf16", "f16"), ("bf16x3", "bf16", "f16", "exact", "f32")
CLASSES = ("selector", "group-2-spread", "group-2-packed", "group-4-spread", "group-4-packed", "twin-both")
WIDE_CLASSES = ("selector", "group-2-packed", "group-4-spread", "twin-both")      # at C = 256 / 512, where a case costs the CPU more


@pytest.fixture(autouse=True)
def _default_mode_after(plugin):
    E = plugin.engine
    assert E.get_precision() == E.PRECISION_BF16X3
    yield
    mode = E.get_precision()
    E.set_precision(E.PRECISION_BF16X3)
    assert mode == E.PRECISION_BF16X3, "a test leaked its precision mode"


def _mode(E, mode):
    return E.precision({"bf16x3": E.PRECISION_BF16X3, "bf16": E.PRECISION_BF16, "f16": E.PRECISION_F16, "f32": E.PRECISION_F32,
                        "exact": E.PRECISION_BF16X3}[mode])


def _case(cls, C, Tq, Tk, B=1):
    """the shared case of a class; (e) is asserted where there are keys enough for a fraction to mean something"""
    if cls.startswith("twin"):
        case = ar.twin_case(C, Tq, Tk, B, cls.split("-")[1])
    else:
        n, placement = (1, "spread") if cls == "selector" else (int(cls.split("-")[1]), cls.split("-")[2])
        case = ar.group_case(C, Tq, Tk, B, n, placement)
    if Tk >= 31:
        ar.check_discrimination(case)
    return case


def _nsplit(E, B, C, Tq, Tk, entry):
    """the key-range split of a launch, from the workspace the library asks for: past the three record images it holds
    ns * (B C Tq + 2 B Tq128) floats, and nothing when ns = 1"""
    ws = E.lib().mdtile_vae_attn_ws_size(B, C, Tq) if entry == "attn" else E.lib().mdtile_vae_attn_qk_ws_size(B, C, Tq, Tk)
    Tq128, Tk128 = (Tq + 127) // 128 * 128, (Tk + 127) // 128 * 128
    extra = ws - B * (Tq128 + 2 * Tk128) * C * 4
    per = (B * C * Tq + 2 * B * Tq128) * 4
    assert extra >= 0 and extra % per == 0, (ws, extra, per)
    return extra // per or 1


def _launch(E, cuda, q, k, v, scale, mode, entry="attn", channel_major=False):
    q, k = q.to(cuda), k.to(cuda)
    v = (v.transpose(1, 2).contiguous() if channel_major else v).to(cuda)
    with _mode(E, mode):
        if entry == "qk":
            return E.vae_attn_qk(q, k, v, scale).cpu()
        return E.vae_attn(q, k, v, scale, exact=mode == "exact", v_channel_major=channel_major).cpu()


def _check(plugin, cuda, case, mode, entry="attn"):
    """every v layout the mode takes against the expectation itself (not against the other layout)"""
    E = plugin.engine
    terms = TERMS_OF_MODE[mode]
    want = case.want(terms)
    ns = 1 if terms == "full" else _nsplit(E, case.B, case.C, case.Tq, case.Tk, entry)
    print(f"{case.name} C={case.C} Tq={case.Tq} Tk={case.Tk} B={case.B} {entry} {mode}: key-range split {ns}")
    layouts = (False, True) if entry == "attn" and terms != "full" else (False,)
    for cm in layouts:
        got = _launch(E, cuda, case.q, case.k, case.v, case.scale, mode, entry, cm)
        assert torch.equal(got, want), f"{case.name} {mode} {entry} {'channel' if cm else 'token'}-major v: {case.report(got, terms, ns)}"
    return ns


def _B(T):
    return 2 if T in (33, 129, 450) else 1


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("T", ar.T_SWEEP)
@pytest.mark.parametrize("cls", CLASSES + ("twin-lh", "twin-hl", "twin-ll"))
def test_vae_attn_c128_sweep(plugin, cuda, cls, T, mode):
    """T % 4 == 0 and ragged, below / at / above a key tile and a 128-key block, splits 1 (<= 384), 3 (450), 4 (1000)"""
    _check(plugin, cuda, _case(cls, 128, T, T, _B(T)), mode)


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("cls", WIDE_CLASSES)
@pytest.mark.parametrize("C,T", [(C, T) for C in (256, 512) for T in ar.T_EDGE[C]])
def test_vae_attn_wide_edges(plugin, cuda, C, T, cls, mode):
    _check(plugin, cuda, _case(cls, C, T, T, _B(T)), mode)


QK = [(128,) + s + (cls,) for s in ar.QK_SHAPES for cls in CLASSES] + \
     [(C, Tq, Tk, cls) for C, Tq, Tk in ((256, 64, 200), (512, 300, 1100), (512, 129, 1)) for cls in WIDE_CLASSES]


@pytest.mark.parametrize("mode", SPLIT_MODES)
@pytest.mark.parametrize("C,Tq,Tk,cls", QK)
def test_vae_attn_qk(plugin, cuda, C, Tq, Tk, cls, mode):
    """a band of queries against all keys (token-major v only)"""
    _check(plugin, cuda, _case(cls, C, Tq, Tk, 2 if Tq == 64 else 1), mode, entry="qk")


@pytest.mark.parametrize("mode", ("bf16x3", "bf16", "exact"))
@pytest.mark.parametrize("variant", ("both", "lh", "hl", "ll"))
@pytest.mark.parametrize("C", (128, 256, 512))
def test_twin_tie_break_positions(plugin, cuda, C, variant, mode):
    """each lo term alone responsible for the result, with its channel in every 64-channel slab, both lane halves of a k-step, the first
    and the last k-step of a slab and on the last channel.  "ll": three-term kernels must NOT tell the twins apart, the exact one must."""
    for pos in ar.twin_positions(C):
        case = ar.twin_case(C, 77, 77, 1, variant, pos)
        ar.check_discrimination(case)
        _check(plugin, cuda, case, mode)


def test_every_key_range_split_is_reached(plugin, cuda):
    """over the shapes of the value tests the library picks 1, 2, 3 and 4 key ranges (attn_nsplit at 256 CUs)"""
    E = plugin.engine
    got = {("attn", T): _nsplit(E, 1, 128, T, T, "attn") for T in ar.T_SWEEP}
    got.update({("qk", s): _nsplit(E, 1, 128, s[0], s[1], "qk") for s in ar.QK_SHAPES})
    for key, ns in got.items():
        print(f"{key}: key-range split {ns}")
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    if cus != 256:
        pytest.skip(f"{cus} CUs, not 256: splits reached {sorted(set(got.values()))}")
    assert set(got.values()) == {1, 2, 3, 4}
    for key, ns in ar.SPLIT_EXPECTED.items():
        assert got[key] == ns, (key, got[key], ns)
    assert all(ns == 1 for (entry, T), ns in got.items() if entry == "attn" and T <= 384)


STACKED = [("attn", 128, 450, 450, m) for m in SPLIT_MODES + ("exact",)] + [("attn", 512, 129, 129, m) for m in SPLIT_MODES + ("exact",)] + \
          [("qk", 128, 300, 1100, m) for m in SPLIT_MODES] + [("qk", 256, 1000, 200, m) for m in SPLIT_MODES]      # splits 3, 1, 2, 2


@pytest.mark.parametrize("entry,C,Tq,Tk,mode", STACKED)
def test_stacked_batch_equals_single_images(plugin, cuda, entry, C, Tq, Tk, mode):
    """two images with different targets, codes and values: image b of the stack is the launch of image b alone, and both are the
    expectation -- part / pstat offsets taken with the wrong b read the other image's part"""
    E = plugin.engine
    case = _case("group-2-spread", C, Tq, Tk, 2)
    terms = TERMS_OF_MODE[mode]
    want = case.want(terms)
    assert not torch.equal(want[0], want[1])
    ns = _check(plugin, cuda, case, mode, entry)
    both = _launch(E, cuda, case.q, case.k, case.v, case.scale, mode, entry)
    for b in range(2):
        q, k, v = case.image(b)
        alone = _launch(E, cuda, q, k, v, case.scale, mode, entry)
        assert torch.equal(alone, want[b:b + 1]), f"image {b} alone: {ar.attn_mismatch_report(alone, want[b:b + 1], case.live(terms)[b:b + 1], ns)}"
        assert torch.equal(both[b:b + 1], alone), f"image {b} of the stack differs from its own launch"


@pytest.mark.parametrize("mode", ALL_MODES)
@pytest.mark.parametrize("C,T", ar.GRADED_SHAPES)
def test_graded_vs_fp64_softmax(plugin, cuda, C, T, mode):
    """P is no power of two here: |out - ref| <= tol * sum_j p_j |v_j| per element, tol = 2^-15 (P split to 16 bits 2^-17, P_lo V_lo not
    formed 2^-18, v_exp_f32 2^-23, the rounding of s' below 2^-19: under 2^-16, margin 2) or 2^-7 (P_hi and V_hi at 2^-9 each, margin 2)"""
    E = plugin.engine
    case = ar.graded_case(C, T)
    terms = TERMS_OF_MODE[mode]
    ref, mag = case.reference(terms)
    tol = ar.TOL_ONE if terms == "hh" else ar.TOL_THREE
    for cm in ((False, True) if terms != "full" else (False,)):
        got = _launch(E, cuda, case.q, case.k, case.v, case.scale, mode, "attn", cm).double()
        ratio = float(((got - ref).abs() / (tol * mag)).max())
        print(f"graded C={C} T={T} {mode} {'channel' if cm else 'token'}-major v: max error / bound = {ratio:.4f}")
        assert ratio < 1.0
