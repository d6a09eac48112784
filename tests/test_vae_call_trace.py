"""The engine-call trace of the Tiled VAE hook on CPU: VAEHook (scripts/tilevae.py) driven with tracing subclasses of the torch doubles
(tests/torch_engine.py) must issue, per mode / pair of doubles / switch setting, exactly the sequence of engine and conv calls that is
recorded in tests/golden/vae_call_trace.json -- name, channel counts, input shape and every argument that selects behaviour (which
outputs are wanted, a residual, pending coefficients, `out is x` of gn_apply, the per-image window origins of stacked tiles, the boxes
of crop_store).  The golden was recorded from the commit it names (tests/golden/make_golden_call_trace.py) and is data: a refactor of
the host logic replays the matrix against it, it is never regenerated from the code under test."""
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLUGIN = os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd")
for _p in (ROOT, PLUGIN, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch_engine as te  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "vae_call_trace.json")

LOG = []          # the trace of the run in progress
_INNER = [0]      # > 0 inside a *_stats double: the calls it makes itself are not the hook's


def _shape(t):
    return None if t is None else list(t.shape)


def _log(name, *args):
    if not _INNER[0]:
        LOG.append(json.dumps([name, *args], separators=(",", ":")))


def _origins(v, B):
    return [int(v)] * B if isinstance(v, int) else [int(a) for a in v]


class _TraceConvMixin:
    def __call__(self, x, residual=None, upsample2x=False, token_major=False, exact=False, pre_gn=None):
        _log("conv", self.cin, self.cout, _shape(x), residual is not None, bool(upsample2x), bool(token_major), bool(exact), _shape(pre_gn))
        return super().__call__(x, residual, upsample2x, token_major, exact, pre_gn)

    def call_stats(self, x, pre_gn, residual=None, groups=32):
        _log("call_stats", self.cin, self.cout, _shape(x), _shape(pre_gn), residual is not None, groups)
        _INNER[0] += 1
        try:
            return super().call_stats(x, pre_gn, residual=residual, groups=groups)
        finally:
            _INNER[0] -= 1

    def down2(self, x):
        _log("down2", self.cin, self.cout, _shape(x))
        return super().down2(x)


class TraceConv(_TraceConvMixin, te.TorchConv):
    pass


class TraceConvCounting(_TraceConvMixin, te.TorchConvCounting):
    pass


class TraceConvRec(_TraceConvMixin, te.TorchConvRec):
    def call_rec_stats(self, xrec, residual=None, upsample2x=False, family=0, groups=32):
        _log("call_rec_stats", self.cin, self.cout, list(xrec.shape), residual is not None, bool(upsample2x), family, groups)
        _INNER[0] += 1
        try:
            return super().call_rec_stats(xrec, residual=residual, upsample2x=upsample2x, family=family, groups=groups)
        finally:
            _INNER[0] -= 1

    def call_rec(self, xrec, residual=None, upsample2x=False, want_f32=True, want_rec=False, rec_coef=None, window=None, family=0):
        B = xrec.shape[0]
        win = None if window is None else [_origins(window[0], B), _origins(window[1], B), int(window[2]), int(window[3])]
        _log("call_rec", self.cin, self.cout, list(xrec.shape), residual is not None, bool(upsample2x), bool(want_f32), bool(want_rec),
             _shape(rec_coef), win, family)
        return super().call_rec(xrec, residual=residual, upsample2x=upsample2x, want_f32=want_f32, want_rec=want_rec, rec_coef=rec_coef,
                                window=window, family=family)


class _TraceEngineMixin:
    def tanh(self, x, out=None):
        _log("tanh", _shape(x), out is not None)
        return super().tanh(x, out)

    def crop_store(self, tile, in_bbox, out_bbox, result, is_decoder=True):
        _log("crop_store", _shape(tile), [int(v) for v in in_bbox], [int(v) for v in out_bbox], _shape(result), bool(is_decoder))
        return super().crop_store(tile, in_bbox, out_bbox, result, is_decoder)

    def gn_stats(self, x, groups=32):
        _log("gn_stats", _shape(x), groups)
        return super().gn_stats(x, groups)

    def gn_pool(self, means, vars_, pixels):
        _log("gn_pool", _shape(means), _shape(vars_), [int(p) for p in pixels])
        return super().gn_pool(means, vars_, pixels)

    def gn_coeffs(self, mean, var, gamma, beta, C, groups=32, eps=1e-6):
        _log("gn_coeffs", _shape(mean), _shape(var), gamma is not None, beta is not None, int(C), groups, eps)
        return super().gn_coeffs(mean, var, gamma, beta, C, groups, eps)

    def gn_apply(self, x, mean, var, gamma, beta, groups=32, eps=1e-6, silu=False, out=None):
        _log("gn_apply", _shape(x), _shape(mean), gamma is not None, beta is not None, groups, eps, bool(silu), out is x, out is None)
        return super().gn_apply(x, mean, var, gamma, beta, groups, eps, silu, out)

    def vae_attn(self, q, k, v_tok, scale, **kw):
        _log("vae_attn", _shape(q), _shape(k), _shape(v_tok), sorted(kw.items()))
        return super().vae_attn(q, k, v_tok, scale, **kw)


class TraceEngine(_TraceEngineMixin, te.TorchEngine):
    pass


class TraceEngineRec(_TraceEngineMixin, te.TorchEngineRec):
    def rec_from_f32(self, x, coef=None):
        _log("rec_from_f32", _shape(x), _shape(coef))
        return super().rec_from_f32(x, coef)


# ---- the matrix ----------------------------------------------------------------------------------------------------------------------
MODES = {      # name -> (is_decoder, fast, color_fix, input shape, tile size): the small nets of hostsim.ldm_decoder
    "dec_fast": (True, True, False, (1, 4, 70, 40), 16),        # stacks tiles with different window origins
    "dec_slow": (True, False, False, (1, 4, 36, 44), 16),
    "enc_fast": (False, True, False, (1, 3, 136, 200), 64),
    "enc_slow": (False, False, False, (1, 3, 136, 200), 64),
    "enc_color_fix": (False, True, True, (1, 3, 136, 200), 64),
}
DOUBLES = {"rec": (TraceConvRec, TraceEngineRec), "counting": (TraceConvCounting, TraceEngineRec), "plain": (TraceConv, TraceEngine)}
SWITCHES = ("FUSE_PRE_GN", "REC_PATH", "SLOW_REC", "SLOW_STATS", "LIVE_WINDOW")


def matrix(mode):
    """(doubles, switch turned off alone or None) of every run of one mode."""
    return [(d, off) for d in ("rec", "counting") for off in (None,) + SWITCHES] + [("plain", None)]


def run_key(mode, doubles, off):
    return f"{mode}/{doubles}/{'defaults' if off is None else off + '=0'}"


def trace(mode, doubles, off):
    """The call trace (a list of strings, one per call) of one run."""
    from hostsim import ldm_decoder as ld, stub_host as sh
    sh.install("cpu")
    pl = sh.load_plugin().tilevae
    is_decoder, fast, color_fix, shape, ts = MODES[mode]
    net = (ld.make_decoder if is_decoder else ld.make_encoder)(0, small=True)
    net.original_forward = net.forward
    hook = pl.VAEHook(net, ts, is_decoder=is_decoder, fast_decoder=fast, fast_encoder=fast, color_fix=color_fix)
    conv, engine = DOUBLES[doubles]
    hook.engine, hook._pack, hook._sp_ops = engine(), conv, te.TorchSeqParOps()
    torch.manual_seed(2)
    x = torch.randn(*shape)
    old = {name: getattr(pl, name) for name in SWITCHES}
    del LOG[:]
    try:
        for name in SWITCHES:
            setattr(pl, name, name != off)
        with torch.no_grad():
            hook(x)
    finally:
        for name, v in old.items():
            setattr(pl, name, v)
    out = list(LOG)
    del LOG[:]
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("mode", list(MODES))
def test_engine_call_trace_equals_the_recorded_one(golden, mode):
    entries, traces, runs = golden["entries"], golden["traces"], golden["runs"]
    for doubles, off in matrix(mode):
        key = run_key(mode, doubles, off)
        want = [entries[j] for j in traces[runs[key]]]
        got = trace(mode, doubles, off)
        if got != want:
            n = next((j for j, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            msg = (f"{key}: call {n} of {len(got)} (recorded at {golden['recorded_at']}: {len(want)})\n"
                   f"  recorded: {want[n] if n < len(want) else '<end of trace>'}\n  now:      {got[n] if n < len(got) else '<end of trace>'}")
            print(msg)
            pytest.fail(msg)
