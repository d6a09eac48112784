"""Cross-faded tile borders of Tiled VAE, host side (no GPU): the invariants of the numpy restatement (tests/seam_ref.py), the host's
legality function against hand-made grids, the --mdtile-vae-seam-blend wiring, and the hook on the torch doubles of tests/torch_engine.py
with vae_assemble_blend implemented by the restatement."""
import argparse
import importlib.util
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

import seam_cases as sc
import seam_ref as sr


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- the restatement's own invariants -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(sc.LEGAL))
def test_weights_sum_to_D_and_every_pixel_has_one_rule(case):
    """Integer weights sum to D at every pixel of every band; outside the bands exactly one tile contributes; the runs cover the result
    exactly once; every weight is odd x odd, positive and below 2^24."""
    xs, ys, margin, is_dec, band, (N, C) = sc.LEGAL[case]
    RH, RW = sc.result_size(sc.LEGAL[case])
    tab = sc.table(xs, ys, margin, is_dec, 1, 1)
    rows, cols = len(ys) - 1, len(xs) - 1
    assert sr.check_grid(tab, rows, cols, RH, RW, band, is_dec) is None
    cover = np.zeros((RH, RW), dtype=np.int64)
    mask = sr.band_mask(tab, rows, cols, RH, RW, band)
    for y0, y1, x0, x1, terms, D in sr.contributions(tab, rows, cols, band):
        cover[y0:y1, x0:x1] += 1
        if D == 1:
            assert len(terms) == 1 and terms[0][1] is None and not mask[y0:y1, x0:x1].any()
            ob = tab[terms[0][0]][2]
            assert ob[0] <= x0 and x1 <= ob[1] and ob[2] <= y0 and y1 <= ob[3], "outside the bands the owner is the tile whose out box holds the pixel"
            continue
        assert D in (4 * band, 16 * band * band) and len(terms) == (2 if D == 4 * band else 4) and mask[y0:y1, x0:x1].all()
        total = sum(w for _, w in terms)
        assert (total == D).all()
        for _, w in terms:
            assert (w % 2 == 1).all() and w.min() >= 1 and w.max() < 2 ** 24
    assert (cover == 1).all()
    a1, a2 = sr.ramp(band)
    assert (a1 + a2 == 4 * band).all() and a2[0] == 1 and a2[-1] == 4 * band - 1 and (a1 == a2[::-1]).all()


@pytest.mark.parametrize("case", list(sc.LEGAL))
def test_tiles_cut_from_one_image_of_small_integers_give_that_image(case):
    """All tiles agree (cut from one common image of small integers): sum w v = D v exactly, the division is exact -- the image, bit for bit."""
    xs, ys, margin, is_dec, band, (N, C) = sc.LEGAL[case]
    RH, RW = sc.result_size(sc.LEGAL[case])
    rng = np.random.RandomState(3)
    image = rng.randint(-8, 9, size=(N, C, RH, RW)).astype(np.float32)
    tab = sc.table(xs, ys, margin, is_dec, N, C, common=image)
    got = sr.assemble_blend(tab, len(ys) - 1, len(xs) - 1, RH, RW, band, is_dec)
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(image))
    assert np.array_equal(_bits(sr.assemble_plain(tab, RH, RW, is_dec)), _bits(image))


def test_outside_the_bands_the_restatement_is_the_plain_crop_bit_for_bit():
    xs, ys, margin, is_dec, band, (N, C) = sc.LEGAL["3x3_touch"]
    RH, RW = sc.result_size(sc.LEGAL["3x3_touch"])
    tab = sc.table(xs, ys, margin, is_dec, N, C, seed=4, special_band=band)
    got, plain = sr.assemble_blend(tab, 3, 3, RH, RW, band, is_dec), sr.assemble_plain(tab, RH, RW, is_dec)
    m = sr.band_mask(tab, 3, 3, RH, RW, band)
    assert m.any() and not m.all()
    assert np.array_equal(_bits(got)[:, :, ~m], _bits(plain)[:, :, ~m])
    ok = ~np.isnan(got) & ~np.isnan(plain)
    assert (got[:, :, m][ok[:, :, m]] != plain[:, :, m][ok[:, :, m]]).any(), "the bands changed nothing"


# ---- legality -----------------------------------------------------------------------------------------------------------------------
def _host_reason(tv, tab, RH, RW, band, is_dec):
    return tv.seam_grid([ib for _, ib, _ in tab], [ob for _, _, ob in tab], RH, RW, band, is_dec)


@pytest.mark.parametrize("case", list(sc.LEGAL))
def test_host_legality_admits_the_legal_grids(plugin, case):
    xs, ys, margin, is_dec, band, _ = sc.LEGAL[case]
    RH, RW = sc.result_size(sc.LEGAL[case])
    tab = sc.table(xs, ys, margin, is_dec, 1, 1)
    assert _host_reason(plugin.tilevae, tab, RH, RW, band, is_dec) == ((len(ys) - 1, len(xs) - 1), None)


@pytest.mark.parametrize("case", list(sc.ILLEGAL) + ["hole"])
def test_host_legality_names_the_reason(plugin, case):
    """A band wider than a tile, bands overlapping, a margin smaller than b, a grid with a hole (and band < 1): refused, and the host
    function, the restatement and the expected words agree."""
    import re
    if case == "hole":
        xs, ys, margin, is_dec, band, _ = sc.LEGAL["2x2_b1"]
        tab, why = sc.with_hole(sc.table(xs, ys, margin, is_dec, 1, 1)), "grid"
    else:
        xs, ys, margin, is_dec, band, why = sc.ILLEGAL[case]
        tab = sc.table(xs, ys, margin, is_dec, 1, 1)
    RH, RW = ys[-1], xs[-1]
    assert sr.check_grid(tab, len(ys) - 1, len(xs) - 1, RH, RW, band, is_dec) == why
    grid, text = _host_reason(plugin.tilevae, tab, RH, RW, band, is_dec)
    assert grid is None and re.search(sc.REASON_TEXT[why], text), text
    with pytest.raises(ValueError, match=why):
        sr.assemble_blend(tab, len(ys) - 1, len(xs) - 1, RH, RW, band, is_dec)


def test_split_tiles_grids_are_legal_up_to_the_padding():
    """The two real tables of the GPU test, on the CPU: latent 64 x 64 / tile 16 (3 x 3: out extents 216 / 128 / 168, so b = 64 makes the
    interior tile's bands touch) and 96 x 80 / tile 32 (3 x 2: 344 / 296 wide, 344 / 256 / 168 tall, b = 88 = the padding); margins 88."""
    from hostsim import stub_host as sh
    from oracle import vae_oracle as vo
    tv = sh.load_plugin().tilevae
    for (h, w, ts, band), (ws, hs) in (((64, 64, 16, 64), ([216, 128, 168], [216, 128, 168])), ((96, 80, 32, 88), ([344, 296], [344, 256, 168]))):
        ins, outs = vo.split_tiles(h, w, ts, True)
        assert tv.seam_grid(ins, outs, h * 8, w * 8, band, True) == ((len(hs), len(ws)), None)
        assert [o[1] - o[0] for o in outs[:len(ws)]] == ws and [outs[r * len(ws)][3] - outs[r * len(ws)][2] for r in range(len(hs))] == hs
        for i, (ib, ob) in enumerate(zip(ins, outs)):
            r, c = divmod(i, len(ws))
            assert sr.margins(ib, ob, True) == (88 * (c > 0), 88 * (c < len(ws) - 1), 88 * (r > 0), 88 * (r < len(hs) - 1))
    assert "margin" in tv.seam_grid(ins, outs, 96 * 8, 80 * 8, 89, True)[1]           # one px past the padding
    ins, outs = vo.split_tiles(64, 64, 16, True)
    assert "overlap" in tv.seam_grid(ins, outs, 512, 512, 65, True)[1]               # the 128-px interior tile holds two bands of 64 at most


# ---- option wiring ------------------------------------------------------------------------------------------------------------------
def test_preload_registers_the_option():
    spec = importlib.util.spec_from_file_location("mdtile_preload_seam", os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd", "preload.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = argparse.ArgumentParser()
    mod.preload(parser)
    assert parser.parse_args(["--mdtile-vae-seam-blend", "24"]).mdtile_vae_seam_blend == 24
    assert parser.parse_args([]).mdtile_vae_seam_blend is None
    text = parser.format_help()
    assert "1-88" in text and "16-32" in text and "PX" in text


class _Net(torch.nn.Module):
    def forward(self, x):
        return x


def _process(plugin, monkeypatch, value):
    import modules.shared as shared
    enc, dec = _Net(), _Net()
    p = SimpleNamespace(sd_model=SimpleNamespace(first_stage_model=SimpleNamespace(encoder=enc, decoder=dec)), extra_generation_params={})
    if value is not None:
        monkeypatch.setattr(shared.cmd_opts, "mdtile_vae_seam_blend", value, raising=False)
    s = plugin.tilevae.Script()
    s.process(p, True, 3072, 256, True, True, True, False)
    hooks = (dec.forward, enc.forward)
    s.postprocess(p, None, True)
    return p, hooks


def test_process_sets_the_decoder_hook_only(plugin, monkeypatch, capsys):
    p, (dec, enc) = _process(plugin, monkeypatch, 24)
    assert dec.seam_blend == 24 and enc.seam_blend == 0
    assert p.extra_generation_params == {"Tiled VAE seam blend": 24}
    assert "seam" not in capsys.readouterr().out


def test_process_without_the_option_changes_nothing(plugin, monkeypatch, capsys):
    p, (dec, enc) = _process(plugin, monkeypatch, None)
    assert dec.seam_blend == 0 and enc.seam_blend == 0 and p.extra_generation_params == {}
    assert "seam" not in capsys.readouterr().out


@pytest.mark.parametrize("value", [0, -4, 89, 1000])
def test_process_ignores_a_value_out_of_range_with_one_line(plugin, monkeypatch, capsys, value):
    p, (dec, enc) = _process(plugin, monkeypatch, value)
    assert dec.seam_blend == 0 and enc.seam_blend == 0 and p.extra_generation_params == {}
    lines = [l for l in capsys.readouterr().out.splitlines() if "--mdtile-vae-seam-blend" in l]
    assert len(lines) == 1 and lines[0].startswith("[Tiled VAE]") and "ignored" in lines[0]


def test_ui_and_process_orders_are_unchanged(plugin):
    import inspect
    names = list(inspect.signature(plugin.tilevae.Script.process).parameters)
    assert names == ["self", "p", "enabled", "encoder_tile_size", "decoder_tile_size", "vae_to_gpu", "fast_decoder", "fast_encoder", "color_fix"]


# ---- the hook on the torch doubles --------------------------------------------------------------------------------------------------
def _doubles():
    import torch_engine as te

    class SeamEngine(te.TorchEngineRec):
        """The record-path doubles plus the two assemblies: vae_assemble by crop_store, vae_assemble_blend by the restatement."""

        def __init__(self):
            self.blend_calls, self.plain_calls = [], []

        def vae_assemble(self, tiles, result, is_decoder=True):
            self.plain_calls.append([(tuple(ib), tuple(ob)) for _, ib, ob in tiles])
            for t, ib, ob in tiles:
                self.crop_store(t, ib, ob, result, is_decoder)

        def vae_assemble_blend(self, tiles, rows, cols, result, band, is_decoder=True):
            self.blend_calls.append(SimpleNamespace(tiles=[(t.clone(), tuple(ib), tuple(ob)) for t, ib, ob in tiles], rows=rows, cols=cols, band=band,
                                                    is_decoder=is_decoder))
            tab = [(t.numpy(), tuple(ib), tuple(ob)) for t, ib, ob in tiles]
            result.copy_(torch.from_numpy(sr.assemble_blend(tab, rows, cols, result.shape[2], result.shape[3], band, is_decoder)))

    return te, SeamEngine


def _hook(fast, seam, rec=True):
    from hostsim import stub_host as sh, ldm_decoder as ld
    te, SeamEngine = _doubles()
    sh.install("cpu")
    pl = sh.load_plugin()
    net = ld.make_decoder(0, small=True)
    net.original_forward = net.forward
    hook = pl.tilevae.VAEHook(net, 16, is_decoder=True, fast_decoder=fast, fast_encoder=fast, color_fix=False)
    hook.engine, hook._pack, hook._sp_ops = SeamEngine(), (te.TorchConvRec if rec else te.TorchConv), te.TorchSeqParOps()
    hook.seam_blend = seam
    return hook, pl


H, W = 40, 56          # 2 x 3 tiles at tile 16: out extents 216 / 128 / 104 px wide, 216 / 104 px tall, 88 px of padding between them


@pytest.fixture(scope="module")
def z():
    torch.manual_seed(2)
    return torch.randn(1, 4, H, W)


@pytest.fixture(scope="module")
def plain_images(z):
    """The option-off images, once per mode -- and vae_assemble_blend is never called without the option."""
    out = {}
    for fast in (True, False):
        hook, _ = _hook(fast, 0)
        with torch.no_grad():
            out[fast] = hook(z)
        assert hook.engine.blend_calls == [] and hook.engine.plain_calls == []
    return out


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "slow"])
def test_hook_keeps_the_tiles_and_assembles_with_the_blend(z, plain_images, fast, capsys):
    from oracle import vae_oracle as vo
    band = 16
    hook, pl = _hook(fast, band)
    with torch.no_grad():
        got = hook(z)
    E = hook.engine
    assert len(E.blend_calls) == 1 and E.plain_calls == []
    call = E.blend_calls[0]
    ins, outs = vo.split_tiles(H, W, 16, True)
    assert (call.rows, call.cols, call.band, call.is_decoder) == (2, 3, band, True) and len(call.tiles) == len(outs) == 6
    assert [ob for _, _, ob in call.tiles] == [tuple(o) for o in outs], "kept tiles reach the assembly in row-major order"
    g = -(-band // 8)
    for i, (t, ib, ob) in enumerate(call.tiles):
        r, c = divmod(i, 3)
        ml, mr, mt, mb = sr.margins(ib, ob, True)
        assert tuple(t.shape[2:]) == ((ib[3] - ib[2]) * 8, (ib[1] - ib[0]) * 8)
        for m, has in ((ml, c > 0), (mr, c < 2), (mt, r > 0), (mb, r < 1)):
            assert m >= band if has else m >= 0
            if fast and has:     # live windows: the valid rectangle grown by ceil(b / 8), then by the 1 latent px behind the last upsample conv
                assert m == 8 * (g + 1), (i, ib, ob)
        if not fast:
            assert tuple(ib) == tuple(ins[i])
    tab = [(t.numpy(), ib, ob) for t, ib, ob in call.tiles]
    want = sr.assemble_blend(tab, 2, 3, H * 8, W * 8, band, True)
    assert np.array_equal(_bits(got.numpy()), _bits(want))
    m = torch.from_numpy(sr.band_mask(tab, 2, 3, H * 8, W * 8, band))
    plain = plain_images[fast]
    # (the doubles' CPU convs pick their blocking by plane size: a tile narrowed differently agrees to rounding only; bitwise on the GPU)
    tol = 0.0 if not fast else 1e-5 * plain.abs().max().item()
    assert (got[:, :, ~m] - plain[:, :, ~m]).abs().max().item() <= tol
    assert not torch.equal(got[:, :, m], plain[:, :, m]), "the bands changed nothing"
    assert "seam" not in capsys.readouterr().out


def test_hook_falls_back_when_the_grid_does_not_admit_the_band(z, plain_images, capsys):
    hook, _ = _hook(True, 88)            # the 128-px interior column cannot hold two bands of 88 px
    with torch.no_grad():
        got = hook(z)
    assert hook.engine.blend_calls == [] and hook.engine.plain_calls == []
    assert torch.equal(got, plain_images[True])
    lines = [l for l in capsys.readouterr().out.splitlines() if "seam blend" in l]
    assert len(lines) == 1 and lines[0].startswith("[Tiled VAE]") and "overlap" in lines[0]


def test_interrupted_call_returns_the_partial_image_without_the_blend(z, plain_images, capsys, monkeypatch):
    import modules.shared as shared
    hook, pl = _hook(True, 16)
    finish = pl.tilevae.VAEHook._Lane.finish
    done = []

    def finish_then_interrupt(self, i):
        finish(self, i)
        done.append(i)
        shared.state.interrupted = True

    monkeypatch.setattr(pl.tilevae.VAEHook._Lane, "finish", finish_then_interrupt)
    try:
        with torch.no_grad():
            got = hook(z)
    finally:
        shared.state.interrupted = False
    E = hook.engine
    assert 0 < len(done) < 6 and E.blend_calls == [] and len(E.plain_calls) == 1 and len(E.plain_calls[0]) == len(done)
    lines = [l for l in capsys.readouterr().out.splitlines() if "seam blend" in l]
    assert len(lines) == 1 and lines[0].startswith("[Tiled VAE]") and "interrupted" in lines[0]
    from oracle import vae_oracle as vo
    _, outs = vo.split_tiles(H, W, 16, True)
    tol = 1e-5 * plain_images[True].abs().max().item()
    for i, ob in enumerate(outs):             # upstream's partial image: the finished tiles pasted, zeros elsewhere
        box = got[:, :, ob[2]:ob[3], ob[0]:ob[1]]
        if i in done:
            assert (box - plain_images[True][:, :, ob[2]:ob[3], ob[0]:ob[1]]).abs().max().item() <= tol
        else:
            assert not box.any()


def test_shard_with_the_option_raises(z):
    hook, _ = _hook(True, 16)
    hook.shard = (0, 2)
    with pytest.raises(RuntimeError, match=r"(?s)seam_blend.*shard"):
        with torch.no_grad():
            hook(z)


def test_encoder_hook_ignores_the_setting(capsys):
    from hostsim import stub_host as sh, ldm_decoder as ld
    te, SeamEngine = _doubles()
    sh.install("cpu")
    pl = sh.load_plugin()
    outs = []
    for seam in (0, 16):
        net = ld.make_encoder(0, small=True)
        net.original_forward = net.forward
        hook = pl.tilevae.VAEHook(net, 64, is_decoder=False, fast_decoder=True, fast_encoder=True, color_fix=False)
        hook.engine, hook._pack, hook._sp_ops = SeamEngine(), te.TorchConv, te.TorchSeqParOps()
        hook.seam_blend = seam
        torch.manual_seed(4)
        with torch.no_grad():
            outs.append(hook(torch.randn(1, 3, 136, 200)))
        assert hook.engine.blend_calls == [] and hook.engine.plain_calls == []
    assert torch.equal(outs[0], outs[1]) and "seam" not in capsys.readouterr().out
