"""The colour fix (mdtile_colorfix_wavelet / mdtile_hist_u8 / mdtile_lut_u8, mdtile.adain_lut, tile_utils.utils.color_fix_image,
--mdtile-color-fix), the checks that need no GPU: the restatements of tests/colorfix_ref.py agree with each other and tell the wrong variant
apart, the library exports the entry points and refuses bad arguments, the host-side AdaIN table equals the per-pixel float64 restatement, the
option is registered, and the routing of Script.postprocess_image / color_fix_image -- with the engine calls replaced by the restatement."""
import argparse
import importlib.util
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from hostsim import stub_host as sh
import colorfix_ref as cr
import resample_ref as rr
from colorfix_helpers import apply_lut, lanczos_upscalers, photo, process, set_option

SYMBOLS = ["mdtile_colorfix_wavelet_ws_size", "mdtile_colorfix_wavelet", "mdtile_hist_u8", "mdtile_lut_u8"]
PKG = os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd")


# ---- the definition --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cr.cases(), ids=cr.case_id)
def test_literal_definition_equals_the_integer_form(case):
    content, style = cr.make_pair(*case)
    lit, integer = cr.wavelet_literal(content, style), cr.wavelet_int(content, style)
    assert integer.dtype == np.uint8 and integer.shape == content.shape
    assert int((lit != integer).sum()) == 0
    assert np.array_equal(cr.wavelet_int(content, content), content)          # style == content returns the content
    assert np.array_equal(cr.wavelet_int(style, style), style)


def test_pad_once_is_another_function():
    """Padding once by 31 instead of clamping every level: the random cases of at least 2 x 3 all separate the two."""
    seen = 0
    for case in cr.cases():
        (h, w, _), kind = case
        if kind != "random" or h * w < 6:
            continue
        content, style = cr.make_pair(*case)
        differ = int((cr.wavelet_pad_once(content, style) != cr.wavelet_int(content, style)).sum())
        print(f"{cr.case_id(case)}: pad-once changes {differ} of {content.size} bytes")
        assert differ > 0
        seen += 1
    assert seen == 8
    # where no index is ever clamped twice the two agree: a 1 x 1 image
    c, s = cr.make_pair((1, 1, 1), "random")
    assert np.array_equal(cr.wavelet_pad_once(c, s), cr.wavelet_int(c, s))


# ---- the library -----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points(built_lib):
    src = open(os.path.join(ROOT, "include", "mdtile.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], capture_output=True, text=True).stdout
    public = [l.split()[-1] for l in out.splitlines() if " T " in l]
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, src), f"include/mdtile.h does not declare {s}"
        assert s in public, f"libmdtile.so does not export {s}"
        assert s in built_lib.exported_symbols()
    for name in ("colorfix_wavelet", "hist_u8", "adain_lut", "lut_u8", "colorfix_adain"):
        assert callable(getattr(built_lib, name))


def test_bad_arguments(built_lib):
    L = built_lib.lib()
    assert L.mdtile_colorfix_wavelet_ws_size(8192, 8192, 3) == 8192 * 8192 * 3 * 4
    assert L.mdtile_colorfix_wavelet_ws_size(16, 16, 2) == 0 and L.mdtile_colorfix_wavelet_ws_size(0, 16, 3) == 0
    assert L.mdtile_colorfix_wavelet_ws_size(32768, 65536, 1) == 0                 # 2^31 bytes
    one = 4096                                                                     # refused before anything touches the device

    def err(rc):
        return rc, L.mdtile_last_error().decode()

    rc, msg = err(L.mdtile_colorfix_wavelet(one, one, one, 16, 16, 2, one, None))
    assert rc == built_lib.E_ARG and "channels" in msg
    rc, msg = err(L.mdtile_colorfix_wavelet(one, one, one, 32768, 65536, 1, one, None))
    assert rc == built_lib.E_ARG and "2^31" in msg
    rc, msg = err(L.mdtile_colorfix_wavelet(one, one, one, 16, 0, 3, one, None))
    assert rc == built_lib.E_ARG and "sizes" in msg
    rc, msg = err(L.mdtile_colorfix_wavelet(one, None, one, 16, 16, 3, one, None))
    assert rc == built_lib.E_ARG and "null" in msg
    rc, msg = err(L.mdtile_colorfix_wavelet(one, one, one, 16, 16, 3, None, None))
    assert rc == built_lib.E_ARG and "null" in msg
    rc, msg = err(L.mdtile_colorfix_wavelet(one, one, one, 16, 16, 3, one + 4, None))
    assert rc == built_lib.E_ARG and "aligned" in msg
    rc, msg = err(L.mdtile_hist_u8(one, 16, 16, 4, one, None))
    assert rc == built_lib.E_ARG and "channels" in msg
    assert L.mdtile_hist_u8(one, 16, 16, 3, None, None) == built_lib.E_ARG
    assert L.mdtile_hist_u8(one, -1, 16, 3, one, None) == built_lib.E_ARG
    rc, msg = err(L.mdtile_lut_u8(one, 16, 16, 2, one, one, None))
    assert rc == built_lib.E_ARG and "channels" in msg
    assert L.mdtile_lut_u8(one, 16, 16, 3, None, one, None) == built_lib.E_ARG
    assert L.mdtile_lut_u8(one, 65536, 32768, 1, one, one, None) == built_lib.E_ARG


def test_cpu_tensors_are_refused(built_lib):
    img = torch.zeros(16, 16, 3, dtype=torch.uint8)
    with pytest.raises(built_lib.MdtileError, match="no CPU fallback"):
        built_lib.colorfix_wavelet(img, img)
    with pytest.raises(built_lib.MdtileError, match="no CPU fallback"):
        built_lib.hist_u8(img)
    with pytest.raises(built_lib.MdtileError, match="no CPU fallback"):
        built_lib.lut_u8(img[:, :, 0], np.zeros((1, 256), np.uint8))
    with pytest.raises(built_lib.MdtileError, match="no CPU fallback"):
        built_lib.colorfix_adain(img, img)


# ---- AdaIN on the host -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cr.cases(), ids=cr.case_id)
def test_adain_lut_equals_the_per_pixel_restatement(built_lib, case):
    content, style = cr.make_pair(*case)
    lut = built_lib.adain_lut(cr.hist(content), cr.hist(style))
    assert lut.dtype == np.uint8 and lut.shape == (case[0][2], 256)
    assert np.array_equal(apply_lut(lut, content), cr.adain_pixels(content, style))


def test_adain_lut_edge_cases(built_lib):
    # n == 1: the variance is 0 by definition, both deviations sqrt(0.65025), the table a shift by style - content
    lut = built_lib.adain_lut(cr.hist(np.array([[7]], np.uint8)), cr.hist(np.array([[200]], np.uint8)))
    assert lut[0, 7] == 200 and lut[0, 0] == 193 and lut[0, 255] == 255 and (np.diff(lut[0].astype(int)) >= 0).all()
    # a flat content channel under a busy style: finite, clamped, the flat value lands on the style's mean
    flat = np.full((40, 50, 3), 90, np.uint8)
    style = cr.make_pair((40, 50, 3), "random")[1]
    lut = built_lib.adain_lut(cr.hist(flat), cr.hist(style))
    want = cr.adain_pixels(flat, style)
    assert np.array_equal(apply_lut(lut, flat), want)
    for ch in range(3):
        assert int(want[0, 0, ch]) == int(np.floor(cr.channel_stats(style[:, :, ch])[0] + 0.5))
        assert lut[ch, 0] == 0 and lut[ch, 255] == 255           # the steep table saturates away from the flat value
    # a style of another size: only its statistics matter
    content, _ = cr.make_pair((17, 33, 3), "random")
    small = cr.make_pair((5, 9, 3), "ramps")[1]
    assert np.array_equal(apply_lut(built_lib.adain_lut(cr.hist(content), cr.hist(small)), content), cr.adain_pixels(content, small))
    # tensors and lists are taken as well; shapes are checked
    h = cr.hist(content)
    assert np.array_equal(built_lib.adain_lut(torch.from_numpy(h), h.tolist()), built_lib.adain_lut(h, h))
    with pytest.raises(built_lib.MdtileError):
        built_lib.adain_lut(h, h[:1])
    with pytest.raises(built_lib.MdtileError):
        built_lib.adain_lut(np.zeros((1, 256), np.int64), np.zeros((1, 256), np.int64))


# ---- the option ------------------------------------------------------------------------------------------------------------------------------
def test_preload_registers_the_color_fix_option():
    spec = importlib.util.spec_from_file_location("mdtile_preload_color_fix", os.path.join(PKG, "preload.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = argparse.ArgumentParser()
    mod.preload(parser)
    assert parser.parse_args([]).mdtile_color_fix is None
    for v in ("wavelet", "adain"):
        assert parser.parse_args(["--mdtile-color-fix", v]).mdtile_color_fix == v
    action = [a for a in parser._actions if "--mdtile-color-fix" in a.option_strings][0]
    assert list(action.choices) == ["wavelet", "adain"]
    with pytest.raises(SystemExit):
        parser.parse_args(["--mdtile-color-fix", "histogram"])


# ---- routing ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def engine_calls(plugin, monkeypatch):
    """The engine calls color_fix_image makes, replaced by the restatements on CPU tensors; `calls` lists (name, shapes ...) in order."""
    calls = []
    E = plugin.engine

    def wavelet(content, style):
        calls.append(("wavelet", tuple(content.shape), tuple(style.shape), style))
        return torch.from_numpy(cr.wavelet_int(content.cpu().numpy(), style.cpu().numpy()))

    def adain(content, style):
        calls.append(("adain", tuple(content.shape), tuple(style.shape), style))
        return torch.from_numpy(cr.adain_pixels(content.cpu().numpy(), style.cpu().numpy()))

    def resize(t, size, filt):
        calls.append(("resize", tuple(t.shape), (int(size[0]), int(size[1])), int(filt)))
        return torch.from_numpy(rr.resize(t.cpu().numpy(), int(size[0]), int(size[1]), int(filt)))

    monkeypatch.setattr(E, "colorfix_wavelet", wavelet)
    monkeypatch.setattr(E, "colorfix_adain", adain)
    monkeypatch.setattr(E, "resize_u8", resize)
    uploads = []
    real_upload = plugin.utils.image_to_device
    monkeypatch.setattr(plugin.utils, "image_to_device", lambda image: uploads.append(image) or real_upload(image))
    assert plugin.utils.mdtile is E
    return SimpleNamespace(calls=calls, uploads=uploads)


def test_postprocess_image_does_nothing_unless_asked(plugin, engine_calls, monkeypatch):
    pytest.importorskip("PIL")
    s = plugin.tilediffusion.Script()
    result, init = photo(64, 48, seed=1), photo(64, 48)

    def run(p, enabled):
        pp = SimpleNamespace(image=result)
        s.postprocess_image(p, pp, enabled)
        return pp.image

    img2img = SimpleNamespace(init_images=[init])
    set_option(monkeypatch, None)
    assert run(img2img, True) is result                                    # option unset
    _, shared = sh.host()
    monkeypatch.delattr(shared.cmd_opts, "mdtile_color_fix")               # a host that never heard of the option
    assert run(img2img, True) is result
    set_option(monkeypatch, "wavelet")
    assert run(SimpleNamespace(), True) is result                          # txt2img: no init images at all
    assert run(SimpleNamespace(init_images=[]), True) is result
    assert run(SimpleNamespace(init_images=None), True) is result
    assert run(img2img, False) is result                                   # the script is disabled
    assert engine_calls.calls == [] and engine_calls.uploads == []
    fixed = run(img2img, True)
    assert fixed is not result and [c[0] for c in engine_calls.calls] == ["wavelet"]
    assert np.array_equal(np.asarray(fixed), cr.wavelet_int(np.asarray(result), np.asarray(init)))


@pytest.mark.parametrize("mode", ["wavelet", "adain"])
def test_kept_tensor_is_used_only_for_its_image(plugin, engine_calls, mode):
    pytest.importorskip("PIL")
    U = plugin.utils
    result, init, other = photo(64, 48, seed=1), photo(64, 48), photo(64, 48, seed=2)
    kept = torch.from_numpy(np.asarray(init).copy())
    want = (cr.wavelet_int if mode == "wavelet" else cr.adain_pixels)(np.asarray(result), np.asarray(init))

    got = U.color_fix_image(result, init, mode, (init, kept))
    assert engine_calls.uploads == [result]                                # the result goes up once, the style not at all
    assert engine_calls.calls[-1][3] is kept and len(engine_calls.calls) == 1
    assert got.mode == "RGB" and got.size == result.size and np.array_equal(np.asarray(got), want)

    del engine_calls.uploads[:]
    got = U.color_fix_image(result, init, mode, (other, kept))             # the kept bytes belong to another image: upload
    assert engine_calls.uploads == [result, init] and engine_calls.calls[-1][3] is not kept
    assert np.array_equal(np.asarray(got), want)

    del engine_calls.uploads[:]
    got = U.color_fix_image(result, init, mode)                            # nothing kept
    assert engine_calls.uploads == [result, init] and np.array_equal(np.asarray(got), want)
    assert [c[0] for c in engine_calls.calls] == [mode] * 3


def test_style_of_another_size(plugin, engine_calls):
    pytest.importorskip("PIL")
    U = plugin.utils
    result, init = photo(64, 48, seed=1), photo(40, 30)
    got = U.color_fix_image(result, init, "wavelet")
    assert engine_calls.calls[0] == ("resize", (30, 40, 3), (48, 64), rr.LANCZOS)          # once, Lanczos
    assert [c[:3] for c in engine_calls.calls[1:]] == [("wavelet", (48, 64, 3), (48, 64, 3))]
    style = rr.resize(np.asarray(init), 48, 64, rr.LANCZOS)
    assert np.array_equal(np.asarray(got), cr.wavelet_int(np.asarray(result), style))
    del engine_calls.calls[:]
    got = U.color_fix_image(result, init, "adain")                         # statistics only: never resized
    assert [c[:3] for c in engine_calls.calls] == [("adain", (48, 64, 3), (30, 40, 3))]
    assert np.array_equal(np.asarray(got), cr.adain_pixels(np.asarray(result), np.asarray(init)))
    # a kept tensor of another size is resized from the device copy, without an upload of the style
    del engine_calls.calls[:], engine_calls.uploads[:]
    kept = torch.from_numpy(np.asarray(init).copy())
    U.color_fix_image(result, init, "wavelet", (init, kept))
    assert engine_calls.uploads == [result] and [c[0] for c in engine_calls.calls] == ["resize", "wavelet"]


def test_modes(plugin, engine_calls):
    pytest.importorskip("PIL")
    U = plugin.utils
    # a grey result under an RGB init image: the style is converted, and its kept RGB bytes are of no use
    result, init = photo(64, 48, "L", seed=1), photo(64, 48)
    kept = torch.from_numpy(np.asarray(init).copy())
    got = U.color_fix_image(result, init, "wavelet", (init, kept))
    assert got.mode == "L" and engine_calls.calls[-1][1:3] == ((48, 64), (48, 64)) and engine_calls.calls[-1][3] is not kept
    assert np.array_equal(np.asarray(got), cr.wavelet_int(np.asarray(result), np.asarray(init.convert("L"))))
    # an RGBA init image under an RGB result
    rgba = photo(64, 48, "RGBA")
    got = U.color_fix_image(photo(64, 48, seed=1), rgba, "adain")
    assert got.mode == "RGB" and np.array_equal(np.asarray(got), cr.adain_pixels(np.asarray(photo(64, 48, seed=1)), np.asarray(rgba.convert("RGB"))))
    # results in any other mode come back untouched, without a call
    n = len(engine_calls.calls)
    for mode in ("RGBA", "P", "I;16"):
        odd = photo(64, 48).convert(mode) if mode != "I;16" else photo(64, 48, "L").convert("I;16")
        assert U.color_fix_image(odd, init, "wavelet") is odd
    assert len(engine_calls.calls) == n
    with pytest.raises(ValueError):
        U.color_fix_image(photo(64, 48), init, "histogram")


@pytest.mark.parametrize("option", [None, "wavelet", "adain"])
def test_infotext_key_only_under_the_condition(plugin, monkeypatch, option):
    pytest.importorskip("PIL")
    set_option(monkeypatch, option)
    key = "Tiled Diffusion color fix"
    # img2img, enabled
    p = sh.make_processing(512, 320, init_images=[photo(520, 328)], extra_generation_params={"Seed": 1})
    s = process(plugin, p)
    try:
        assert (p.extra_generation_params.get(key) == option) and ((key in p.extra_generation_params) == (option is not None))
    finally:
        s.postprocess(p, None, True)
    # an image that fits one tile: process has nothing to tile, the fix still runs on it, so the key is there
    p = sh.make_processing(64, 64, init_images=[photo(64, 64)], extra_generation_params=None)
    s = process(plugin, p)
    try:
        assert ((p.extra_generation_params or {}).get(key) == option)
    finally:
        s.postprocess(p, None, True)
    # txt2img, and a disabled script
    p = sh.make_processing(2048, 2048, extra_generation_params={})
    s = process(plugin, p)
    try:
        assert key not in p.extra_generation_params
    finally:
        s.postprocess(p, None, True)
    p = sh.make_processing(512, 320, init_images=[photo(520, 328)], extra_generation_params={})
    process(plugin, p, enabled=False)
    assert p.extra_generation_params == {}


def test_process_then_postprocess_image_then_postprocess(plugin, engine_calls, monkeypatch):
    """The whole order of a job with the built-in Lanczos upscaler: process keeps the upscaled bytes, postprocess_image takes them as the style
    (no second upload), postprocess drops them."""
    pytest.importorskip("PIL")
    _, shared = sh.host()
    set_option(monkeypatch, "wavelet")
    monkeypatch.setattr(shared, "sd_upscalers", lanczos_upscalers())
    first = photo(128, 96)
    p = sh.make_processing(128, 96, init_images=[first], extra_generation_params={})
    s = process(plugin, p, "Lanczos", 2)
    try:
        init = p.init_images[0]
        assert init.size == (256, 192) and p.init_image_bytes_md[0] is init
        result = photo(256, 192, seed=5)
        pp = SimpleNamespace(image=result)
        del engine_calls.calls[:], engine_calls.uploads[:]
        s.postprocess_image(p, pp, True)
        assert engine_calls.uploads == [result]
        assert [c[0] for c in engine_calls.calls] == ["wavelet"] and engine_calls.calls[0][3] is p.init_image_bytes_md[1]
        assert np.array_equal(np.asarray(pp.image), cr.wavelet_int(np.asarray(result), np.asarray(init)))
    finally:
        s.postprocess(p, None, True)
    assert not hasattr(p, "init_image_bytes_md") and p.init_images[0].size == (128, 96)
