"""The img2img upscale on the engine (mdtile_resample_* / mdtile.resize_u8 / tile_utils.utils.upscale_init_image), the checks that need no GPU:
the C ABI carries the entry points, the tap tables the library computes on the host equal the numpy restatement (tests/resample_ref.py)
exactly, the restatement equals Pillow bit for bit, the binding refuses CPU tensors, and upscale_init_image follows the host's
Upscaler.upscale step by step -- with mdtile.resize_u8 replaced by the restatement, so that the routing is checked without a GPU."""
import copy
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT
from hostsim import stub_host as sh
import resample_ref as rr

SYMBOLS = ["mdtile_resample_ksize", "mdtile_resample_table", "mdtile_resample_u8_ws_size", "mdtile_resample_u8"]


def test_header_declares_and_library_exports_the_entry_points(built_lib):
    src = open(os.path.join(ROOT, "include", "mdtile.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], capture_output=True, text=True).stdout
    public = [l.split()[-1] for l in out.splitlines() if " T " in l]
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, src), f"include/mdtile.h does not declare {s}"
        assert s in public, f"libmdtile.so does not export {s}"
        assert s in built_lib.exported_symbols()
    assert re.search(r"#define\s+MDTILE_RESAMPLE_NEAREST\s+0\b", src) and re.search(r"#define\s+MDTILE_RESAMPLE_LANCZOS\s+1\b", src)
    assert (built_lib.RESAMPLE_NEAREST, built_lib.RESAMPLE_LANCZOS) == (rr.NEAREST, rr.LANCZOS) == (0, 1)


# every (in, out) one axis of the case list sees, and the two flagship axes
AXES = sorted({(s[i], d[i]) for s, d in rr.PAIRS + rr.NEAREST_ONLY for i in (0, 1)}) + [(2048, 8192), (16384, 8192)]


@pytest.mark.parametrize("filt", [rr.LANCZOS, rr.NEAREST], ids=["lanczos", "nearest"])
def test_tables_equal_the_restatement(built_lib, filt):
    L = built_lib.lib()
    for n_in, n_out in AXES:
        want_c, want_b = rr.tables(n_in, n_out, filt)
        assert L.mdtile_resample_ksize(n_in, n_out, filt) == rr.ksize(n_in, n_out, filt) == want_c.shape[1], (n_in, n_out)
        coef, bounds = built_lib.resample_tables(n_in, n_out, filt)
        assert coef.dtype == np.int32 and bounds.dtype == np.int32
        assert coef.shape == want_c.shape and bounds.shape == (n_out, 2)
        assert np.array_equal(bounds, want_b), (n_in, n_out)
        assert np.array_equal(coef, want_c), (n_in, n_out)           # the zero padding past n included
        assert built_lib.resample_tables(n_in, n_out, filt)[0] is coef   # kept per (in, out, filter)
    # the tables are written in full: a poisoned buffer comes back with zeros past the taps
    n_in, n_out = 8, 64
    k = L.mdtile_resample_ksize(n_in, n_out, filt)
    coef = np.full((n_out, k), 0x55555555, np.int32)
    bounds = np.full((n_out, 2), 0x55555555, np.int32)
    assert L.mdtile_resample_table(n_in, n_out, filt, coef.ctypes.data, bounds.ctypes.data) == built_lib.OK
    assert np.array_equal(coef, rr.tables(n_in, n_out, filt)[0]) and np.array_equal(bounds, rr.tables(n_in, n_out, filt)[1])


def test_table_properties():
    """What the kernels lean on: windows inside the axis, moving right with the output index, taps summing to about 2^22."""
    for n_in, n_out in AXES[:-2]:
        for filt in (rr.LANCZOS, rr.NEAREST):
            coef, b = rr.tables(n_in, n_out, filt)
            assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= coef.shape[1]).all()
            assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()
            assert np.abs(coef.astype(np.int64).sum(axis=1) - (1 << 22)).max() <= coef.shape[1]
            assert np.abs(coef.astype(np.int64)).sum(axis=1).max() * 255 + (1 << 21) < 2 ** 31      # the int32 sum cannot overflow


def test_bad_arguments(built_lib):
    L = built_lib.lib()
    assert L.mdtile_resample_ksize(0, 8, 1) == 0 and L.mdtile_resample_ksize(8, 0, 1) == 0 and L.mdtile_resample_ksize(8, 8, 2) == 0
    assert L.mdtile_resample_ksize(8, -1, 0) == 0 and L.mdtile_resample_ksize(2 ** 31 - 1, 1, 1) == 0
    buf = np.zeros(64, np.int32)
    assert L.mdtile_resample_table(8, 8, 7, buf.ctypes.data, buf.ctypes.data) == built_lib.E_ARG and b"filter" in L.mdtile_last_error()
    assert L.mdtile_resample_table(0, 8, 1, buf.ctypes.data, buf.ctypes.data) == built_lib.E_ARG and b"sizes" in L.mdtile_last_error()
    assert L.mdtile_resample_table(8, 8, 1, None, buf.ctypes.data) == built_lib.E_ARG
    with pytest.raises(built_lib.MdtileError):
        built_lib.resample_tables(8, 0, built_lib.RESAMPLE_LANCZOS)
    assert L.mdtile_resample_u8_ws_size(2048, 2048, 3, 8192, 8192) == 2048 * 8192 * 3
    assert L.mdtile_resample_u8_ws_size(16, 16, 2, 32, 32) == 0 and L.mdtile_resample_u8_ws_size(0, 16, 3, 32, 32) == 0
    assert L.mdtile_resample_u8_ws_size(32768, 32768, 3, 8, 8) == 0 and L.mdtile_resample_u8_ws_size(8, 8, 1, 65536, 32768) == 0   # 2^31 and more
    # refused before anything touches the device: the pointers are never read
    one = 4096

    def call(H, W, C, oh, ow, cx, bx, kx, cy, by, ky, ws):
        rc = L.mdtile_resample_u8(one, H, W, C, one, oh, ow, cx, bx, kx, cy, by, ky, ws, None)
        return rc, L.mdtile_last_error().decode()

    rc, msg = call(16, 16, 2, 32, 32, one, one, 7, one, one, 7, one)
    assert rc == built_lib.E_ARG and "channels" in msg
    rc, msg = call(65536, 32768, 1, 8, 8, one, one, 7, one, one, 7, one)
    assert rc == built_lib.E_ARG and "2^31" in msg
    rc, msg = call(16, 16, 3, 32, 32, None, None, 0, one, one, 7, one)
    assert rc == built_lib.E_ARG and "outW == W" in msg
    rc, msg = call(16, 16, 3, 32, 32, one, one, 7, one, None, 7, one)
    assert rc == built_lib.E_ARG and "vertical" in msg
    rc, msg = call(16, 16, 3, 32, 32, one, one, 7, one, one, 7, None)
    assert rc == built_lib.E_ARG and "workspace" in msg


def test_cpu_tensors_are_refused(built_lib):
    with pytest.raises(built_lib.MdtileError, match="no CPU fallback"):
        built_lib.resize_u8(torch.zeros(16, 16, 3, dtype=torch.uint8), (32, 32), built_lib.RESAMPLE_LANCZOS)
    with pytest.raises(built_lib.MdtileError, match="no CPU fallback"):
        built_lib.resize_u8(torch.zeros(16, 16, dtype=torch.uint8), (8, 8), built_lib.RESAMPLE_NEAREST)


@pytest.mark.parametrize("case", rr.cases(), ids=rr.case_id)
def test_restatement_is_pillows(case):
    Image = pytest.importorskip("PIL.Image")
    src, dst, filt, rgb = case
    img = rr.make_image(src, rgb)
    how = Image.Resampling.LANCZOS if filt == rr.LANCZOS else Image.Resampling.NEAREST
    want = np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), how))
    got = rr.expected(*case)
    assert got.shape == want.shape and int((got != want).sum()) == 0
    if filt == rr.LANCZOS and rr.hard_edged(src) and dst[0] >= src[0] and dst[1] >= src[1] and dst != src:
        # the clamp at work: a hard 0 / 255 image overshoots under Lanczos, and those sums are cut to the byte range
        assert ((want == 0) | (want == 255)).any()


# ---- routing: upscale_init_image against a copy of the host's Upscaler.upscale -----------------------------------------------------------
def _lanczos():
    from PIL import Image
    return Image.Resampling.LANCZOS


class _HostUpscaler:
    """modules/upscaler.py of the host: Upscaler.upscale, which scripts/tilediffusion.py called until now."""
    scale = 1

    def __init__(self):
        self.rounds = 0

    def upscale(self, img, scale, selected_model=None):
        self.scale = scale
        dest_w = int((img.width * scale) // 8 * 8)
        dest_h = int((img.height * scale) // 8 * 8)
        for _ in range(3):
            if img.width >= dest_w and img.height >= dest_h:
                break
            shape = (img.width, img.height)
            img = self.do_upscale(img, selected_model)
            if shape == (img.width, img.height):
                break
        if img.width != dest_w or img.height != dest_h:
            img = img.resize((int(dest_w), int(dest_h)), resample=_lanczos())
        return img


class UpscalerLanczos(_HostUpscaler):
    def do_upscale(self, img, selected_model=None):
        self.rounds += 1
        return img.resize((int(img.width * self.scale), int(img.height * self.scale)), resample=_lanczos())


class UpscalerNearest(_HostUpscaler):
    def do_upscale(self, img, selected_model=None):
        from PIL import Image
        self.rounds += 1
        return img.resize((int(img.width * self.scale), int(img.height * self.scale)), resample=Image.Resampling.NEAREST)


class UpscalerModel(_HostUpscaler):
    """A model-like upscaler: always x4, whatever scale is asked for."""
    def do_upscale(self, img, selected_model=None):
        from PIL import Image
        self.rounds += 1
        return img.resize((img.width * 4, img.height * 4), resample=Image.Resampling.BICUBIC)


def _upscaler(kind):
    cls = {"Lanczos": UpscalerLanczos, "Nearest": UpscalerNearest, "Model": UpscalerModel}[kind]
    return SimpleNamespace(name=kind if kind != "Model" else "R-ESRGAN 4x+", scaler=cls(), data_path="weights.pth")


@pytest.fixture
def engine_calls(plugin, monkeypatch):
    """mdtile.resize_u8 replaced by the numpy restatement (on CPU tensors); the list collects (in size, out size, filter) of every call."""
    calls = []

    def fake(t, size, filt):
        assert t.dtype == torch.uint8
        calls.append(((int(t.shape[0]), int(t.shape[1])), (int(size[0]), int(size[1])), int(filt)))
        return torch.from_numpy(rr.resize(t.cpu().numpy(), int(size[0]), int(size[1]), int(filt)))
    monkeypatch.setattr(plugin.engine, "resize_u8", fake)
    assert plugin.utils.mdtile is plugin.engine
    return calls


def _photo(w, h, mode="RGB"):
    from PIL import Image
    rng = np.random.default_rng(w + 3 * h)
    if mode == "L":
        return Image.fromarray(rng.integers(0, 256, size=(h, w)).astype(np.uint8))
    img = Image.fromarray(rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8))
    return img if mode == "RGB" else img.convert(mode)


@pytest.mark.parametrize("scale", [2, 2.5, 1.05])
@pytest.mark.parametrize("size", [(256, 384), (1023, 517)], ids=["256x384", "1023x517"])
@pytest.mark.parametrize("kind", ["Lanczos", "Nearest", "Model"])
def test_upscale_init_image_is_the_hosts_upscale(plugin, engine_calls, kind, size, scale):
    pytest.importorskip("PIL")
    image = _photo(*size)
    ref_up = _upscaler(kind)
    want = ref_up.scaler.upscale(image, scale, ref_up.data_path)
    up = _upscaler(kind)
    got, kept = plugin.utils.upscale_init_image(image, up, scale)
    assert got.mode == want.mode and got.size == want.size
    assert got.size == (int(size[0] * scale // 8 * 8), int(size[1] * scale // 8 * 8))
    assert np.array_equal(np.asarray(got), np.asarray(want))
    assert up.scaler.scale == scale
    fit = [c for c in engine_calls if c[1] == (want.height, want.width) and c[2] == rr.LANCZOS][-1:]
    if kind == "Model":
        # the model's rounds are the host's do_upscale; the engine runs the final fit alone
        assert up.scaler.rounds == ref_up.scaler.rounds >= 1
        assert engine_calls == fit and len(fit) == (0 if (size[0] * 4, size[1] * 4) == want.size else 1)
    else:
        assert up.scaler.rounds == 0                                   # no Pillow resize on the host
        filt = rr.LANCZOS if kind == "Lanczos" else rr.NEAREST
        rounds = engine_calls[:ref_up.scaler.rounds]
        assert len(rounds) == ref_up.scaler.rounds and all(c[2] == filt for c in rounds)
        assert rounds[0][0] == (size[1], size[0]) and rounds[0][1] == (int(size[1] * scale), int(size[0] * scale))
        rest = engine_calls[ref_up.scaler.rounds:]
        assert rest == ([] if rounds[-1][1] == (want.height, want.width) else fit) and len(rest) <= 1
    if engine_calls:
        assert kept is not None and tuple(kept.shape) == (want.height, want.width, 3)
        assert np.array_equal(kept.cpu().numpy(), np.asarray(want))    # the bytes handed on to the renoise mask are the image's
    else:
        assert kept is None


def test_1023_times_2_is_two_resamples(plugin, engine_calls):
    """1023 x 2 = 2046 -> 2040: the round and the fit both run, as they do on the host."""
    pytest.importorskip("PIL")
    plugin.utils.upscale_init_image(_photo(1023, 64), _upscaler("Lanczos"), 2)
    assert engine_calls == [((64, 1023), (128, 2046), rr.LANCZOS), ((128, 2046), (128, 2040), rr.LANCZOS)]


def test_grey_images_go_through_the_engine(plugin, engine_calls):
    pytest.importorskip("PIL")
    image = _photo(100, 60, "L")
    got, kept = plugin.utils.upscale_init_image(image, _upscaler("Lanczos"), 2)
    want = _upscaler("Lanczos").scaler.upscale(image, 2)
    assert got.mode == "L" and np.array_equal(np.asarray(got), np.asarray(want)) and kept.dim() == 2 and len(engine_calls) == 1


def test_other_modes_and_foreign_upscalers_take_the_host_call(plugin, engine_calls):
    pytest.importorskip("PIL")
    image = _photo(64, 48, "RGBA")
    up = _upscaler("Lanczos")
    got, kept = plugin.utils.upscale_init_image(image, up, 2)
    assert kept is None and engine_calls == [] and up.scaler.rounds == 1 and got.mode == "RGBA" and got.size == (128, 96)
    assert np.array_equal(np.asarray(got), np.asarray(_upscaler("Lanczos").scaler.upscale(image, 2)))
    # an upscaler object that only has upscale(): called as before
    seen = []
    blob = SimpleNamespace(name="Lanczos", data_path=None, scaler=SimpleNamespace(upscale=lambda img, s, path: seen.append((s, path)) or img))
    got, kept = plugin.utils.upscale_init_image(_photo(64, 48), blob, 2)
    assert kept is None and seen == [(2, None)] and engine_calls == []
    # the name alone does not make a built-in upscaler: another class listed as "Lanczos" keeps its own rounds
    other = SimpleNamespace(name="Lanczos", data_path=None, scaler=UpscalerModel())
    got, kept = plugin.utils.upscale_init_image(_photo(64, 48), other, 2)
    assert other.scaler.rounds == 1 and got.size == (128, 96) and [c[1] for c in engine_calls] == [(96, 128)]


def _process(plugin, p, upscaler_name, scale, keep_input_size, noise_inverse=False):
    s = plugin.tilediffusion.Script()
    defaults = list(plugin.utils.DEFAULT_BBOX_SETTINGS) * 8
    s.process(p, True, "MultiDiffusion", False, keep_input_size, 1024, 1024, 96, 96, 48, 4, upscaler_name, scale, noise_inverse, 10, 1, 1, 64, False,
              False, False, False, *defaults)
    return s


@pytest.mark.parametrize("keep_input_size", [True, False])
@pytest.mark.parametrize("kind,scale", [("Lanczos", 2), ("Lanczos", 2.5), ("Nearest", 2), ("Model", 2)])
def test_process_leaves_p_as_the_host_call_does(plugin, engine_calls, monkeypatch, kind, scale, keep_input_size):
    """Script.process with upscale_init_image against the same process with the one line it replaces
    (image = upscaler.scaler.upscale(image, scale_factor, upscaler.data_path)) put back."""
    pytest.importorskip("PIL")
    _, shared = sh.host()
    td = plugin.tilediffusion
    results = []
    for parent in (False, True):
        up = _upscaler(kind)
        monkeypatch.setattr(shared, "sd_upscalers", [SimpleNamespace(name="None", scaler=None, data_path=None), up])
        if parent:
            monkeypatch.setattr(td, "upscale_init_image", lambda image, upscaler, s: (upscaler.scaler.upscale(image, s, upscaler.data_path), None))
        first = _photo(520, 328)
        p = sh.make_processing(512, 320, init_images=[first, _photo(520, 328)], extra_generation_params={"Seed": 1})
        s = _process(plugin, p, up.name, scale, keep_input_size)
        try:
            assert p.init_images[0] is p.init_images[1] and p.init_images[0] is not first
            assert hasattr(p, "init_image_bytes_md") == (not parent)
            if not parent:
                assert p.init_image_bytes_md[0] is p.init_images[0]
            results.append((p.width, p.height, copy.deepcopy(p.extra_generation_params), p.init_images[0].mode, p.init_images[0].size,
                            np.asarray(p.init_images[0]).copy(), [im.size for im in p.init_images_original_md]))
        finally:
            s.postprocess(p, None, True)
        assert not hasattr(p, "init_image_bytes_md") and p.init_images[0] is not None and p.init_images[0].size == (520, 328)
        assert (p.width, p.height) == (512, 320)
    new, old = results
    assert new[:5] == old[:5] and np.array_equal(new[5], old[5]) and new[6] == old[6]
    assert new[2]["Tiled Diffusion upscaler"] == up.name and new[2]["Tiled Diffusion scale factor"] == scale
    assert new[2]["Tiled Diffusion"]["Upscaler"] == up.name and new[2]["Tiled Diffusion"]["Upscale factor"] == scale
    assert (new[0], new[1]) == (new[4] if keep_input_size else (int(scale * 512), int(scale * 320)))


def test_renoise_mask_takes_the_kept_bytes_only_for_their_image(plugin, monkeypatch):
    """AbstractDiffusion.renoise_mask hands get_retouch_mask the device tensor when p.init_images[0] IS the image it belongs to, and the
    host pixels otherwise (another extension may have replaced the init image after the upscale)."""
    pytest.importorskip("PIL")
    absd = plugin.abstractdiffusion
    seen = []
    monkeypatch.setattr(absd, "get_retouch_mask", lambda pixels, k: seen.append(pixels) or torch.zeros(48, 64))
    monkeypatch.setattr(absd.mdtile, "renoise_resize", lambda m, size, strength: m)
    me = SimpleNamespace(noise_inverse_renoise_strength=1.0, noise_inverse_renoise_kernel=3)
    image, other = _photo(64, 48), _photo(64, 48)
    kept = torch.zeros(48, 64, 3, dtype=torch.uint8)
    p = SimpleNamespace(init_images=[image], init_image_bytes_md=(image, kept))
    absd.AbstractDiffusion.renoise_mask(me, p, (6, 8))
    p.init_images[0] = other
    absd.AbstractDiffusion.renoise_mask(me, p, (6, 8))
    del p.init_image_bytes_md
    absd.AbstractDiffusion.renoise_mask(me, p, (6, 8))
    assert seen[0] is kept and isinstance(seen[1], np.ndarray) and isinstance(seen[2], np.ndarray)
    assert np.array_equal(seen[1], np.asarray(other))
