"""What tests/test_colorfix_host.py and tests/test_gpu_colorfix.py share besides the restatements of tests/colorfix_ref.py: images, the option,
a call of Script.process with the UI's argument order, and a stand-in for the host's built-in Lanczos upscaler."""
from types import SimpleNamespace

import numpy as np

from hostsim import stub_host as sh
import colorfix_ref as cr


def apply_lut(lut, img):
    """lut[c] applied to channel c of img, on the host."""
    a = cr._hwc(img)
    return np.stack([lut[ch][a[:, :, ch]] for ch in range(a.shape[2])], axis=2).reshape(img.shape)


def photo(w, h, mode="RGB", seed=0):
    from PIL import Image
    rng = np.random.default_rng(w + 3 * h + seed)
    if mode == "L":
        return Image.fromarray(rng.integers(0, 256, size=(h, w)).astype(np.uint8))
    img = Image.fromarray(rng.integers(0, 256, size=(h, w, 3)).astype(np.uint8))
    return img if mode == "RGB" else img.convert(mode)


def set_option(monkeypatch, value):
    _, shared = sh.host()
    monkeypatch.setattr(shared.cmd_opts, "mdtile_color_fix", value, raising=False)


def process(plugin, p, upscaler_name="None", scale=2, enabled=True):
    s = plugin.tilediffusion.Script()
    defaults = list(plugin.utils.DEFAULT_BBOX_SETTINGS) * 8
    s.process(p, enabled, "MultiDiffusion", False, True, 1024, 1024, 96, 96, 48, 4, upscaler_name, scale, False, 10, 1, 1, 64, False,
              False, False, False, *defaults)
    return s


class UpscalerLanczos:
    """The host's built-in Lanczos upscaler as far as these tests need it (the plugin knows it by this class name and the name it is listed
    under): one Pillow Lanczos round per do_upscale, and upscale to the scaled size cut to multiples of 8."""
    scale = 1

    def do_upscale(self, img, selected_model=None):
        from PIL import Image
        return img.resize((int(img.width * self.scale), int(img.height * self.scale)), resample=Image.Resampling.LANCZOS)

    def upscale(self, img, scale, selected_model=None):
        from PIL import Image
        self.scale = scale
        dest = (int(img.width * scale // 8 * 8), int(img.height * scale // 8 * 8))
        img = self.do_upscale(img, selected_model)
        return img if img.size == dest else img.resize(dest, resample=Image.Resampling.LANCZOS)


def lanczos_upscalers():
    """A host's upscaler list: "None" and the built-in Lanczos."""
    return [SimpleNamespace(name="None", scaler=None, data_path=None), SimpleNamespace(name="Lanczos", scaler=UpscalerLanczos(), data_path=None)]
