"""A/B of the img2img init-image upscale: the host's Pillow route (Upscaler.upscale on one CPU thread) against tile_utils.utils.upscale_init_image
(mdtile_resample_u8) in ONE process, alternating, every timed region closed by a device synchronise.  Prints one JSON line.

    python probes/upscale_ab.py [--reps 5] [--cases lanczos_x4,fit_half,nearest_x4] [--mask]     (on the GPU box)
    rocprofv3 --kernel-trace --stats -d DIR -- python probes/upscale_ab.py --kernels              kernel time of the two passes next to
                                                                                                   mdtile_stream_copy of the same bytes

  lanczos_x4   built-in Lanczos upscaler, 2048^2 -> 8192^2 RGB
  fit_half     a x4 model upscaler asked for x2 on 4096^2: its 16384^2 output (made once, outside the timing) is fitted to 8192^2
  nearest_x4   built-in Nearest upscaler, 2048^2 -> 8192^2 RGB
  --mask       Noise Inversion's renoise mask at 8192^2 with and without the bytes the upscale leaves on the device
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from hostsim import stub_host as sh  # noqa: E402

sh.install("cuda:0")
sh.set_device("cuda:0")
pl = sh.load_plugin()
E, U = pl.engine, pl.utils
from PIL import Image  # noqa: E402

Image.MAX_IMAGE_PIXELS = None
DEV = torch.device("cuda:0")


class HostUpscaler:
    """Upscaler.upscale of the host (modules/upscaler.py)."""
    scale = 1

    def upscale(self, img, scale, selected_model=None):
        self.scale = scale
        dest_w, dest_h = int((img.width * scale) // 8 * 8), int((img.height * scale) // 8 * 8)
        for _ in range(3):
            if img.width >= dest_w and img.height >= dest_h:
                break
            shape = (img.width, img.height)
            img = self.do_upscale(img, selected_model)
            if shape == (img.width, img.height):
                break
        if img.width != dest_w or img.height != dest_h:
            img = img.resize((int(dest_w), int(dest_h)), resample=Image.Resampling.LANCZOS)
        return img


class UpscalerLanczos(HostUpscaler):
    def do_upscale(self, img, selected_model=None):
        return img.resize((int(img.width * self.scale), int(img.height * self.scale)), resample=Image.Resampling.LANCZOS)


class UpscalerNearest(HostUpscaler):
    def do_upscale(self, img, selected_model=None):
        return img.resize((int(img.width * self.scale), int(img.height * self.scale)), resample=Image.Resampling.NEAREST)


class UpscalerModel(HostUpscaler):
    """Stands in for a x4 model: hands out an image made beforehand, so that only the fit is timed."""
    def __init__(self, ready):
        self.ready = ready

    def do_upscale(self, img, selected_model=None):
        return self.ready


def photo(n, seed):
    return Image.fromarray(np.random.default_rng(seed).integers(0, 256, size=(n, n, 3), dtype=np.uint8))


def sync():
    torch.cuda.synchronize()


def timed(fn):
    sync()
    t = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t) * 1e3, out


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3)}


def make_case(name):
    if name == "lanczos_x4":
        return photo(2048, 1), SimpleNamespace(name="Lanczos", scaler=UpscalerLanczos(), data_path=None), 4, E.RESAMPLE_LANCZOS
    if name == "nearest_x4":
        return photo(2048, 2), SimpleNamespace(name="Nearest", scaler=UpscalerNearest(), data_path=None), 4, E.RESAMPLE_NEAREST
    if name == "fit_half":
        return photo(4096, 3), SimpleNamespace(name="R-ESRGAN 4x+", scaler=UpscalerModel(photo(16384, 4)), data_path=None), 2, E.RESAMPLE_LANCZOS
    raise SystemExit(f"unknown case {name}")


def run_case(name, reps):
    image, up, scale, filt = make_case(name)
    host = lambda: up.scaler.upscale(image, scale, up.data_path)              # noqa: E731
    engine = lambda: U.upscale_init_image(image, up, scale)                   # noqa: E731
    want = host()
    got, kept = engine()                                                      # warm-up of both routes (tables, pinned buffer, kernels)
    res = {"out": list(want.size), "bytes_differ": int((np.asarray(got) != np.asarray(want)).sum())}
    del got, kept
    t_host, t_eng = [], []
    for _ in range(reps):
        t_host.append(timed(host)[0])
        t_eng.append(timed(engine)[0])
    res["pillow"], res["engine"] = summary(t_host), summary(t_eng)
    res["speedup_median"] = round(res["pillow"]["median_ms"] / res["engine"]["median_ms"], 2)
    res["faster_beyond_spread"] = bool(max(t_eng) < min(t_host))
    # the engine route in its parts: what goes up is the image the resize reads (the model's output for fit_half)
    src = up.scaler.ready if name == "fit_half" else image
    size = (want.height, want.width)
    parts = {"upload": [], "kernels": [], "download": [], "fromarray": []}
    for _ in range(reps):
        ms, t = timed(lambda: U.image_to_device(src))
        parts["upload"].append(ms)
        ms, out = timed(lambda: E.resize_u8(t, size, filt))
        parts["kernels"].append(ms)
        host_buf = torch.empty(out.shape, dtype=torch.uint8, pin_memory=True)
        ms, _ = timed(lambda: host_buf.copy_(out, non_blocking=True))
        parts["download"].append(ms)
        ms, _ = timed(lambda: Image.fromarray(host_buf.numpy()))
        parts["fromarray"].append(ms)
        del t, out, host_buf
    res["engine_parts_median_ms"] = {k: round(statistics.median(v), 3) for k, v in parts.items()}
    print(f"[upscale_ab] {name}: {res}", file=sys.stderr, flush=True)
    return res


def run_mask(reps):
    """AbstractDiffusion.renoise_mask (kernel 64, strength 1) on an 8192^2 RGB init image: from the bytes kept on the device / from the host image."""
    absd = pl.abstractdiffusion
    image = photo(8192, 5)
    kept = U.image_to_device(image)
    me = SimpleNamespace(noise_inverse_renoise_strength=1.0, noise_inverse_renoise_kernel=64)
    with_kept = SimpleNamespace(init_images=[image], init_image_bytes_md=(image, kept))
    without = SimpleNamespace(init_images=[image])
    a = absd.AbstractDiffusion.renoise_mask(me, with_kept, (1024, 1024))
    b = absd.AbstractDiffusion.renoise_mask(me, without, (1024, 1024))
    same = bool(torch.equal(a, b))
    t_kept, t_host = [], []
    for _ in range(reps):
        t_kept.append(timed(lambda: absd.AbstractDiffusion.renoise_mask(me, with_kept, (1024, 1024)))[0])
        t_host.append(timed(lambda: absd.AbstractDiffusion.renoise_mask(me, without, (1024, 1024)))[0])
    return {"identical": same, "kept_device_bytes": summary(t_kept), "host_image": summary(t_host)}


def run_kernels():
    """For a kernel trace: each case's resize three times, then mdtile_stream_copy moving as many bytes as the two passes read + write."""
    out = {}
    for name, (h, oh, filt) in {"lanczos_x4": (2048, 8192, E.RESAMPLE_LANCZOS), "fit_half": (16384, 8192, E.RESAMPLE_LANCZOS),
                                "nearest_x4": (2048, 8192, E.RESAMPLE_NEAREST)}.items():
        src = torch.randint(0, 256, (h, h, 3), dtype=torch.uint8, device=DEV)
        for _ in range(3):
            E.resize_u8(src, (oh, oh), filt)
        moved = h * h * 3 + 2 * h * oh * 3 + oh * oh * 3           # in + intermediate written and read + out
        a = torch.empty(moved // 2, dtype=torch.uint8, device=DEV)
        b = torch.empty_like(a)
        for _ in range(3):
            E.stream_copy(a, b)
        sync()
        out[name] = {"bytes_read_plus_written": moved, "stream_copy_bytes": int(a.numel())}
        del src, a, b
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="lanczos_x4,fit_half,nearest_x4")
    ap.add_argument("--mask", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    a = ap.parse_args()
    result = {"probe": "upscale_ab", "pillow": Image.__version__, "reps": a.reps}
    if a.kernels:
        result["kernels"] = run_kernels()
    else:
        result["cases"] = {c: run_case(c, a.reps) for c in a.cases.split(",") if c}
        if a.mask:
            result["renoise_mask_8192"] = run_mask(a.reps)
    print(json.dumps(result))
