"""Renoise mask of Noise Inversion (mdtile_retouch_mask / mdtile_renoise_resize), the checks that need no GPU: the C ABI carries the
entry points, the plugin no longer names OpenCV, the binding refuses CPU tensors, and the numpy restatement the GPU tests compare
against (tests/retouch_ref.py) is itself sane."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
import retouch_ref as rr

SYMBOLS = ["mdtile_retouch_mask_ws_size", "mdtile_retouch_mask", "mdtile_renoise_resize"]
PLUGIN_DIR = os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd")


def test_header_declares_and_library_exports_the_entry_points(built_lib):
    src = open(os.path.join(ROOT, "include", "mdtile.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", built_lib.LIB_PATH], capture_output=True, text=True).stdout
    public = [l.split()[-1] for l in out.splitlines() if " T " in l]
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, src), f"include/mdtile.h does not declare {s}"
        assert s in public, f"libmdtile.so does not export {s}"
        assert s in built_lib.exported_symbols()


def test_workspace_size_is_eight_bytes_per_pixel(built_lib):
    L = built_lib.lib()
    assert L.mdtile_retouch_mask_ws_size(224, 320, 64) == 8 * 224 * 320
    assert L.mdtile_retouch_mask_ws_size(8192, 8192, 512) == 8 * 8192 * 8192
    assert L.mdtile_retouch_mask_ws_size(224, 320, 0) == 0 and L.mdtile_retouch_mask_ws_size(224, 320, 513) == 0
    assert L.mdtile_retouch_mask_ws_size(65536, 32768, 3) == 0      # H * W = 2^31


def test_plugin_does_not_name_opencv():
    hits = []
    for d, _, files in os.walk(PLUGIN_DIR):
        for f in files:
            if f.endswith(".py") and "cv2" in open(os.path.join(d, f), errors="replace").read():
                hits.append(os.path.relpath(os.path.join(d, f), ROOT))
    assert hits == []


def test_cpu_tensors_are_refused(built_lib):
    with pytest.raises(built_lib.MdtileError, match="no CPU fallback"):
        built_lib.retouch_mask(torch.zeros(16, 16, dtype=torch.uint8), 3)
    with pytest.raises(built_lib.MdtileError, match="no CPU fallback"):
        built_lib.renoise_resize(torch.zeros(16, 16), (2, 2), 1.0)


def test_reference_flat_image_gives_zero():
    for k in (1, 2, 3, 64, 512):
        assert not rr.retouch_mask(np.full((20, 30), 77, np.uint8), k).any()
        assert not rr.retouch_mask(np.full((20, 30, 3), 255, np.uint8), k).any()


def test_reference_grey_is_pils():
    from PIL import Image
    rgb = np.random.default_rng(5).integers(0, 256, size=(96, 128, 3)).astype(np.uint8)
    assert np.array_equal(rr.grey(rgb), np.asarray(Image.fromarray(rgb).convert("L")))


def test_reference_window_sums_against_the_plain_loop():
    """The reflected window, anchor k/2, written as loops over a tiny image -- also with windows many times the image."""
    L = np.random.default_rng(6).integers(0, 256, size=(5, 7)).astype(np.int64)

    def refl(i, n):
        if n == 1:
            return 0
        while i < 0 or i >= n:
            i = -i if i < 0 else 2 * (n - 1) - i
        return i

    for k in (1, 2, 3, 8, 33):
        s1, s2 = rr.window_sums(L, k)
        for y in range(5):
            for x in range(7):
                win = [L[refl(y - k // 2 + dy, 5), refl(x - k // 2 + dx, 7)] for dy in range(k) for dx in range(k)]
                assert s1[y, x] == sum(win) and s2[y, x] == sum(int(v) * int(v) for v in win), (k, y, x)


def test_reference_bilinear_is_torchs_on_exact_ratios():
    import torch.nn.functional as F
    m = np.random.default_rng(7).random((64, 96)).astype(np.float32)
    want = F.interpolate(torch.from_numpy(m)[None, None], size=(8, 12), mode="bilinear")[0, 0].numpy()
    assert np.abs(rr.bilinear(m, (8, 12)) - want).max() <= 2.0 ** -22
