"""Noise Inversion's renoise mask on the GPU (csrc/retouch.hip; upstream tile_utils/utils.py:216-247 + abstractdiffusion.py:607-621, where it
is OpenCV on the CPU).  mdtile_retouch_mask is DEFINED exactly (include/mdtile.h), so the mask is compared bit for bit with the numpy
restatement tests/retouch_ref.py -- on images where 0.2 - 1 % of the pixels sit within 1e-3 of a quantisation threshold, a tolerance would
hide any last-bit error by letting whole levels through.  mdtile_renoise_resize is compared with torch's own CPU bilinear resize where the
source coordinates carry no rounding, and with the op-by-op restatement elsewhere.  Last: the default Noise Inversion job through the
delegate with nothing stubbed."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from hostsim import stub_host as sh
from oracle import blend_oracle as bo
import retouch_ref as rr

pytestmark = pytest.mark.gpu

# (H, W, k).  Kernel geometry (csrc/retouch.hip): a block scans one row segment of <= 1536 px (+ k - 1 halo), a thread walks one column of
# a chunk of clamp(k, 32, 256) rows, 256 columns per block.
MASK_CASES = [
    (8, 8, 2),
    (8, 8, 512),            # many reflections on both axes
    (224, 320, 3),
    (224, 320, 64),
    (136, 200, 512),
    (67, 131, 5),           # odd sizes
    (520, 1032, 64),        # 9 row chunks, 5 column blocks
    (1024, 1536, 63),       # odd window, a full segment
    (67, 131, 1),           # k = 1: the window is the pixel
    (5, 3100, 9),           # three row segments
    (3, 1537, 512),         # two segments, window wider than a segment's share and 170 x the height
    (1, 40, 7),
    (40, 1, 7),             # n == 1 -> index 0
    (300, 70, 257),         # chunk size capped at 256 rows
]


@functools.lru_cache(maxsize=None)
def _case(H, W, k, rgb):
    img = rr.make_image(H, W, seed=H * 7 + W + k, rgb=rgb)
    return img, rr.retouch_mask(img, k)


# RGB and grey input for every case but the largest, whose grey twin would add a second of reference time and no new path
MASK_PARAMS = [(H, W, k, rgb) for (H, W, k) in MASK_CASES for rgb in (True, False) if rgb or H * W < 600000]


@pytest.mark.parametrize("H,W,k,rgb", MASK_PARAMS, ids=[f"{H}x{W}-k{k}-{'rgb' if rgb else 'grey'}" for (H, W, k, rgb) in MASK_PARAMS])
def test_mask_is_bitwise_the_definition(plugin, cuda, H, W, k, rgb):
    E = plugin.engine
    img, want = _case(H, W, k, rgb)
    got = E.retouch_mask(torch.from_numpy(img).to(cuda), k).cpu()
    diff = int((got != torch.from_numpy(want)).sum())
    print(f"retouch_mask {H}x{W} k={k} {'rgb' if rgb else 'grey'}: {len(np.unique(want))} levels, {diff} of {H * W} pixels differ")
    assert got.dtype == torch.float32 and tuple(got.shape) == (H, W)
    assert torch.equal(got, torch.from_numpy(want))


@pytest.mark.parametrize("value,k", [(93, 64), (0, 3), (255, 5), (255, 512)])
def test_flat_images_give_exactly_zero(plugin, cuda, value, k):
    E = plugin.engine
    for shape in ((64, 96), (64, 96, 3)):
        img = np.full(shape, value, np.uint8)
        got = E.retouch_mask(torch.from_numpy(img).to(cuda), k).cpu()
        assert torch.equal(got, torch.from_numpy(rr.retouch_mask(img, k)))
        assert not got.any()


def _coef(B, C, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.rand(B, 1, C, generator=g) * 1.5 + 0.25, torch.randn(B, 1, C, generator=g) * 0.5], dim=1).contiguous().to(dev)


def test_mask_is_deterministic_alone_and_next_to_an_mfma_kernel(plugin, cuda):
    """Integer sums and a fixed fp32 sequence: the same bits on every call, also with the CUs shared with a split-bf16 MFMA conv that another
    stream launched (one run, as tests/test_gpu_coresidency.py does it)."""
    E, dev = plugin.engine, cuda
    img, want = _case(1024, 1536, 63, True)
    d_img = torch.from_numpy(img).to(dev)
    alone = E.retouch_mask(d_img, 63)
    again = E.retouch_mask(d_img, 63)
    torch.cuda.synchronize()
    assert torch.equal(alone, again)
    torch.manual_seed(3)
    c = torch.nn.Conv2d(256, 256, 3, padding=1).to(dev)
    pc = E.PackedConv(c.weight.detach(), c.bias.detach())
    x, coef = torch.randn(1, 256, 556, 556, device=dev), _coef(1, 256, 2, dev)
    pc(x, pre_gn=coef)                                   # packed and warmed up before the overlap
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(3):
            pc(x, pre_gn=coef)
    beside = E.retouch_mask(d_img, 63)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(beside, alone)
    assert torch.equal(alone.cpu(), torch.from_numpy(want))


def test_argument_errors(plugin, cuda):
    E = plugin.engine
    L = E.lib()
    img = torch.zeros(16, 16, 3, dtype=torch.uint8, device=cuda)
    out = torch.empty(16, 16, device=cuda)
    ws = torch.empty(8 * 16 * 16, dtype=torch.uint8, device=cuda)

    def call(H, W, ch, k):
        rc = L.mdtile_retouch_mask(img.data_ptr(), H, W, ch, k, out.data_ptr(), ws.data_ptr(), None)
        return rc, L.mdtile_last_error().decode()

    for k in (0, 513, -3):
        rc, msg = call(16, 16, 3, k)
        assert rc == E.E_ARG and "kernel_size" in msg, (k, rc, msg)
        with pytest.raises(E.MdtileError, match="kernel_size"):
            E.retouch_mask(img, k)
    rc, msg = call(16, 16, 2, 3)
    assert rc == E.E_ARG and "channels" in msg, (rc, msg)
    rc, msg = call(65536, 32768, 1, 3)                      # H * W = 2^31: refused before anything is launched
    assert rc == E.E_ARG and "2^31" in msg, (rc, msg)
    rc, msg = call(0, 16, 1, 3)
    assert rc == E.E_ARG
    with pytest.raises(E.MdtileError, match="shape"):
        E.retouch_mask(torch.zeros(16, 16, 2, dtype=torch.uint8, device=cuda), 3)
    with pytest.raises(E.MdtileError, match="dtype"):
        E.retouch_mask(torch.zeros(16, 16, device=cuda), 3)
    assert call(16, 16, 3, 3)[0] == E.OK                    # and the same buffers are fine for a legal call
    torch.cuda.synchronize()


# max |delta| <= 3e-6: every operand lies in [0, 1]; each side rounds at most 9 times (2 weights per axis, 6 for the interpolation, the
# subtraction from 1) by at most 2^-24 = 6e-8 each, and the scaling by strength <= 2 doubles that: ~1.2e-6 per side.
RESIZE_TOL = 3e-6
STRENGTHS = [0.7, 1.0, 2.0]


def _levels(H, W, seed):
    """A mask as mdtile_retouch_mask leaves it: multiples of 1 / 255, many of them 0."""
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, size=(H, W)) * (rng.random((H, W)) < 0.7)
    return (q.astype(np.float32) / np.float32(255.0))


@pytest.mark.parametrize("src,dst", [((224, 320), (28, 40)), ((64, 64), (16, 16)), ((32, 48), (32, 48)), ((16, 24), (32, 48))])
def test_resize_against_torch(plugin, cuda, src, dst):
    E = plugin.engine
    m = _levels(*src, seed=src[0] + dst[0])
    base = F.interpolate(torch.from_numpy(m)[None, None], size=dst, mode="bilinear")[0, 0]
    d_m = torch.from_numpy(m).to(cuda)
    for s in STRENGTHS:
        want = torch.clamp((1 - base) * s, 0, 1)
        got = E.renoise_resize(d_m, dst, s).cpu()
        err = (got - want).abs().max().item()
        print(f"renoise_resize {src} -> {dst} strength {s}: max |delta| vs torch {err:.3g}")
        assert tuple(got.shape) == dst and err <= RESIZE_TOL
        assert got.min().item() >= 0.0 and got.max().item() <= 1.0


@pytest.mark.parametrize("src,dst", [((100, 75), (13, 9)), ((250, 333), (31, 41)), ((224, 320), (28, 40))])
def test_resize_against_the_restatement(plugin, cuda, src, dst):
    E = plugin.engine
    m = _levels(*src, seed=src[1] + dst[1])
    d_m = torch.from_numpy(m).to(cuda)
    for s in STRENGTHS:
        want = rr.renoise_resize(m, dst, s)
        got = E.renoise_resize(d_m, dst, s).cpu().numpy()
        err = float(np.abs(got - want).max())
        print(f"renoise_resize {src} -> {dst} strength {s}: max |delta| vs the fp32 restatement {err:.3g}")
        assert err <= RESIZE_TOL


# ---- through the delegate, nothing stubbed -------------------------------------------------------------------------------------
NI_REGIONS = [(3, 2, 20, 12, "Background", 0.2), (10, 6, 18, 14, "Foreground", 0.3), (16, 10, 20, 12, "Foreground", 0.6),
              (0, 14, 9, 10, "Background", 0.2)]


def _through_the_delegate(plugin, cuda, monkeypatch, grid, kernel, rgb):
    from PIL import Image
    import sys
    W, H, strength = 40, 28, 0.7
    p = sh.make_processing(W * 8, H * 8)
    smp = sh.kdiff_sampler()
    smp.model_wrap_cfg = SimpleNamespace(step=0, inner_model=SimpleNamespace(forward=None), image_cfg_scale=None)
    cls = plugin.multidiffusion.MultiDiffusion
    cls.is_edit_model = False
    d = cls(p, smp)
    if grid:
        d.init_grid_bbox(16, 16, 4, 2)
    d.enable_grid_bbox = grid
    d.custom_bboxes = [plugin.utils.CustomBBox(x, y, w, h, "", "", m, fr, 1) for (x, y, w, h, m, fr) in NI_REGIONS]
    g = torch.Generator().manual_seed(11)
    noise = torch.randn(2, 4, H, W, generator=g)
    init_latent = torch.randn(2, 4, H, W, generator=g)
    xt = torch.randn(2, 4, H, W, generator=g) * 3.0
    sigmas = torch.linspace(7.5, 0.03, 9)
    pixels = rr.make_image(H * 8, W * 8, seed=21, rgb=rgb)
    p.init_images = [Image.fromarray(pixels)]
    assert p.init_images[0].mode == ("RGB" if rgb else "L") and p.init_images[0].size == (W * 8, H * 8)
    p.sd_model = SimpleNamespace(sd_model_hash="hash")
    p.init_latent = init_latent.to(cuda)
    cache = plugin.utils.NoiseInverseCache("hash", init_latent.clone(), xt, 5, 1.0, [""])
    captured = {}
    smp = d.sampler_raw
    smp.sample_img2img = lambda p_, x_, n_, c_, uc_, steps_=None, ic_=None: captured.setdefault("noise", n_)
    d.init_noise_inverse(5, 1.0, lambda: cache, lambda *a: None, strength, kernel)
    assert plugin.abstractdiffusion.get_retouch_mask is plugin.utils.get_retouch_mask        # the real one
    monkeypatch.setattr(sys.modules["modules.sd_samplers_common"], "setup_img2img_steps", lambda p_, steps: (steps or 8, 6), raising=False)
    smp.get_sigmas = lambda p_, steps: sigmas.to(cuda)
    smp.sample_img2img(p, torch.zeros_like(noise).to(cuda), noise.to(cuda), None, None, 8, None)
    full = torch.from_numpy(rr.retouch_mask(pixels, kernel))
    assert len(torch.unique(full)) > 20                         # a mask with structure, not a constant
    m = 1 - F.interpolate(full[None, None], size=(H, W), mode="bilinear")[0, 0]
    m = torch.clamp(m * strength, 0, 1)
    ref = bo.noise_inverse_blend(noise, xt - init_latent / sigmas[0], m, [bo.Region(*r) for r in NI_REGIONS], grid)
    assert torch.allclose(captured["noise"].cpu(), ref, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("kernel", [3, 64])
@pytest.mark.parametrize("grid", [True, False])
def test_noise_inversion_through_the_delegate_with_the_real_mask(plugin, cuda, grid, kernel, monkeypatch):
    """sample_img2img of the product with a real 320 x 224 RGB init image and get_retouch_mask left alone: the noise handed to the original
    sample_img2img is upstream's composite (:606-681) of the mask the definition gives, resized by torch."""
    _through_the_delegate(plugin, cuda, monkeypatch, grid, kernel, rgb=True)


def test_noise_inversion_through_the_delegate_with_a_grey_init_image(plugin, cuda, monkeypatch):
    """An init image that is not RGB takes the host-side convert("L") branch and goes up as one channel."""
    _through_the_delegate(plugin, cuda, monkeypatch, True, 64, rgb=False)
