"""The img2img upscale on the GPU (csrc/resample.hip): mdtile.resize_u8 is DEFINED as Pillow's 8-bit Image.resize (include/mdtile.h), so it is
compared bit for bit with the numpy restatement tests/resample_ref.py and with Pillow itself.  Then Script.process with nothing stubbed, and
Noise Inversion's renoise mask from the bytes the upscale left on the device."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from hostsim import stub_host as sh
import resample_ref as rr
from test_resample_host import _photo, _process, _upscaler

pytestmark = pytest.mark.gpu

# Kernel geometry (csrc/resample.hip): the horizontal pass runs blocks of 64 output columns x 16 rows, a wave per row, and stages the stretch
# of the input row a strip reads in 4096 bytes of LDS per wave, or reads global memory where that does not fit; taps sit in registers up to
# ksize 8.  The vertical pass runs blocks of 4096 bytes of one output row, 16 per thread, the bytes past the last full 16 one by one.
OWN_PAIRS = [
    ((130, 1030), (520, 4120)),     # 65 strips (the last of 24 columns) x 9 row chunks (the last of 2 rows); rows of 12360 / 4120 bytes = 3 / 1 full
                                    # blocks + 72 / 24 bytes, ending in a run of 8 single bytes
    ((3, 40000), (5, 64)),          # ksize 3751: a strip reads the whole 40000-pixel row, which no LDS slice holds
]
CASES = rr.cases(OWN_PAIRS)


def _pil(filt):
    from PIL import Image
    return Image.Resampling.LANCZOS if filt == rr.LANCZOS else Image.Resampling.NEAREST


@pytest.mark.parametrize("case", CASES, ids=rr.case_id)
def test_resize_is_bitwise_the_definition(plugin, cuda, case):
    E = plugin.engine
    src, dst, filt, rgb = case
    img, want = rr.make_image(src, rgb), torch.from_numpy(rr.expected(*case))
    got = E.resize_u8(torch.from_numpy(img).to(cuda), dst, filt).cpu()
    print(f"resize_u8 {rr.case_id(case)}: {int((got != want).sum()) if got.shape == want.shape else 'shape'} of {want.numel()} bytes differ from the "
          f"restatement, {int(((want == 0) | (want == 255)).sum())} at 0 / 255")
    assert got.dtype == torch.uint8 and got.shape == want.shape
    assert torch.equal(got, want)
    if filt == rr.LANCZOS and rr.hard_edged(src) and dst[0] >= src[0] and dst[1] >= src[1]:
        assert ((want == 0) | (want == 255)).any()          # the clamp was at work
    try:
        from PIL import Image
    except ImportError:
        return
    pil = torch.from_numpy(np.asarray(Image.fromarray(img).resize((dst[1], dst[0]), _pil(filt))).copy())
    print(f"    {int((got != pil).sum())} bytes differ from Pillow")
    assert torch.equal(got, pil)


@pytest.mark.parametrize("filt", [rr.LANCZOS, rr.NEAREST], ids=["lanczos", "nearest"])
@pytest.mark.parametrize("src,dst", [((67, 131), (134, 262)), ((47, 33), (94, 33)), ((33, 47), (33, 94))])
def test_strided_and_misaligned_inputs(plugin, cuda, src, dst, filt):
    """A slice of a wider image (not contiguous) and a contiguous image that starts at an odd byte give the bytes of the plain copy; with the
    width kept, the vertical pass reads the misaligned input itself, 16 bytes at a time."""
    E = plugin.engine
    (h, w) = src
    for rgb in (True, False):
        img = rr.make_image(src, rgb)
        want = torch.from_numpy(rr.resize(img, dst[0], dst[1], filt))
        wide = torch.zeros((h, w + 5) + img.shape[2:], dtype=torch.uint8, device=cuda)
        wide[:, 3:3 + w] = torch.from_numpy(img).to(cuda)
        view = wide[:, 3:3 + w]
        assert not view.is_contiguous()
        assert torch.equal(E.resize_u8(view, dst, filt).cpu(), want)
        flat = torch.zeros(img.size + 1, dtype=torch.uint8, device=cuda)
        flat[1:] = torch.from_numpy(img).to(cuda).reshape(-1)
        odd = flat[1:].view(img.shape)
        assert odd.is_contiguous() and odd.data_ptr() % 2 == 1
        assert torch.equal(E.resize_u8(odd, dst, filt).cpu(), want)


def test_same_size_and_argument_errors(plugin, cuda):
    E = plugin.engine
    img = torch.from_numpy(rr.make_image((33, 47), True)).to(cuda)
    same = E.resize_u8(img, (33, 47), E.RESAMPLE_LANCZOS)              # Pillow returns a copy
    assert torch.equal(same, img) and same.data_ptr() != img.data_ptr()
    assert torch.equal(E.resize_u8(img, (33, 47), E.RESAMPLE_NEAREST), img)
    with pytest.raises(E.MdtileError, match="shape"):
        E.resize_u8(torch.zeros(16, 16, 2, dtype=torch.uint8, device=cuda), (8, 8), E.RESAMPLE_LANCZOS)
    with pytest.raises(E.MdtileError, match="dtype"):
        E.resize_u8(torch.zeros(16, 16, device=cuda), (8, 8), E.RESAMPLE_LANCZOS)
    with pytest.raises(E.MdtileError, match="filter"):
        E.resize_u8(img, (8, 8), 2)
    with pytest.raises(E.MdtileError, match="sizes"):
        E.resize_u8(img, (0, 8), E.RESAMPLE_LANCZOS)


def _upscaled_job(plugin, scale, noise_inverse=False):
    """Script.process on a 96 x 128 RGB init image with the built-in Lanczos upscaler; nothing of the engine is stubbed."""
    _, shared = sh.host()
    up = _upscaler("Lanczos")
    shared.sd_upscalers = [SimpleNamespace(name="None", scaler=None, data_path=None), up]
    first = _photo(128, 96)
    p = sh.make_processing(128, 96, init_images=[first], extra_generation_params={})
    s = _process(plugin, p, "Lanczos", scale, True, noise_inverse=noise_inverse)
    return s, p, first, up


@pytest.mark.parametrize("scale", [2, 2.5])
def test_process_upscales_on_the_engine(plugin, cuda, scale):
    _, shared = sh.host()
    old = shared.sd_upscalers
    s, p, first, up = _upscaled_job(plugin, scale)
    try:
        want = _upscaler("Lanczos").scaler.upscale(first, scale)      # Pillow, as the host runs it
        got = p.init_images[0]
        diff = int((np.asarray(got) != np.asarray(want)).sum()) if got.size == want.size else "size"
        print(f"process, Lanczos x{scale}: {got.size}, {diff} bytes differ from Pillow")
        assert up.scaler.rounds == 0                                   # not a single resize on the host
        assert got.mode == "RGB" and got.size == want.size == (int(128 * scale // 8 * 8), int(96 * scale // 8 * 8))
        assert np.array_equal(np.asarray(got), np.asarray(want))
        assert (p.width, p.height) == got.size
        image, kept = p.init_image_bytes_md
        assert image is got and kept.device.type == "cuda" and np.array_equal(kept.cpu().numpy(), np.asarray(want))
    finally:
        s.postprocess(p, None, True)
        shared.sd_upscalers = old
    assert not hasattr(p, "init_image_bytes_md") and p.init_images[0].size == (128, 96)


def test_renoise_mask_from_the_kept_bytes(plugin, cuda, monkeypatch):
    """The default Noise Inversion job (renoise strength 1, kernel 64) after such a process call: get_retouch_mask gets the tensor the upscale
    left on the device, not host pixels, and both the full-size mask and the renoise mask equal the ones from the host image bit for bit."""
    _, shared = sh.host()
    old = shared.sd_upscalers
    s, p, first, up = _upscaled_job(plugin, 2, noise_inverse=True)
    try:
        absd = plugin.abstractdiffusion
        real = absd.get_retouch_mask
        assert real is plugin.utils.get_retouch_mask
        seen = []

        def wrapped(pixels, k):
            out = real(pixels, k)
            seen.append((pixels, k, out))
            return out
        monkeypatch.setattr(absd, "get_retouch_mask", wrapped)
        cls = plugin.multidiffusion.MultiDiffusion
        cls.is_edit_model = False
        smp = sh.kdiff_sampler()
        smp.sample_img2img = lambda *a, **k: None
        d = cls(p, smp)
        d.init_noise_inverse(10, 1, lambda: None, lambda *a: None, 1, 64)
        size = (p.height // 8, p.width // 8)
        on_device = d.renoise_mask(p, size)
        del p.init_image_bytes_md
        from_host = d.renoise_mask(p, size)
        torch.cuda.synchronize()
        (px0, k0, full0), (px1, k1, full1) = seen
        assert isinstance(px0, torch.Tensor) and px0.device.type == "cuda" and px0.dtype == torch.uint8 and k0 == k1 == 64
        assert isinstance(px1, np.ndarray) and np.array_equal(px0.cpu().numpy(), px1)
        assert tuple(full0.shape) == (p.height, p.width) and len(torch.unique(full0)) > 4         # a mask with structure
        assert torch.equal(full0, full1)
        assert tuple(on_device.shape) == size and torch.equal(on_device, from_host)
    finally:
        s.postprocess(p, None, True)
        shared.sd_upscalers = old
