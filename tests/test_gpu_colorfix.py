"""The colour fix on the GPU (csrc/colorfix.hip): mdtile.colorfix_wavelet is DEFINED as the integer form of include/mdtile.h, so it is compared
bit for bit with the numpy restatement tests/colorfix_ref.py; the histogram with bincount, the table apply and colorfix_adain with the host
composition; then beside an MFMA kernel, and Script.process + postprocess_image with nothing stubbed."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from hostsim import stub_host as sh
import colorfix_ref as cr
from colorfix_helpers import apply_lut, lanczos_upscalers, photo, process, set_option

pytestmark = pytest.mark.gpu

# Kernel geometry (csrc/colorfix.hip): the vertical pass runs blocks of 64 rows x 64 flat columns (bytes of a row) with 31 rows of halo, 4 columns
# per thread and the bytes past the last full 4 of a row one by one; the horizontal pass runs blocks of 1024 pixels of one row with 31 pixels of
# halo and writes 4 bytes per thread, the last bytes of a strip one by one.
OWN_SHAPES = [
    (129, 2079, 3),     # crosses every block boundary in both axes: 3 row blocks (64 + 64 + a last block of ONE row), 98 column blocks of the
                        # 6237-byte rows (the last of 29 bytes: 7 full 4s + 1 byte), 3 strips of 1024 + 1024 + 31 pixels (93 bytes: 23 4s + 1 byte)
    (65, 1025, 1),      # every tail is ONE: a last strip of one pixel, a last column block of one byte, a last row block of one row
]
CASES = cr.cases(OWN_SHAPES)
_WANT = {}


def _want(case):
    """(content, style, restatement) of a case, computed once and shared; the arrays are not written to."""
    if case not in _WANT:
        content, style = cr.make_pair(*case)
        _WANT[case] = (content, style, cr.wavelet_int(content, style))
    return _WANT[case]


@pytest.mark.parametrize("case", CASES, ids=cr.case_id)
def test_wavelet_is_bitwise_the_definition(plugin, cuda, case):
    E = plugin.engine
    content, style, want = _want(case)
    got = E.colorfix_wavelet(torch.from_numpy(content).to(cuda), torch.from_numpy(style).to(cuda)).cpu()
    want_t = torch.from_numpy(want)
    print(f"colorfix_wavelet {cr.case_id(case)}: {int((got != want_t).sum()) if got.shape == want_t.shape else 'shape'} of {want.size} bytes differ "
          f"from the restatement")
    assert got.dtype == torch.uint8 and got.shape == want_t.shape
    assert torch.equal(got, want_t)


def test_the_cases_are_not_vacuous():
    """Checked on the restatement alone: the random cases move most bytes and clamp some, the two-level cases sit at the limits and reach the
    largest intermediate value the int32 arithmetic has to hold."""
    extremes = 0
    for case in CASES:
        (h, w, c), kind = case
        if h < 17 or w < 32:
            continue
        content, style, want = _want(case)
        limits = float(((want == 0) | (want == 255)).mean())
        changed = float((want != content).mean())
        v = cr.low5_int(cr._hwc(style).astype(np.int64) - cr._hwc(content).astype(np.int64))
        top = int((np.abs(v) == 255 << cr.SHIFT).sum())
        print(f"{cr.case_id(case)}: {limits:.4f} at 0 / 255, {changed:.4f} differ from the content, {top} values at +-255 * 2^20")
        if kind == "random":
            assert limits > 0 and changed > 0.8
        if kind.startswith("two_level"):
            assert limits >= 0.3
        if kind == "two_level_inverse" and h >= 64 and w >= 64:
            assert top > 0
            extremes += 1
    assert extremes >= 5


@pytest.mark.parametrize("shape", [(67, 131, 3), (47, 33, 1), (130, 1100, 3)], ids=lambda s: "x".join(map(str, s)))
def test_strided_and_misaligned_inputs(plugin, cuda, shape):
    """A slice of a wider image (not contiguous) and a contiguous image that starts at an odd byte give the bytes of the plain copy: both passes
    and the pointwise kernels read 4 or 16 bytes at a time from rows that start anywhere."""
    E = plugin.engine
    h, w, c = shape
    content, style = cr.make_pair(shape, "random")
    want = torch.from_numpy(cr.wavelet_int(content, style))
    want_adain = torch.from_numpy(cr.adain_pixels(content, style))
    want_hist = torch.from_numpy(cr.hist(content))

    def views(img):
        wide = torch.zeros((h, w + 5) + img.shape[2:], dtype=torch.uint8, device=cuda)
        wide[:, 3:3 + w] = torch.from_numpy(img).to(cuda)
        view = wide[:, 3:3 + w]
        assert not view.is_contiguous()
        flat = torch.zeros(img.size + 1, dtype=torch.uint8, device=cuda)
        flat[1:] = torch.from_numpy(img).to(cuda).reshape(-1)
        odd = flat[1:].view(img.shape)
        assert odd.is_contiguous() and odd.data_ptr() % 2 == 1
        return view, odd

    (cv, co), (sv, so) = views(content), views(style)
    plain = torch.from_numpy(style).to(cuda)
    assert torch.equal(E.colorfix_wavelet(cv, sv).cpu(), want)
    assert torch.equal(E.colorfix_wavelet(co, so).cpu(), want)
    assert torch.equal(E.colorfix_wavelet(co, plain).cpu(), want)
    assert torch.equal(E.hist_u8(cv).cpu(), want_hist) and torch.equal(E.hist_u8(co).cpu(), want_hist)
    assert torch.equal(E.colorfix_adain(cv, so).cpu(), want_adain) and torch.equal(E.colorfix_adain(co, sv).cpu(), want_adain)


HIST_IMAGES = {
    "1x1x1": lambda: np.array([[9]], np.uint8),
    "flat": lambda: np.full((300, 500, 3), 200, np.uint8),                  # every lane of every wave adds to one bin per channel
    "flat_grey": lambda: np.full((257, 129), 0, np.uint8),
    "random": lambda: cr.make_pair((97, 200, 3), "random")[0],
    "ramps_grey": lambda: cr.make_pair((130, 67, 1), "ramps")[0],
    "many_blocks": lambda: np.random.default_rng(5).integers(0, 256, size=(1500, 2000, 3), dtype=np.uint8),   # 9 MB: every block strides twice
}


@pytest.mark.parametrize("name", list(HIST_IMAGES))
def test_hist_is_bincount(plugin, cuda, name):
    E = plugin.engine
    img = HIST_IMAGES[name]()
    got = E.hist_u8(torch.from_numpy(img).to(cuda))
    assert got.dtype == torch.int64 and tuple(got.shape) == (1 if img.ndim == 2 else 3, 256)
    assert torch.equal(got.cpu(), torch.from_numpy(cr.hist(img)))
    assert int(got.sum()) == img.size


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 3, 3), (97, 200, 3), (130, 67, 1), (129, 2079, 3)], ids=lambda s: "x".join(map(str, s)))
def test_lut_and_adain_equal_the_host_composition(plugin, cuda, shape):
    E = plugin.engine
    content, style = cr.make_pair(shape, "random")
    d_content, d_style = torch.from_numpy(content).to(cuda), torch.from_numpy(style).to(cuda)
    lut = np.random.default_rng(shape[1]).integers(0, 256, size=(shape[2], 256), dtype=np.uint8)
    assert torch.equal(E.lut_u8(d_content, lut).cpu(), torch.from_numpy(apply_lut(lut, content)))
    assert torch.equal(E.lut_u8(d_content, torch.from_numpy(lut).to(cuda)).cpu(), torch.from_numpy(apply_lut(lut, content)))
    host = apply_lut(E.adain_lut(cr.hist(content), cr.hist(style)), content)
    assert np.array_equal(host, cr.adain_pixels(content, style))
    assert torch.equal(E.colorfix_adain(d_content, d_style).cpu(), torch.from_numpy(host))
    # a style of another size, and a flat content: finite and equal to the restatement
    small = cr.make_pair((5, 9, shape[2]), "ramps")[1]
    assert torch.equal(E.colorfix_adain(d_content, torch.from_numpy(small).to(cuda)).cpu(), torch.from_numpy(cr.adain_pixels(content, small)))
    flat = np.full_like(content, 90)
    assert torch.equal(E.colorfix_adain(torch.from_numpy(flat).to(cuda), d_style).cpu(), torch.from_numpy(cr.adain_pixels(flat, style)))


def test_argument_errors(plugin, cuda):
    E = plugin.engine
    img = torch.zeros(16, 16, 3, dtype=torch.uint8, device=cuda)
    with pytest.raises(E.MdtileError, match="shape"):
        E.colorfix_wavelet(torch.zeros(16, 16, 2, dtype=torch.uint8, device=cuda), torch.zeros(16, 16, 2, dtype=torch.uint8, device=cuda))
    with pytest.raises(E.MdtileError, match="does not match"):
        E.colorfix_wavelet(img, img[:8])
    with pytest.raises(E.MdtileError, match="does not match"):
        E.colorfix_wavelet(img, img[:, :, 0])
    with pytest.raises(E.MdtileError, match="dtype"):
        E.colorfix_wavelet(img.float(), img)
    with pytest.raises(E.MdtileError, match="empty"):
        E.hist_u8(img[:0])
    with pytest.raises(E.MdtileError, match="lut"):
        E.lut_u8(img, np.zeros((1, 256), np.uint8))
    same = E.colorfix_wavelet(img + 7, img + 7)
    assert torch.equal(same, img + 7)                                  # style == content returns the content


def _coef(B, C, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.rand(B, 1, C, generator=g) * 1.5 + 0.25, torch.randn(B, 1, C, generator=g) * 0.5], dim=1).contiguous().to(dev)


def test_wavelet_is_the_same_next_to_an_mfma_kernel(plugin, cuda):
    """Integer sums: the same bytes with the CUs shared with a split-bf16 MFMA conv that another stream launched (one run, as
    tests/test_gpu_coresidency.py does it)."""
    E, dev = plugin.engine, cuda
    content, style = cr.make_pair((1024, 1536, 3), "random")
    d_content, d_style = torch.from_numpy(content).to(dev), torch.from_numpy(style).to(dev)
    alone = E.colorfix_wavelet(d_content, d_style)
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
    beside = E.colorfix_wavelet(d_content, d_style)
    side.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(beside, alone)
    assert torch.equal(alone.cpu(), torch.from_numpy(cr.wavelet_int(content, style)))


@pytest.mark.parametrize("option", ["wavelet", "adain", None])
def test_process_and_postprocess_image_unstubbed(plugin, cuda, monkeypatch, option):
    """A 328 x 520 photo upscaled 2x by the built-in Lanczos upscaler, then the host's per-image hook on a decoded result of that size: with the
    option the saved image is the restatement applied to the host-side images, without it the image is left alone."""
    _, shared = sh.host()
    set_option(monkeypatch, option)
    monkeypatch.setattr(shared, "sd_upscalers", lanczos_upscalers())
    p = sh.make_processing(520, 328, init_images=[photo(520, 328)], extra_generation_params={})
    s = process(plugin, p, "Lanczos", 2)
    try:
        init = p.init_images[0]
        assert init.size == (1040, 656) and p.init_image_bytes_md[0] is init and p.init_image_bytes_md[1].device.type == "cuda"
        result = photo(1040, 656, seed=11)
        pp = SimpleNamespace(image=result)
        s.postprocess_image(p, pp, True)
        if option is None:
            assert pp.image is result and "Tiled Diffusion color fix" not in p.extra_generation_params
            return
        restate = cr.wavelet_int if option == "wavelet" else cr.adain_pixels
        want = restate(np.asarray(result), np.asarray(init))
        got = np.asarray(pp.image)
        print(f"postprocess_image, {option}: {int((got != want).sum())} of {want.size} bytes differ from the restatement, "
              f"{float((want != np.asarray(result)).mean()):.3f} of the bytes changed")
        assert pp.image is not result and pp.image.mode == "RGB" and pp.image.size == result.size
        assert np.array_equal(got, want) and (want != np.asarray(result)).mean() > 0.5
        assert p.extra_generation_params["Tiled Diffusion color fix"] == option
        assert hasattr(p, "init_image_bytes_md")                      # still there for the next image of the job
    finally:
        s.postprocess(p, None, True)
    assert not hasattr(p, "init_image_bytes_md") and p.init_images[0].size == (520, 328)
