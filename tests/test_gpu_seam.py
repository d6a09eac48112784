"""Cross-faded tile borders of Tiled VAE on the GPU (csrc/vae_assemble.hip: mdtile_vae_assemble_blend), BITWISE against
the numpy restatement tests/seam_ref.py: the C call on synthetic "finished tiles" (hand-built tables, so the tiles can be tiny), on tables
from mdtile_vae_split_tiles, special values, the refused calls, and the decoder hook with VAEHook.seam_blend.  No tolerance appears in
this file: every comparison is on int views."""
import functools
import re

import numpy as np
import pytest
import torch

from hostsim import ldm_decoder as ld
from hostsim import stub_host as sh

import seam_cases as sc
import seam_ref as sr

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _assert_bitwise(got, ref, what):
    """got (device tensor) == ref (numpy) bit for bit; where the reference is NaN the result must be NaN (payloads of computed NaNs are not
    part of the definition -- copied ones are: see _assert_copied)."""
    got = got.detach().cpu().contiguous()
    ref = torch.from_numpy(np.ascontiguousarray(ref))
    assert got.dtype == ref.dtype == torch.float32 and got.shape == ref.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {ref.dtype} {tuple(ref.shape)}"
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs ({int(torch.isnan(got).sum())} vs {int(nan.sum())} NaNs)"
    gb, rb = got.view(torch.int32), ref.view(torch.int32)
    z = torch.zeros((), dtype=torch.int32)
    bad = torch.where(nan, z, gb) != torch.where(nan, z, rb)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ bitwise; first at {i}: got {got[i].item()!r}, want {ref[i].item()!r}")


def _assert_copied(got, plain, mask, what):
    """Outside the bands (mask false) the image is mdtile_vae_assemble's, NaN payloads included: torch.equal on int views."""
    keep = ~torch.from_numpy(mask).to(got.device)
    a, b = got.contiguous().view(torch.int32)[:, :, keep], plain.contiguous().view(torch.int32)[:, :, keep]
    assert keep.any() and torch.equal(a, b), f"{what}: {int((a != b).sum())} pixels outside the bands differ from mdtile_vae_assemble"


def _result(shape, cuda, misaligned=False):
    """A NaN-filled result (an unwritten pixel shows); misaligned: it starts one element into its storage."""
    n = int(np.prod(shape))
    store = torch.full((n + 16,), NAN, device=cuda)
    out = store[1:1 + n].view(shape) if misaligned else store[:n].view(shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == (4 if misaligned else 0)
    return out


def _upload(tab, cuda):
    return [(torch.from_numpy(t).to(cuda), ib, ob) for t, ib, ob in tab]


def _check_table(E, cuda, tab, rows, cols, RH, RW, band, is_dec, what, misaligned=False):
    N, C = tab[0][0].shape[:2]
    want = sr.assemble_blend(tab, rows, cols, RH, RW, band, is_dec)
    dev = _upload(tab, cuda)
    got = _result((N, C, RH, RW), cuda, misaligned)
    E.vae_assemble_blend(dev, rows, cols, got, band, is_dec)
    _assert_bitwise(got, want, what)
    plain = torch.zeros(N, C, RH, RW, device=cuda)
    E.vae_assemble(dev, plain, is_dec)
    mask = sr.band_mask(tab, rows, cols, RH, RW, band)
    _assert_copied(got, plain, mask, what)
    inside = torch.from_numpy(mask).to(cuda)
    assert not torch.equal(got[:, :, inside], plain[:, :, inside]), f"{what}: the bands changed nothing"


# ---- the C call on synthetic finished tiles ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("special", [False, True], ids=["randn", "special_values"])
@pytest.mark.parametrize("nc", [(2, 3), (1, 4)], ids=["2x3", "1x4"])
@pytest.mark.parametrize("case", list(sc.LEGAL))
def test_blend_assembly_bitwise(plugin, cuda, case, nc, special):
    """Every synthetic grid in both N C pairs; special values (NaN, +-inf, -0.0, denormals, fp32 max) in every tile on both sides of every
    border, inside and outside the bands; the result pre-filled with NaN; in the encoder convention the result starts one element into its
    storage."""
    xs, ys, margin, is_dec, band, _ = sc.LEGAL[case]
    RH, RW = sc.result_size(sc.LEGAL[case])
    tab = sc.table(xs, ys, margin, is_dec, nc[0], nc[1], seed=len(case), special_band=band if special else 0, sub=0 if is_dec else 5)
    if case == "6x6_chunks":
        assert len(tab) > plugin.engine.VAE_ASSEMBLE_CHUNK > plugin.engine.VAE_BLEND_CHUNK
    if special:
        allv = np.concatenate([t.ravel() for t, _, _ in tab])
        assert np.isnan(allv).any() and np.isinf(allv).any() and (np.signbit(allv) & (allv == 0)).any() and ((allv != 0) & (np.abs(allv) < 1e-38)).any()
    _check_table(plugin.engine, cuda, tab, len(ys) - 1, len(xs) - 1, RH, RW, band, is_dec, f"{case} {nc}", misaligned=not is_dec)


def test_encoder_cases_take_both_copy_paths():
    """What makes the encoder-convention cases bite: out boxes at odd origins, RW no multiple of 4, tile pitches that are and are not
    multiples of 4 (the copy between the bands reads 16 bytes at a time only where source and destination have the same phase)."""
    pitches = set()
    for case in ("enc_odd", "enc_1x2", "enc_wide_pitch"):
        xs, ys, margin, is_dec, band, _ = sc.LEGAL[case]
        assert not is_dec
        _, outs, shapes = sc.boxes(xs, ys, margin, is_dec)
        pitches |= {tw for _, tw in shapes}
        if case != "enc_wide_pitch":
            assert xs[-1] % 4 and any(o[0] % 2 for o in outs)
    assert any(p % 4 == 0 for p in pitches) and any(p % 4 for p in pitches)


# ---- tables from mdtile_vae_split_tiles ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,ts,band,grid", [(64, 64, 16, 16, (3, 3)), (64, 64, 16, 64, (3, 3)), (96, 80, 32, 88, (3, 2))],
                         ids=["64x64_b16", "64x64_b64_touch", "96x80_b88_margin"])
def test_blend_assembly_on_split_tiles_tables(plugin, cuda, h, w, ts, band, grid):
    """The decoder's real geometry: 88 px of padding between out boxes of 216 / 128 / 168 px (bands of 64 touch in the interior tile) and
    of 344 / 296 x 344 / 256 / 168 px with b = 88, the whole padding."""
    E = plugin.engine
    ins, outs = E.vae_split_tiles(h, w, ts, True)
    assert len(ins) == grid[0] * grid[1]
    rng = np.random.RandomState(h + band)
    tab = [(rng.standard_normal((1, 3, (ib[3] - ib[2]) * 8, (ib[1] - ib[0]) * 8)).astype(np.float32), tuple(ib), tuple(ob)) for ib, ob in zip(ins, outs)]
    _check_table(E, cuda, tab, grid[0], grid[1], h * 8, w * 8, band, True, f"split_tiles {h}x{w} b={band}")


# ---- refused calls ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(sc.ILLEGAL) + ["hole", "tile_count"])
def test_refused_calls_write_nothing(plugin, cuda, case):
    """Every illegal grid of the host test, band < 1, and a table that is no rows x cols: an error whose text names the reason, and the
    NaN-filled result untouched."""
    E = plugin.engine
    if case in ("hole", "tile_count"):
        xs, ys, margin, is_dec, band, _ = sc.LEGAL["2x2_b1"]
        tab, why = sc.table(xs, ys, margin, is_dec, 1, 4), "grid"
        if case == "hole":
            tab = sc.with_hole(tab)
    else:
        xs, ys, margin, is_dec, band, why = sc.ILLEGAL[case]
        tab = sc.table(xs, ys, margin, is_dec, 1, 4)
    rows, cols = len(ys) - 1, len(xs) - 1
    dev = _upload(tab, cuda)
    if case == "tile_count":
        dev = dev[:-1]
    out = _result((1, 4, ys[-1], xs[-1]), cuda)
    with pytest.raises(E.MdtileError, match=sc.REASON_TEXT[why]) as err:
        E.vae_assemble_blend(dev, rows, cols, out, band, is_dec)
    assert re.search(r"tile \d+|band|tiles are no", str(err.value))
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote to its result"


# ---- the hook ------------------------------------------------------------------------------------------------------------------------
BAND = 16


def _decoder():
    dec = ld.make_decoder(0, small=True).cuda()
    dec.original_forward = dec.forward
    return dec


def _latent(cuda):
    torch.manual_seed(13)
    return torch.randn(1, 4, 64, 64, device=cuda)              # 9 tiles at tile 16


def _run(plugin, cuda, fast, seam, devices=None, record=None, z=None):
    hook = plugin.tilevae.VAEHook(_decoder(), 16, is_decoder=True, fast_decoder=fast, fast_encoder=False, color_fix=False)
    hook.seam_blend = seam
    hook.devices = devices
    E = plugin.engine
    real = E.vae_assemble_blend

    def recording(tiles, rows, cols, result, band, is_decoder=True):
        if record is not None:
            record.append((tiles, rows, cols, band, is_decoder))
        return real(tiles, rows, cols, result, band, is_decoder)

    E.vae_assemble_blend = recording
    try:
        with torch.no_grad():
            return hook(_latent(cuda) if z is None else z).clone()
    finally:
        E.vae_assemble_blend = real


@functools.lru_cache(maxsize=None)
def _images(fast):
    """(option-off image, image with seam_blend = 16, what the hook handed to the assembly), once per mode."""
    plugin, cuda = sh.load_plugin(), torch.device("cuda:0")
    calls = []
    off = _run(plugin, cuda, fast, 0, record=calls)
    assert calls == [], "without the option vae_assemble_blend is never called"
    on = _run(plugin, cuda, fast, BAND, record=calls)
    assert len(calls) == 1
    tiles, rows, cols, band, is_dec = calls[0]
    assert (rows, cols, band, is_dec) == (3, 3, BAND, True) and len(tiles) == 9
    tab = [(t.cpu().numpy(), tuple(ib), tuple(ob)) for t, ib, ob in tiles]
    return off, on, tab


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "slow"])
def test_hook_image_is_the_restatement_of_its_tiles(plugin, cuda, fast):
    """The image equals the restatement applied to the tiles and boxes the hook handed to the assembly; outside the bands it is the
    option-off image bit for bit, inside at least one band it differs."""
    off, on, tab = _images(fast)
    assert on.shape == off.shape == (1, 3, 512, 512)
    _assert_bitwise(on, sr.assemble_blend(tab, 3, 3, 512, 512, BAND, True), f"hook fast={fast}")
    mask = sr.band_mask(tab, 3, 3, 512, 512, BAND)
    _assert_copied(on, off, mask, f"hook fast={fast} vs option off")
    inside = torch.from_numpy(mask).to(cuda)
    assert not torch.equal(on[:, :, inside], off[:, :, inside]), "the option changed nothing"
    for i, (t, ib, ob) in enumerate(tab):                 # the narrowed input bbox still satisfies the margin rule
        r, c = divmod(i, 3)
        ml, mr, mt, mb = sr.margins(ib, ob, True)
        assert all(m >= BAND for m, has in ((ml, c > 0), (mr, c < 2), (mt, r > 0), (mb, r < 2)) if has)
        if fast:
            assert all(m == 24 for m, has in ((ml, c > 0), (mr, c < 2), (mt, r > 0), (mb, r < 2)) if has), "live windows: ceil(16 / 8) + 1 latent px"


def test_hook_without_live_windows_gives_the_same_bits(plugin, cuda, monkeypatch):
    """The valid rectangle handed to live_windows grows by ceil(b / 8) latent px: the band is exactly what a whole-tile decode yields."""
    _, on, _ = _images(True)
    monkeypatch.setattr(plugin.tilevae, "LIVE_WINDOW", False)
    calls = []
    whole = _run(plugin, cuda, True, BAND, record=calls)
    ins, _ = plugin.engine.vae_split_tiles(64, 64, 16, True)
    assert [tuple(ib) for _, ib, _ in calls[0][0]] == [tuple(ib) for ib in ins]
    assert torch.equal(whole.view(torch.int32), on.view(torch.int32))


@pytest.mark.parametrize("fast", [True, False], ids=["fast", "slow"])
def test_hook_on_two_slots_gives_the_same_bits(plugin, cuda, fast):
    _, on, _ = _images(fast)
    many = _run(plugin, cuda, fast, BAND, devices=[0, 0])
    assert torch.equal(many.view(torch.int32), on.view(torch.int32))


def test_hook_composes_with_wrap_x(plugin, cuda):
    """--mdtile-wrap-x and seam_blend together: the option pair applied by hand -- pad with the columns of the other edge, blend-decode,
    crop -- bit for bit."""
    _, shared = sh.host()
    z = _latent(cuda)[..., :48].contiguous()
    P = 11
    shared.cmd_opts.mdtile_wrap_x = True
    try:
        calls = []
        got = _run(plugin, cuda, True, BAND, record=calls, z=z)
    finally:
        del shared.cmd_opts.mdtile_wrap_x
    assert len(calls) == 1
    padded = _run(plugin, cuda, True, BAND, z=torch.cat([z[..., -P:], z, z[..., :P]], dim=-1))
    want = padded[..., 8 * P:padded.shape[-1] - 8 * P]
    assert got.shape == want.shape == (1, 3, 512, 384)
    assert torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))
    plain = _run(plugin, cuda, True, 0, z=z)
    assert not torch.equal(got, plain)
