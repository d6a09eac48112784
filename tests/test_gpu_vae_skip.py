"""Tiled VAE tile skipping for inpaint jobs on the GPU (csrc/vae_skip.hip), BITWISE against the numpy restatement
tests/vae_skip_ref.py: mdtile_mask_activity_u8, mdtile_vae_assemble_sparse (also against mdtile_vae_assemble), the refused calls, and the
decoder hook with VAEHook.inpaint_job.  No tolerance appears in this file: every comparison of images is on int views."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

from hostsim import ldm_decoder as ld
from hostsim import stub_host as sh

import seam_cases as sc
import vae_skip_ref as vr

pytestmark = pytest.mark.gpu

NAN = float("nan")
NOT_APPLIED = "--mdtile-vae-inpaint-skip not applied:"


def _same_bits(got, ref, what):
    """got (device tensor) == ref (numpy) as int32, NaN payloads included: everything here is copied or computed without NaN."""
    got = got.detach().cpu().contiguous()
    ref = torch.from_numpy(np.ascontiguousarray(ref))
    assert got.dtype == ref.dtype == torch.float32 and got.shape == ref.shape, f"{what}: {tuple(got.shape)} vs {tuple(ref.shape)}"
    bad = got.view(torch.int32) != ref.view(torch.int32)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ bitwise; first at {i}: got {got[i].item()!r}, want {ref[i].item()!r}")


def _result(shape, cuda, misaligned=True):
    """A NaN-filled result (an unwritten pixel shows); misaligned: it starts one element (4 bytes) into its storage."""
    n = int(np.prod(shape))
    store = torch.full((n + 16,), NAN, device=cuda)
    out = store[1:1 + n].view(shape) if misaligned else store[:n].view(shape)
    assert out.is_contiguous() and out.data_ptr() % 16 == (4 if misaligned else 0)
    return out


# ---- activity -------------------------------------------------------------------------------------------------------------------------
def _odd_boxes():
    """Hand-made boxes with odd x1 and widths 1, 3, 15, 17 and 65 in a 203-px-wide mask (a row pitch that is no multiple of 16); they
    share borders, so that a byte one pixel outside one lies in its neighbour."""
    boxes, x = [], 1
    for w in (1, 3, 15, 17, 65, 1, 17, 3, 65, 15):
        boxes.append((x, x + w, 3, 20))
        x += w
    assert x == 203 and any(b[0] % 2 for b in boxes)
    return boxes + [(1, 66, 20, 37), (66, 67, 20, 37), (67, 203, 20, 21), (67, 203, 21, 37)], 37, 203


GRIDS = {"64x64_t16": (64, 64, 16), "40x72_t16": (40, 72, 16), "36x44_t16": (36, 44, 16), "odd_boxes": None}


def _geometry(E, name):
    if GRIDS[name] is None:
        return _odd_boxes()
    h, w, ts = GRIDS[name]
    _, outs = E.vae_split_tiles(h, w, ts, True)
    return [tuple(o) for o in outs], 8 * h, 8 * w


def _box_with_room(boxes, RH, RW, side=None):
    """The first box with a pixel of the mask next to it on `side` (None: on every side, failing that to its left and right, failing that
    the last box)."""
    room = {"left": lambda b: b[0] > 0, "right": lambda b: b[1] < RW, "above": lambda b: b[2] > 0, "below": lambda b: b[3] < RH}
    if side is not None:
        return next((i for i, b in enumerate(boxes) if room[side](b)), None)
    for sides in (list(room), ["left", "right"]):
        i = next((i for i, b in enumerate(boxes) if all(room[k](b) for k in sides)), None)
        if i is not None:
            return i
    return len(boxes) - 1


def _check_activity(E, cuda, mask, boxes, what):
    want = vr.activity(mask, boxes)
    got = E.mask_activity_u8(torch.from_numpy(mask).to(cuda), boxes)
    assert got == want, f"{what}: got {got}, want {want}"
    return got


@pytest.mark.parametrize("grid", list(GRIDS))
def test_activity_matches_the_restatement(plugin, cuda, grid):
    """All zero, all 255, random sparse masks; the grids of mdtile_vae_split_tiles (out boxes at x = 8 mod 16: the 16-byte path has a head
    and a tail) and the hand-made odd boxes."""
    E = plugin.engine
    boxes, RH, RW = _geometry(E, grid)
    if grid == "36x44_t16":
        assert any(b[0] % 16 == 8 for b in boxes)
    if grid == "odd_boxes":
        assert RW % 16
    assert _check_activity(E, cuda, np.zeros((RH, RW), np.uint8), boxes, "zeros") == [0] * len(boxes)
    assert _check_activity(E, cuda, np.full((RH, RW), 255, np.uint8), boxes, "255") == [1] * len(boxes)
    rng = np.random.RandomState(len(grid))
    for k in range(4):
        m = np.zeros((RH, RW), np.uint8)
        for _ in range(k + 1):
            m[rng.randint(RH), rng.randint(RW)] = rng.randint(1, 256)
        _check_activity(E, cuda, m, boxes, f"{k + 1} random bytes")
    # the mask as a view at an odd address: no 16-byte load of it is aligned to the allocation
    m = np.zeros((RH, RW), np.uint8)
    m[RH - 1, RW - 1] = 1
    store = torch.zeros(RH * RW + 16, dtype=torch.uint8, device=cuda)
    view = store[3:3 + RH * RW].view(RH, RW)
    view.copy_(torch.from_numpy(m))
    assert E.mask_activity_u8(view, boxes) == vr.activity(m, boxes)


@pytest.mark.parametrize("corner", ["top_left", "top_right", "bottom_left", "bottom_right"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_one_byte_in_a_corner_of_an_interior_box(plugin, cuda, grid, corner):
    E = plugin.engine
    boxes, RH, RW = _geometry(E, grid)
    i = _box_with_room(boxes, RH, RW)
    x1, x2, y1, y2 = boxes[i]
    x, y = (x1 if "left" in corner else x2 - 1), (y1 if "top" in corner else y2 - 1)
    m = np.zeros((RH, RW), np.uint8)
    m[y, x] = 1
    got = _check_activity(E, cuda, m, boxes, f"{grid} {corner}")
    assert got[i] == 1 and sum(got) == 1


@pytest.mark.parametrize("side", ["left", "right", "above", "below"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_one_byte_just_outside_a_box_flags_the_neighbour(plugin, cuda, grid, side):
    E = plugin.engine
    boxes, RH, RW = _geometry(E, grid)
    i = _box_with_room(boxes, RH, RW, side)
    if i is None:          # every box reaches that edge of the mask (a grid of one row): there is no pixel outside on that side
        assert side in ("above", "below") and all(b[2] == 0 and b[3] == RH for b in boxes)
        return
    x1, x2, y1, y2 = boxes[i]
    x, y = {"left": (x1 - 1, y1), "right": (x2, y2 - 1), "above": (x1, y1 - 1), "below": (x2 - 1, y2)}[side]
    holders = sum(1 for b in boxes if b[0] <= x < b[1] and b[2] <= y < b[3])      # the hand-made list leaves a margin no box covers
    assert holders <= 1 and (holders == 1 or GRIDS[grid] is None)
    m = np.zeros((RH, RW), np.uint8)
    m[y, x] = 255
    got = _check_activity(E, cuda, m, boxes, f"{grid} {side}")
    assert got[i] == 0 and sum(got) == holders


@pytest.mark.parametrize("case", ["box_right_of_the_mask", "box_below_the_mask", "negative_origin", "empty_box", "no_boxes", "too_many_boxes"])
def test_refused_activity_calls_write_nothing(plugin, cuda, case):
    E = plugin.engine
    RH, RW = 24, 40
    good = [(0, 16, 0, 24), (16, 40, 0, 24)]
    boxes, n, words = {
        "box_right_of_the_mask": (good + [(16, 41, 0, 24)], 3, "box 2.*outside"),
        "box_below_the_mask": ([(0, 16, 0, 25)] + good, 3, "box 0.*outside"),
        "negative_origin": (good + [(-1, 16, 0, 24)], 3, "box 2.*outside"),
        "empty_box": (good + [(16, 16, 0, 24)], 3, "box 2.*empty"),
        "no_boxes": (good, 0, "n_boxes 0"),
        "too_many_boxes": (good, E.MASK_ACTIVITY_MAX_BOXES + 1, "n_boxes 4097"),
    }[case]
    mask = torch.full((RH, RW), 255, dtype=torch.uint8, device=cuda)
    d_boxes = torch.tensor(boxes, dtype=torch.int32, device=cuda)
    flags = torch.full((8,), -77, dtype=torch.int32, device=cuda)
    rc = E.lib().mdtile_mask_activity_u8(mask.data_ptr(), RH, RW, d_boxes.data_ptr(), n, flags.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == E.E_ARG
    import re
    assert re.search(words, E.lib().mdtile_last_error().decode()), E.lib().mdtile_last_error()
    assert (flags == -77).all(), "a refused call wrote to the flags"
    if case.startswith("box") or case in ("negative_origin", "empty_box"):
        with pytest.raises(E.MdtileError, match=words):
            E.mask_activity_u8(mask, boxes)


# ---- assembly -------------------------------------------------------------------------------------------------------------------------
DECODER_CASES = [c for c in sc.LEGAL if sc.LEGAL[c][3]]
SPLIT_CASES = {"split_64x64_t16": (64, 64, 16), "split_40x72_t16": (40, 72, 16)}


@functools.lru_cache(maxsize=None)
def _table(case, N):
    """(table, RH, RW) with C = 3 and the special values of seam_cases.SPECIALS in every tile."""
    if case in SPLIT_CASES:
        h, w, ts = SPLIT_CASES[case]
        ins, outs = sh.load_plugin().engine.vae_split_tiles(h, w, ts, True)
        rng = np.random.RandomState(h + w + N)
        tab = []
        for i, (ib, ob) in enumerate(zip(ins, outs)):
            t = rng.standard_normal((N, 3, (ib[3] - ib[2]) * 8, (ib[1] - ib[0]) * 8)).astype(np.float32)
            flat = t.reshape(-1)
            flat[i::7] = sc.SPECIALS[np.arange(len(flat[i::7])) % len(sc.SPECIALS)]
            tab.append((t, tuple(ib), tuple(ob)))
        return tab, 8 * h, 8 * w
    xs, ys, margin, is_dec, band, _ = sc.LEGAL[case]
    RH, RW = sc.result_size(sc.LEGAL[case])
    return sc.table(xs, ys, margin, True, N, 3, seed=len(case) + N, special_band=1), RH, RW


def _present_sets(n):
    sets = {"none": [], "one": [n // 2], "checkerboard": list(range(0, n, 2)), "all_but_one": [i for i in range(n) if i != n // 2], "all": list(range(n))}
    return sets


@pytest.mark.parametrize("N", [1, 2])
@pytest.mark.parametrize("case", DECODER_CASES + list(SPLIT_CASES))
def test_sparse_assembly_bitwise(plugin, cuda, case, N):
    """No tile, one, a checkerboard, all but one and all of them present; with a fill image and with NULL; the result pre-filled with NaN
    and 4 bytes off a 16-byte boundary; NaN, +-inf, -0.0, denormals and fp32 max in the tiles, copied as bits.  With every tile present
    the image is mdtile_vae_assemble's."""
    E = plugin.engine
    tab, RH, RW = _table(case, N)
    allv = np.concatenate([t.ravel() for t, _, _ in tab])
    assert np.isnan(allv).any() and np.isinf(allv).any() and (np.signbit(allv) & (allv == 0)).any() and ((allv != 0) & (np.abs(allv) < 1e-38)).any()
    dev = [(torch.from_numpy(t).to(cuda), ib, ob) for t, ib, ob in tab]
    fill = np.random.RandomState(RH + RW).randint(0, 256, size=(RH, RW, 3)).astype(np.uint8)
    fill[0, 0], fill[-1, -1] = (0, 255, 128), (255, 0, 127)
    d_fill = torch.from_numpy(fill).to(cuda)
    if case == "6x6_chunks":
        assert len(tab) > E.VAE_ASSEMBLE_CHUNK
    for name, present in _present_sets(len(tab)).items():
        tiles = [dev[i] for i in present]
        boxes = [tab[i][2] for i in range(len(tab)) if i not in present]
        for f_np, f_dev in ((fill, d_fill), (None, None)):
            want = vr.assemble_sparse([tab[i] for i in present], boxes, f_np, N, 3, RH, RW)
            got = _result((N, 3, RH, RW), cuda)
            E.vae_assemble_sparse(tiles, boxes, f_dev, got)
            _same_bits(got, want, f"{case} N={N} {name} fill={'yes' if f_np is not None else 'NULL'}")
        if name == "all":
            plain = _result((N, 3, RH, RW), cuda)
            E.vae_assemble(dev, plain, True)
            assert torch.equal(got.contiguous().view(torch.int32), plain.contiguous().view(torch.int32)), "all tiles present: mdtile_vae_assemble's bits"


def test_more_fill_boxes_than_one_launch_takes(plugin, cuda):
    """A grid of 8-px boxes, more than VAE_FILL_CHUNK of them, no tile: the fill alone, chunked through the kernel arguments."""
    E = plugin.engine
    RH, RW = 96, 136
    boxes = [(x, x + 8, y, y + 8) for y in range(0, RH, 8) for x in range(0, RW, 8)]
    assert len(boxes) > E.VAE_FILL_CHUNK
    fill = np.random.RandomState(3).randint(0, 256, size=(RH, RW, 3)).astype(np.uint8)
    got = _result((2, 3, RH, RW), cuda)
    E.vae_assemble_sparse([], boxes, torch.from_numpy(fill).to(cuda), got)
    _same_bits(got, vr.assemble_sparse([], boxes, fill, 2, 3, RH, RW), "fill only")


@pytest.mark.parametrize("case", ["area_short_by_one_box", "box_is_tile_and_fill", "fill_boxes_overlap", "fill_box_outside", "fill_on_the_host"])
def test_refused_assembly_calls_write_nothing(plugin, cuda, case):
    E = plugin.engine
    tab, RH, RW = _table("3x3_b1", 1)
    dev = [(torch.from_numpy(t).to(cuda), ib, ob) for t, ib, ob in tab]
    present = [0, 4, 8]
    tiles = [dev[i] for i in present]
    boxes = [tab[i][2] for i in range(9) if i not in present]
    fill = torch.zeros(RH, RW, 3, dtype=torch.uint8, device=cuda)
    boxes, words = {
        "area_short_by_one_box": (boxes[:-1], "area sum"),
        "box_is_tile_and_fill": (boxes + [tab[4][2]], "also tile 1's out box"),
        "fill_boxes_overlap": (boxes + [boxes[0]], "overlap"),
        "fill_box_outside": (boxes[:-1] + [(boxes[-1][0], RW + 8, boxes[-1][2], boxes[-1][3])], "outside"),
        "fill_on_the_host": (boxes, "no CPU fallback"),
    }[case]
    if case != "fill_on_the_host":
        assert vr.check_sparse([tab[i] for i in present], boxes, RH, RW) is not None
    out = _result((1, 3, RH, RW), cuda)
    with pytest.raises(E.MdtileError, match=words):
        E.vae_assemble_sparse(tiles, boxes, fill.cpu() if case == "fill_on_the_host" else fill, out)
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "a refused call wrote to its result"


# ---- the hook ---------------------------------------------------------------------------------------------------------------------------
SIZE = (512, 512)
CENTRE, CORNER = 4, 8          # the tiles the main case's mask touches: x 216..344, y 216..344 and x 344..512, y 344..512


def _decoder():
    dec = ld.make_decoder(0, small=True).cuda()
    dec.original_forward = dec.forward
    return dec


def _latent(cuda):
    torch.manual_seed(13)
    return torch.randn(1, 4, 64, 64, device=cuda)              # 9 tiles at tile 16


def _mask_image(size=SIZE, blob=True, pixel=True, value=None):
    m = np.zeros((size[1], size[0]), dtype=np.uint8) if value is None else np.full((size[1], size[0]), value, dtype=np.uint8)
    if blob:
        yy, xx = np.mgrid[:size[1], :size[0]]
        m[(yy - 280) ** 2 + (xx - 270) ** 2 < 40 ** 2] = 255      # inside the centre tile's out box
    if pixel:
        m[size[1] - 1, size[0] - 1] = 1
    return Image.fromarray(m, mode="L")


def _init_image(size=SIZE):
    return Image.fromarray(np.random.RandomState(5).randint(0, 256, size=(size[1], size[0], 3)).astype(np.uint8), mode="RGB")


def _job(**over):
    kw = dict(mask_for_overlay=_mask_image(), overlay_images=[object()], inpaint_full_res=False, color_corrections=None, init_images=[_init_image()])
    kw.update(over)
    return SimpleNamespace(**kw)


def _run(plugin, cuda, job, fast=True, seam=0, devices=None, shard=(0, 1)):
    hook = plugin.tilevae.VAEHook(_decoder(), 16, is_decoder=True, fast_decoder=fast, fast_encoder=False, color_fix=False)
    hook.seam_blend, hook.devices, hook.shard, hook.inpaint_job = seam, devices, shard, job
    with torch.no_grad():
        return hook(_latent(cuda)).clone(), hook


@functools.lru_cache(maxsize=None)
def _off():
    """The option-off image of the fast decoder, once."""
    return _run(sh.load_plugin(), torch.device("cuda:0"), None)[0]


def _outs(plugin):
    return [tuple(o) for o in plugin.engine.vae_split_tiles(64, 64, 16, True)[1]]


def _check_skip_image(plugin, on, off, job, active, fill_np):
    on_i, off_i = on.view(torch.int32), off.view(torch.int32)
    for i, (x1, x2, y1, y2) in enumerate(_outs(plugin)):
        if i in active:
            assert torch.equal(on_i[:, :, y1:y2, x1:x2], off_i[:, :, y1:y2, x1:x2]), f"tile {i}: the decoded bits differ from the full decode's"
        else:
            _same_bits(on[:, :, y1:y2, x1:x2], np.broadcast_to(fill_np[:, :, y1:y2, x1:x2], (1, 3, y2 - y1, x2 - x1)), f"tile {i}: the fill")


def test_hook_decodes_two_of_nine_tiles(plugin, cuda, capsys):
    off = _off()
    job = _job()
    capsys.readouterr()
    on, hook = _run(plugin, cuda, job)
    out = capsys.readouterr().out
    assert "[Tiled VAE]: decoding 2 of 9 tiles (inpaint mask)" in out and NOT_APPLIED not in out
    assert on.shape == off.shape == (1, 3, 512, 512)
    assert hook.last_tiles_run == 2 and hook.last_tile_slots == [0 if i in (CENTRE, CORNER) else -1 for i in range(9)]
    init = vr.fill_value(np.asarray(job.init_images[0])).transpose(2, 0, 1)[None]
    _check_skip_image(plugin, on, off, job, (CENTRE, CORNER), init)
    assert not torch.isnan(on).any()
    # the host's composite: the original wherever the overlay mask is zero
    m = torch.from_numpy(np.asarray(job.mask_for_overlay) > 0).to(cuda)
    init_t = torch.from_numpy(np.ascontiguousarray(init)).to(cuda)
    a, b = torch.where(m, on, init_t), torch.where(m, off, init_t)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert not torch.equal(on, off), "the option changed nothing"


def test_hook_on_two_slots_gives_the_same_bits(plugin, cuda):
    job = _job()
    one, _ = _run(plugin, cuda, job)
    many, hook = _run(plugin, cuda, job, devices=[0, 0])
    assert torch.equal(many.view(torch.int32), one.view(torch.int32))
    assert hook.last_tiles_run == 2 and sorted(hook.last_tile_slots) == [-1] * 7 + [0, 1]


@pytest.mark.parametrize("images", ["none", "two", "wrong_size"])
def test_hook_fills_with_zeros_without_a_usable_init_image(plugin, cuda, images):
    job = _job(init_images={"none": [], "two": [_init_image(), _init_image()], "wrong_size": [_init_image((256, 256))]}[images])
    on, hook = _run(plugin, cuda, job)
    _check_skip_image(plugin, on, _off(), job, (CENTRE, CORNER), np.zeros((1, 3, 512, 512), np.float32))


def test_hook_uses_the_bytes_the_upscale_left_on_the_device(plugin, cuda):
    job = _job()
    kept = torch.full((512, 512, 3), 51, dtype=torch.uint8, device=cuda)
    job.init_image_bytes_md = (job.init_images[0], kept)
    on, _ = _run(plugin, cuda, job)
    _check_skip_image(plugin, on, _off(), job, (CENTRE, CORNER), np.full((1, 3, 512, 512), vr.fill_value(51), np.float32))


REASONS = {
    "slow_decoder": (dict(fast=False), {}, "norm is frozen"),
    "seam_blend": (dict(seam=16), {}, "seam blend"),
    "process_per_gpu": (dict(shard=(0, 2)), {}, "sharded over processes"),
    "no_overlay_mask": ({}, dict(mask_for_overlay=None), "no overlay mask"),
    "no_overlay_images": ({}, dict(overlay_images=[]), "no overlay images"),
    "only_masked": ({}, dict(inpaint_full_res=True), "only masked"),
    "color_correction": ({}, dict(color_corrections=[object()]), "colour correction"),
    "wrap_x": (dict(wrap="mdtile_wrap_x"), {}, "wrap-around"),
    "mask_size": ({}, dict(mask_for_overlay=_mask_image((504, 512))), "overlay mask is 504 x 512 px"),
    "every_tile_active": ({}, dict(mask_for_overlay=_mask_image(value=9)), "all 9 tiles"),
    "no_tile_active": ({}, dict(mask_for_overlay=_mask_image(blob=False, pixel=False)), "no tile"),
}


@pytest.mark.parametrize("reason", list(REASONS))
def test_each_reason_gives_the_option_off_bits_and_one_line(plugin, cuda, capsys, monkeypatch, reason):
    setup, over, words = REASONS[reason]
    _, shared = sh.host()
    monkeypatch.setattr(plugin.tilevae, "SP_ESTIMATOR", False)      # (one rank of a two-process shard on its own: no estimator exchange)
    if "wrap" in setup:
        monkeypatch.setattr(shared.cmd_opts, setup["wrap"], True, raising=False)
    kw = {k: v for k, v in setup.items() if k != "wrap"}
    want = _off() if not setup else _run(plugin, cuda, None, **kw)[0]
    capsys.readouterr()
    got, hook = _run(plugin, cuda, _job(**over), **kw)
    lines = [l for l in capsys.readouterr().out.splitlines() if NOT_APPLIED in l]
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "not applied: the option-off bits"
    assert len(lines) == 1 and lines[0].startswith(f"[Tiled VAE]: {NOT_APPLIED} ") and words in lines[0], lines
