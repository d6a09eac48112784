"""Tiled VAE tile skipping for inpaint jobs, host side (no GPU): the --mdtile-vae-inpaint-skip option, the invariants of the
numpy restatement (tests/vae_skip_ref.py), the fill's round trip through a host's byte conversion, and the decoder hook's decision list on the
torch doubles of tests/torch_engine.py with the two new engine calls implemented by the restatement."""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import seam_cases as sc                  # noqa: E402
import seam_ref as sr                    # noqa: E402
import vae_skip_ref as vr                # noqa: E402
from wrap_common import load_preload     # noqa: E402

NEW_SYMBOLS = ["mdtile_mask_activity_u8", "mdtile_vae_assemble_sparse"]
NOT_APPLIED = "--mdtile-vae-inpaint-skip not applied:"


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- symbols and the option --------------------------------------------------------------------------------------------------------
def test_header_library_and_binding_have_the_new_symbols(built_lib):
    import ctypes
    import re
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mdtile.h")).read(), flags=re.S)
    lib = ctypes.CDLL(built_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), f"{name} is not declared in include/mdtile.h"
        assert hasattr(lib, name), f"libmdtile.so does not export {name}"
        assert name in built_lib.exported_symbols()
    assert built_lib.lib().mdtile_version() == 100
    assert callable(built_lib.mask_activity_u8) and callable(built_lib.vae_assemble_sparse)


def test_refusals_that_need_no_device(built_lib):
    """Argument checks that come before any device is touched name their reason."""
    L = built_lib.lib()
    assert L.mdtile_mask_activity_u8(None, 8, 8, None, 1, None, None) == built_lib.E_ARG and b"null" in L.mdtile_last_error()
    assert L.mdtile_vae_assemble_sparse(None, -1, None, 0, None, 1, 3, None, 8, 8, None) == built_lib.E_ARG and b"bad arguments" in L.mdtile_last_error()
    assert L.mdtile_vae_assemble_sparse(None, 4000, None, 97, None, 1, 3, None, 8, 8, None) == built_lib.E_ARG
    with pytest.raises(built_lib.MdtileError, match="no CPU fallback"):
        built_lib.mask_activity_u8(torch.zeros(8, 8, dtype=torch.uint8), [(0, 8, 0, 8)])
    with pytest.raises(built_lib.MdtileError, match="no CPU fallback"):
        built_lib.vae_assemble_sparse([], [(0, 8, 0, 8)], None, torch.zeros(1, 3, 8, 8))


def test_preload_option_and_its_reader(plugin):
    import modules.shared as shared
    parser = argparse.ArgumentParser()
    load_preload().preload(parser)
    assert parser.parse_args([]).mdtile_vae_inpaint_skip is False
    ns = parser.parse_args(["--mdtile-vae-inpaint-skip"])
    assert ns.mdtile_vae_inpaint_skip is True and ns.mdtile_inpaint_skip is False      # the Tiled Diffusion option is another one
    text = " ".join(parser.format_help().split())
    for word in ("overlay mask", "pasting the original image back", "soft inpainting", "Not applied", "seam-blend", "only masked", "colour correction"):
        assert word in text, word
    if hasattr(shared.cmd_opts, "mdtile_vae_inpaint_skip"):
        del shared.cmd_opts.mdtile_vae_inpaint_skip
    assert plugin.tilevae._cmd_line_vae_inpaint_skip() is False        # a host that never heard of the option
    shared.cmd_opts.mdtile_vae_inpaint_skip = True
    try:
        assert plugin.tilevae._cmd_line_vae_inpaint_skip() is True
    finally:
        del shared.cmd_opts.mdtile_vae_inpaint_skip


class _Net(torch.nn.Module):
    def forward(self, x):
        return x


@pytest.mark.parametrize("on", [False, True], ids=["off", "on"])
def test_process_hands_the_job_to_the_decoder_hook_only(plugin, monkeypatch, on):
    import modules.shared as shared
    enc, dec = _Net(), _Net()
    p = SimpleNamespace(sd_model=SimpleNamespace(first_stage_model=SimpleNamespace(encoder=enc, decoder=dec)), extra_generation_params={})
    if on:
        monkeypatch.setattr(shared.cmd_opts, "mdtile_vae_inpaint_skip", True, raising=False)
    s = plugin.tilevae.Script()
    s.process(p, True, 3072, 256, True, True, True, False)
    hd, he = dec.forward, enc.forward
    assert (hd.inpaint_job is p) == on and he.inpaint_job is None
    assert p.extra_generation_params == ({"Tiled VAE inpaint skip": True} if on else {})
    s.postprocess(p, None, True)
    assert hd.inpaint_job is None and he.inpaint_job is None, "postprocess drops the reference to the job"


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def test_activity_on_hand_made_masks():
    m = np.zeros((8, 12), dtype=np.uint8)
    boxes = [(0, 4, 0, 4), (4, 12, 0, 4), (0, 4, 4, 8), (4, 12, 4, 8)]
    assert vr.activity(m, boxes) == [0, 0, 0, 0]
    m[3, 3] = 1
    assert vr.activity(m, boxes) == [1, 0, 0, 0]
    m[3, 3], m[4, 3] = 0, 200
    assert vr.activity(m, boxes) == [0, 0, 1, 0]
    m[:] = 255
    assert vr.activity(m, boxes) == [1, 1, 1, 1]
    m[:] = 0
    m[0, 11] = 7
    assert vr.activity(m, boxes + [(11, 12, 0, 1), (10, 11, 0, 1)]) == [0, 1, 0, 0, 1, 0]
    for bad, why in (([], "n_boxes"), ([(0, 13, 0, 4)], "outside"), ([(0, 4, -1, 4)], "outside"), ([(4, 4, 0, 4)], "empty"),
                     ([(0, 1, 0, 1)] * (vr.MAX_BOXES + 1), "n_boxes")):
        with pytest.raises(ValueError, match=why):
            vr.activity(m, bad)


@pytest.mark.parametrize("case", [c for c in sc.LEGAL if sc.LEGAL[c][3]])
def test_assemble_sparse_with_every_tile_is_the_edge_to_edge_paste(case):
    xs, ys, margin, is_dec, band, (N, C) = sc.LEGAL[case]
    RH, RW = sc.result_size(sc.LEGAL[case])
    tab = sc.table(xs, ys, margin, True, N, C, seed=5, special_band=1)
    got = vr.assemble_sparse(tab, [], None, N, C, RH, RW)
    want = sr.assemble_plain(tab, RH, RW, True)
    assert np.array_equal(_bits(got), _bits(want))


def test_assemble_sparse_fills_what_is_missing_and_refuses_what_is_no_partition():
    xs, ys, margin, is_dec, band, _ = sc.LEGAL["3x3_b1"]
    RH, RW = sc.result_size(sc.LEGAL["3x3_b1"])
    N, C = 2, 3
    tab = sc.table(xs, ys, margin, True, N, C, seed=1)
    fill = np.random.RandomState(2).randint(0, 256, size=(RH, RW, C)).astype(np.uint8)
    present = [0, 4, 8]
    tiles = [tab[i] for i in present]
    boxes = [tab[i][2] for i in range(9) if i not in present]
    got = vr.assemble_sparse(tiles, boxes, fill, N, C, RH, RW)
    plain = sr.assemble_plain(tab, RH, RW, True)
    for i, (_, _, ob) in enumerate(tab):
        box = got[:, :, ob[2]:ob[3], ob[0]:ob[1]]
        if i in present:
            assert np.array_equal(_bits(box), _bits(plain[:, :, ob[2]:ob[3], ob[0]:ob[1]]))
        else:
            want = (fill[ob[2]:ob[3], ob[0]:ob[1]].astype(np.float32) / np.float32(127.5) - np.float32(1.0)).transpose(2, 0, 1)
            assert np.array_equal(_bits(box), _bits(np.broadcast_to(want, box.shape)))
    zero = vr.assemble_sparse(tiles, boxes, None, N, C, RH, RW)
    ob = tab[1][2]
    assert not _bits(zero[:, :, ob[2]:ob[3], ob[0]:ob[1]]).any(), "+0.0, not -0.0"
    for t, b, why in ((tiles, boxes[:-1], "area sum"), (tiles, boxes + [tab[0][2]], "also tile"), (tiles, boxes + [boxes[0]], "overlap"),
                      (tiles, boxes[:-1] + [(0, RW + 8, 0, 8)], "outside"), (tiles, boxes + [(8, 8, 0, 8)], "empty")):
        with pytest.raises(ValueError, match=why):
            vr.assemble_sparse(t, b, fill, N, C, RH, RW)


def test_fill_round_trip_of_all_256_bytes():
    """A host that rounds gets every byte back; the webui's truncating astype(uint8) gets some values one level low -- never more than one, never
    high -- which the overlay paste hides.  The count is written down as what it is."""
    b = np.arange(256, dtype=np.uint8)
    v = vr.fill_value(b)
    assert v.dtype == np.float32 and v[0] == -1.0 and v[255] == 1.0 and (np.diff(v) > 0).all()
    assert np.array_equal(vr.round_trip(v, truncate=False), b)
    t = vr.round_trip(v, truncate=True).astype(np.int32)
    low = b.astype(np.int32) - t
    assert set(low.tolist()) <= {0, 1}
    assert int(low.sum()) == TRUNCATION_LOW, int(low.sum())


TRUNCATION_LOW = 63      # of the 256 byte values, under (x + 1) / 2 * 255 in fp32 and astype(uint8)


# ---- the hook on the torch doubles --------------------------------------------------------------------------------------------------
H, W = 40, 56          # 2 x 3 tiles at tile 16: out boxes 216 / 128 / 104 px wide, 216 / 104 px tall


def _doubles():
    import torch_engine as te

    class SkipEngine(te.TorchEngineRec):
        """The record-path doubles, the assemblies by crop_store / the seam restatement, and the two new calls by tests/vae_skip_ref.py."""

        def __init__(self):
            self.activity_calls, self.sparse_calls, self.plain_calls = [], [], []

        def vae_assemble(self, tiles, result, is_decoder=True):
            self.plain_calls.append(len(tiles))
            for t, ib, ob in tiles:
                self.crop_store(t, ib, ob, result, is_decoder)

        def vae_assemble_blend(self, tiles, rows, cols, result, band, is_decoder=True):
            tab = [(t.numpy(), tuple(ib), tuple(ob)) for t, ib, ob in tiles]
            result.copy_(torch.from_numpy(sr.assemble_blend(tab, rows, cols, result.shape[2], result.shape[3], band, is_decoder)))

        def mask_activity_u8(self, mask, boxes):
            assert mask.dtype == torch.uint8 and mask.dim() == 2
            self.activity_calls.append([tuple(b) for b in boxes])
            return vr.activity(mask.numpy(), [tuple(b) for b in boxes])

        def vae_assemble_sparse(self, tiles, fill_boxes, fill, result):
            self.sparse_calls.append(SimpleNamespace(outs=[tuple(ob) for _, _, ob in tiles], fill_boxes=[tuple(b) for b in fill_boxes], fill=fill))
            tab = [(t.numpy(), tuple(ib), tuple(ob)) for t, ib, ob in tiles]
            N, C, RH, RW = result.shape
            result.copy_(torch.from_numpy(vr.assemble_sparse(tab, [tuple(b) for b in fill_boxes], None if fill is None else fill.numpy(), N, C, RH, RW)))

    return te, SkipEngine


def _hook(fast=True, is_decoder=True):
    from hostsim import stub_host as sh, ldm_decoder as ld
    te, SkipEngine = _doubles()
    sh.install("cpu")
    sh.set_device("cpu")
    pl = sh.load_plugin()
    net = ld.make_decoder(0, small=True) if is_decoder else ld.make_encoder(0, small=True)
    net.original_forward = net.forward
    hook = pl.tilevae.VAEHook(net, 16 if is_decoder else 64, is_decoder=is_decoder, fast_decoder=fast, fast_encoder=True, color_fix=False)
    hook.engine, hook._pack, hook._sp_ops = SkipEngine(), (te.TorchConvRec if is_decoder else te.TorchConv), te.TorchSeqParOps()
    return hook, pl


def _mask(size, dots):
    m = np.zeros((size[1], size[0]), dtype=np.uint8)
    for x, y in dots:
        m[y, x] = 255
    return Image.fromarray(m, mode="L")


def _init(size, seed=7):
    return Image.fromarray(np.random.RandomState(seed).randint(0, 256, size=(size[1], size[0], 3)).astype(np.uint8), mode="RGB")


class _Job(SimpleNamespace):
    """A processing object that records every attribute read."""

    def __init__(self, **kw):
        super().__init__(**kw)
        object.__setattr__(self, "reads", [])

    def __getattribute__(self, name):
        if not name.startswith("__") and name != "reads":
            object.__getattribute__(self, "reads").append(name)
        return super().__getattribute__(name)


def _job(size=(W * 8, H * 8), dots=((300, 100),), **over):
    """An inpaint job as the webui leaves it after p.init(): the mask touches tile 1 (x 216..344, y 0..216) unless `dots` says otherwise."""
    kw = dict(mask_for_overlay=_mask(size, dots), overlay_images=[object()], inpaint_full_res=False, color_corrections=None,
              init_images=[_init(size)])
    kw.update(over)
    return _Job(**kw)


@pytest.fixture(scope="module")
def z():
    torch.manual_seed(2)
    return torch.randn(1, 4, H, W)


def _lines(capsys):
    out = capsys.readouterr().out.splitlines()
    return [l for l in out if NOT_APPLIED in l], [l for l in out if "(inpaint mask)" in l]


def test_option_off_reads_nothing_and_prints_nothing(z, capsys):
    hook, _ = _hook()
    assert hook.inpaint_job is None
    with torch.no_grad():
        hook(z)
    E = hook.engine
    assert E.activity_calls == [] and E.sparse_calls == [] and hook.last_tiles_run == 6 and hook.last_tile_slots == [0] * 6
    out = capsys.readouterr().out
    assert "inpaint" not in out


def test_skip_decodes_the_touched_tiles_and_fills_the_rest(z, capsys):
    from oracle import vae_oracle as vo
    full_hook, _ = _hook()
    with torch.no_grad():
        full = full_hook(z)
    hook, _ = _hook()
    job = _job(dots=((300, 100), (447, 319)))          # tile 1 and the last pixel of tile 5
    hook.inpaint_job = job
    with torch.no_grad():
        got = hook(z)
    _, outs = vo.split_tiles(H, W, 16, True)
    E = hook.engine
    assert E.activity_calls == [[tuple(o) for o in outs]] and len(E.sparse_calls) == 1 and E.plain_calls == []
    call = E.sparse_calls[0]
    assert sorted(call.outs) == sorted(tuple(outs[i]) for i in (1, 5)) and call.fill_boxes == [tuple(outs[i]) for i in (0, 2, 3, 4)]
    assert hook.last_tiles_run == 2 and hook.last_tile_slots == [-1, 0, -1, -1, -1, 0]
    fill = vr.fill_value(np.asarray(job.init_images[0])).transpose(2, 0, 1)[None]
    # (the doubles' CPU convs pick their blocking by the stack's size: a tile decoded in another stack agrees to rounding only; bitwise on the GPU)
    tol = 1e-5 * full.abs().max().item()
    for i, ob in enumerate(outs):
        box = got[:, :, ob[2]:ob[3], ob[0]:ob[1]]
        if i in (1, 5):
            assert (box - full[:, :, ob[2]:ob[3], ob[0]:ob[1]]).abs().max().item() <= tol
        else:
            assert np.array_equal(_bits(box.numpy()), _bits(fill[:, :, ob[2]:ob[3], ob[0]:ob[1]]))
    not_applied, decoding = _lines(capsys)
    assert not_applied == [] and decoding == ["[Tiled VAE]: decoding 2 of 6 tiles (inpaint mask)"]


def test_fill_is_zero_without_a_usable_init_image_and_reuses_kept_bytes(z):
    size = (W * 8, H * 8)
    for images in ([], [_init(size), _init(size)], [_init((64, 64))], None):
        hook, _ = _hook()
        hook.inpaint_job = _job(init_images=images)
        with torch.no_grad():
            hook(z)
        assert hook.engine.sparse_calls[0].fill is None, images
    hook, _ = _hook()
    grey = Image.fromarray(np.random.RandomState(1).randint(0, 256, size=(size[1], size[0])).astype(np.uint8), mode="L")
    hook.inpaint_job = _job(init_images=[grey])
    with torch.no_grad():
        hook(z)
    f = hook.engine.sparse_calls[0].fill
    assert tuple(f.shape) == (size[1], size[0], 3) and np.array_equal(f.numpy(), np.asarray(grey.convert("RGB")))
    hook, _ = _hook()
    job = _job()
    kept = torch.full((size[1], size[0], 3), 9, dtype=torch.uint8)
    job.init_image_bytes_md = (job.init_images[0], kept)
    hook.inpaint_job = job
    with torch.no_grad():
        hook(z)
    assert torch.equal(hook.engine.sparse_calls[0].fill, kept), "the bytes the upscale left on the device are used, not uploaded again"
    job.init_image_bytes_md = (_init(size, seed=8), kept)          # another image's bytes
    hook, _ = _hook()
    hook.inpaint_job = job
    with torch.no_grad():
        hook(z)
    assert np.array_equal(hook.engine.sparse_calls[0].fill.numpy(), np.asarray(job.init_images[0]))


REASONS = {
    "slow_decoder": (dict(fast=False), {}, "norm is frozen"),
    "seam_blend": (dict(seam=16), {}, "seam blend"),
    "process_per_gpu": (dict(shard=(0, 2)), {}, "sharded over processes"),
    "no_overlay_mask": ({}, dict(mask_for_overlay=None), "no overlay mask"),
    "no_overlay_images": ({}, dict(overlay_images=[]), "no overlay images"),
    "only_masked": ({}, dict(inpaint_full_res=True), "only masked"),
    "color_correction": ({}, dict(color_corrections=[object()]), "colour correction"),
    "wrap_x": (dict(wrap="mdtile_wrap_x"), {}, "wrap-around"),
    "wrap_y": (dict(wrap="mdtile_wrap_y"), {}, "wrap-around"),
    "mask_size": ({}, dict(mask_for_overlay=_mask((W * 8 - 8, H * 8), ((300, 100),))), "overlay mask is 440 x 320 px"),
    "every_tile_active": ({}, dict(mask_for_overlay=Image.new("L", (W * 8, H * 8), 255)), "all 6 tiles"),
    "no_tile_active": ({}, dict(mask_for_overlay=Image.new("L", (W * 8, H * 8), 0)), "no tile"),
}


@pytest.mark.parametrize("reason", list(REASONS))
def test_each_reason_runs_the_full_decode_and_says_so_once(z, capsys, monkeypatch, reason):
    import modules.shared as shared
    setup, over, words = REASONS[reason]

    def run(with_job):
        hook, pl = _hook(fast=setup.get("fast", True))
        monkeypatch.setattr(pl.tilevae, "SP_ESTIMATOR", False)      # (a rank of a two-process shard on its own: no estimator exchange)
        hook.seam_blend = setup.get("seam", 0)
        hook.shard = setup.get("shard", (0, 1))
        if with_job:
            hook.inpaint_job = _job(**over)
        with torch.no_grad():
            return hook, hook(z), hook(z)          # two decodes of one job: one line

    if "wrap" in setup:
        monkeypatch.setattr(shared.cmd_opts, setup["wrap"], True, raising=False)
    _, want, _ = run(False)
    capsys.readouterr()
    hook, got, again = run(True)
    assert torch.equal(got, want) and torch.equal(again, want), "not applied: the option-off image"
    assert hook.engine.sparse_calls == []
    assert hook.last_tiles_run == (3 if "shard" in setup else len(hook.last_tile_slots or [0] * 6))
    not_applied, decoding = _lines(capsys)
    assert len(not_applied) == 1 and decoding == [], not_applied
    assert not_applied[0].startswith(f"[Tiled VAE]: {NOT_APPLIED} ") and words in not_applied[0], not_applied[0]
    # the list is walked in order: a reason in front of the mask never reads the mask's pixels, one in front of the job never reads the job
    if reason in ("slow_decoder", "seam_blend", "process_per_gpu"):
        assert hook.inpaint_job.reads == []
    if reason not in ("every_tile_active", "no_tile_active"):
        assert hook.engine.activity_calls == []


def test_the_encoder_hook_is_refused_by_name(capsys):
    hook, _ = _hook(is_decoder=False)
    hook.inpaint_job = _job()
    torch.manual_seed(4)
    x = torch.randn(1, 3, 136, 200)
    with torch.no_grad():
        got = hook(x)
    plain, _ = _hook(is_decoder=False)
    with torch.no_grad():
        want = plain(x)
    assert torch.equal(got, want) and hook.inpaint_job.reads == []
    not_applied, decoding = _lines(capsys)
    assert len(not_applied) == 1 and "encoder" in not_applied[0] and decoding == []


def test_refusal_order_is_the_documented_one(plugin):
    """inpaint_skip_refusal names the FIRST reason of the list that fails."""
    f = plugin.tilevae.inpaint_skip_refusal
    size = (64, 64)
    bad = _Job(mask_for_overlay=None, overlay_images=[], inpaint_full_res=True, color_corrections=[1])
    order = [(dict(is_decoder=False), "encoder"), (dict(all_frozen=False), "frozen"), (dict(seam_set=True), "seam blend"), (dict(world=2), "sharded")]
    base = dict(is_decoder=False, all_frozen=False, seam_set=True, world=2, wrap=True, size=size)
    for k, (fix, word) in enumerate(order):
        why, mask = f(bad, **base)
        assert word in why and mask is None, (k, why)
        base.update({key: (not v if isinstance(v, bool) else 1) for key, v in fix.items()})
    for attr, value, word in (("mask_for_overlay", _mask((48, 64), ()), "no overlay mask"), ("overlay_images", [1], "no overlay images"),
                              ("inpaint_full_res", False, "only masked"), ("color_corrections", [], "colour correction")):
        why, mask = f(bad, **base)
        assert word in why and mask is None, why
        setattr(bad, attr, value)
    assert "wrap-around" in f(bad, **base)[0]
    base["wrap"] = False
    assert "48 x 64 px" in f(bad, **base)[0]
    bad.mask_for_overlay = _mask(size, ()).convert("RGB")
    why, mask = f(bad, **base)
    assert why is None and mask.mode == "L" and mask.size == size
    # a host object without any of the attributes: not an inpaint job
    assert "no overlay mask" in f(SimpleNamespace(), **base)[0]


def test_interrupt_pastes_what_finished_and_fills_the_rest(z, monkeypatch):
    import modules.shared as shared
    hook, pl = _hook()
    monkeypatch.setattr(pl.tilevae, "TILE_BATCH", 1)
    hook.inpaint_job = _job(dots=((300, 100), (100, 300), (400, 300)))       # tiles 1, 3, 5
    finish = pl.tilevae.VAEHook._Lane.finish
    done = []

    def finish_then_interrupt(self, i):
        finish(self, i)
        done.append(i)
        shared.state.interrupted = True

    monkeypatch.setattr(pl.tilevae.VAEHook._Lane, "finish", finish_then_interrupt)
    try:
        with torch.no_grad():
            hook(z)
    finally:
        shared.state.interrupted = False
    from oracle import vae_oracle as vo
    _, outs = vo.split_tiles(H, W, 16, True)
    call = hook.engine.sparse_calls[0]
    assert len(done) == 1 and hook.last_tiles_run == 3
    assert call.outs == [tuple(outs[done[0]])] and call.fill_boxes == [tuple(o) for i, o in enumerate(outs) if i != done[0]]
