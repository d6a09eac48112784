"""MDTILE_PRECISION_F16 (= 5) on the host side, no GPU needed: the C ABI accepts and reports the mode and still rejects the unknown ones, the
route predicates answer as in the default mode, the record-format tags are checked by the ABI before anything is launched, tools/asm_guard.py
--f16 finds every fp16 kernel next to its bf16 twin, --mdtile-precision is parsed and Script.process / postprocess set and restore the mode
(and never touch it when the option is absent), and tools/precision_model.py reproduces the ordering the mode was designed on."""
import argparse
import ctypes
import importlib.util
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

PKG = os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd")


def test_mode_5_is_accepted_reported_and_nests(built_lib):
    E = built_lib
    assert E.PRECISION_F16 == 5
    assert E.get_precision() == E.PRECISION_BF16X3
    try:
        E.set_precision(E.PRECISION_F16)
        assert E.get_precision() == 5 and E.lib().mdtile_get_precision() == 5
    finally:
        E.set_precision(E.PRECISION_BF16X3)
    with E.precision(E.PRECISION_F16):
        assert E.get_precision() == E.PRECISION_F16
        with E.precision(E.PRECISION_BF16):
            assert E.get_precision() == E.PRECISION_BF16
            with E.precision(E.PRECISION_F16):
                assert E.get_precision() == E.PRECISION_F16
            assert E.get_precision() == E.PRECISION_BF16
        assert E.get_precision() == E.PRECISION_F16
    assert E.get_precision() == E.PRECISION_BF16X3
    with pytest.raises(KeyError):
        with E.precision(E.PRECISION_F16):
            raise KeyError("boom")
    assert E.get_precision() == E.PRECISION_BF16X3


@pytest.mark.parametrize("mode", [3, 4, 7, -1, 6])
def test_the_other_values_are_still_rejected(built_lib, mode):
    E = built_lib
    with E.precision(E.PRECISION_F16):
        with pytest.raises(E.MdtileError):
            E.set_precision(mode)
        assert E.get_precision() == E.PRECISION_F16      # a rejected value leaves the mode in force
        assert f"unknown mode {mode}" in E.lib().mdtile_last_error().decode()
    assert E.get_precision() == E.PRECISION_BF16X3


def test_route_predicates_answer_for_mode_5_as_for_the_default(built_lib):
    E = built_lib
    L = E.lib()
    shapes = [(128, 128, 3, 0), (512, 512, 3, 0), (256, 512, 3, 1), (128, 3, 3, 0), (3, 128, 3, 0), (64, 64, 3, 0), (128, 128, 1, 0)]

    def routes():
        return ([E.v_channel_major_ok(C) for C in (128, 256, 512, 64)],
                [L.mdtile_conv2d_rec_supported(co, ci, k, up) for co, ci, k, up in shapes],
                [L.mdtile_conv2d_gn_supported(co, ci, k, up, 0) for co, ci, k, up in shapes],
                [L.mdtile_conv2d_rec_stats_supported(co, ci, k, up, 32) for co, ci, k, up in shapes],
                [L.mdtile_conv2d_gn_stats_supported(co, ci, k, up, 32) for co, ci, k, up in shapes])

    base = routes()
    assert any(base[0]) and any(base[1]) and any(base[2])
    with E.precision(E.PRECISION_F16):
        assert routes() == base


def test_fp16_weight_plane_has_the_size_of_the_direct_records(built_lib):
    """The plane is the hi-plane layout of the split image's direct 3x3 records: 16 bytes per (8 cin, cout, tap) of both halves of each chunk."""
    L = built_lib.lib()
    assert L.mdtile_conv_pack_f16_size(128, 128, 3) == (128 // 16) * 3 * 2 * 3 * 4 * 64 * 4
    assert L.mdtile_conv_pack_f16_size(512, 256, 3) == 4 * (256 // 16) * 3 * 2 * 3 * 4 * 64 * 4
    assert L.mdtile_conv_pack_f16_size(3, 128, 3) == (128 // 16) * 3 * 2 * 3 * 1 * 64 * 4      # conv_out: one 32-cout tile
    assert L.mdtile_conv_pack_f16_size(128, 128, 1) == 0 and L.mdtile_conv_pack_f16_size(128, 3, 3) == 0
    # the packed buffer of every mode is what it was
    assert L.mdtile_conv_packed_size(128, 128, 3) == 9 * 128 * 128 + ((128 // 16) * 3 * 2 * 3 * 4 * 64 + 2 * (128 // 16) * 16 * 4 * 64) * 4


def test_the_abi_rejects_a_format_tag_that_disagrees_with_the_mode(built_lib):
    """Checked before any launch (no device is touched): the pointers below are never dereferenced."""
    E = built_lib
    L = E.lib()
    p = 4096      # any non-null "pointer"

    def err():
        return L.mdtile_last_error().decode()

    # default mode: no fp16 form can be written or read by a conv
    assert L.mdtile_rec_from_f32_fmt(p, p, p, 1, 32, 8, 8, E.REC_F16, None) == -1 and "record format mismatch" in err()
    assert L.mdtile_conv2d_rec(p, p, None, None, p, None, None, 1, 128, 128, 8, 8, E.CONV_REC_X_F16, None) == -1 and "record format mismatch" in err()
    assert L.mdtile_conv2d_rec(p, p, None, None, None, p, p, 1, 128, 128, 8, 8, E.CONV_REC_Y_F16, None) == -1 and "record format mismatch" in err()
    assert L.mdtile_conv2d_gn(p, p, p, None, None, p, 1, 128, 128, 8, 8, 3, E.CONV_W_F16, None) == -1 and "MDTILE_CONV_W_F16" in err()
    assert L.mdtile_rec_from_f32_fmt(p, p, p, 1, 32, 8, 8, 2, None) == -1 and "unknown record format" in err()
    with E.precision(E.PRECISION_BF16):
        assert L.mdtile_conv2d_rec(p, p, None, None, p, None, None, 1, 128, 128, 8, 8, E.CONV_REC_X_F16, None) == -1 and "record format mismatch" in err()
    with E.precision(E.PRECISION_F16):
        # a raw record is a bf16 split in every mode; an activated record output must be declared fp16; the upsample conv reads no fp16 record
        assert L.mdtile_rec_from_f32_fmt(p, None, p, 1, 32, 8, 8, E.REC_F16, None) == -1 and "record format mismatch" in err()
        assert L.mdtile_conv2d_rec(p, p, None, None, None, p, p, 1, 128, 128, 8, 8, 0, None) == -1 and "record format mismatch" in err()
        assert L.mdtile_conv2d_rec(p, p, None, None, None, p, None, 1, 128, 128, 8, 8, E.CONV_REC_Y_F16, None) == -1 and "record format mismatch" in err()
        assert L.mdtile_conv2d_rec(p, p, None, None, p, None, None, 1, 128, 128, 8, 8, E.CONV_UPSAMPLE2X | E.CONV_REC_X_F16, None) == -1
        assert "record format mismatch" in err()
        y0 = (ctypes.c_int * 1)(0)
        assert L.mdtile_upconv2d_rec_window(p, p, None, None, p, p, 1, 128, 128, 8, 8, y0, y0, 4, 4, 0, None) == -1 and "record format mismatch" in err()


def test_the_abi_rejects_the_fp16_plane_together_with_exact_f32(built_lib):
    """MDTILE_CONV_W_F16 asks for one fp16 MFMA per product, MDTILE_CONV_EXACT_F32 for the fp32 kernel: the hand-over calls name the
    contradiction in every mode instead of picking one (checked before any launch; the pointers are never dereferenced)."""
    E = built_lib
    L = E.lib()
    p = 4096
    both = E.CONV_W_F16 | E.CONV_EXACT_F32
    for mode in (E.PRECISION_BF16X3, E.PRECISION_F16):
        with E.precision(mode):
            assert L.mdtile_conv2d_gn(p, p, p, None, None, p, 1, 128, 128, 8, 8, 3, both, None) == -1
            assert "contradicts MDTILE_CONV_EXACT_F32" in L.mdtile_last_error().decode()
            assert L.mdtile_conv2d_gn_stats(p, p, p, None, None, p, 1, 128, 128, 8, 8, 3, both, 32, p, p, p, None) == -1
            assert "contradicts MDTILE_CONV_EXACT_F32" in L.mdtile_last_error().decode()
            # the predicates are what they were: EXACT_F32 has no fused pre-activation kernel, with or without the fp16 flag
            assert L.mdtile_conv2d_gn_supported(128, 128, 3, both, 0) == 0 == L.mdtile_conv2d_gn_supported(128, 128, 3, E.CONV_EXACT_F32, 0)


def _guard(*flags):
    return subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asm_guard.py"), *flags], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_asm_guard_checks_the_fp16_kernels(built_lib):
    r = _guard("--f16")
    assert r.returncode == 0, r.stdout
    lines = [l for l in r.stdout.splitlines() if l.rstrip().endswith(" ok")]
    for k in ("k_conv3x3_rec_f16ILi2ELi2ELi4", "k_conv3x3_rec_f16sILi2ELi2ELi4", "k_conv3x3_rec_f16sILi1ELi1ELi2", "k_conv3x3_rec_f16_stILi2ELi2ELi4",
              "k_conv3x3_rec2_f16ILi2ELi2ELi4", "k_conv3x3_rec2_f16sILi2ELi2ELi4", "k_upconv_rec_o16E", "k_upconv_rec2_o16E", "k_rec_from_f32_f16E",
              "k_conv3x3_f16ILi4ELb1ELi1ELb0", "k_conv3x3_f16ILi4ELb1ELi1ELb1", "k_conv3x3_f16ILi2ELb1ELi1ELb0"):
        assert sum(1 for l in lines if k in l) == 1, (k, r.stdout)
    assert len(lines) == 14 + 12


def test_asm_guard_alone_is_what_it_was(built_lib):
    r = _guard()
    assert r.returncode == 0, r.stdout
    assert sum(1 for l in r.stdout.splitlines() if l.rstrip().endswith(" ok")) == 14
    assert "rec_f16" not in r.stdout and "_o16" not in r.stdout and "k_conv3x3_f16" not in r.stdout


def test_preload_registers_the_precision_option():
    spec = importlib.util.spec_from_file_location("mdtile_preload_f16", os.path.join(PKG, "preload.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = argparse.ArgumentParser()
    mod.preload(parser)
    assert parser.parse_args([]).mdtile_precision is None
    for v in ("bf16x3", "f32", "bf16", "f16", "auto"):
        assert parser.parse_args(["--mdtile-precision", v]).mdtile_precision == v
    with pytest.raises(SystemExit):
        parser.parse_args(["--mdtile-precision", "fp8"])


def test_resolve_precision(plugin, capsys):
    tv, E = plugin.tilevae, plugin.engine
    assert tv.resolve_precision(None, torch.float16) is None and tv.resolve_precision("", torch.float16) is None
    assert tv.resolve_precision("f16", torch.float32) == E.PRECISION_F16
    assert tv.resolve_precision("BF16", None) == E.PRECISION_BF16
    assert tv.resolve_precision("f32", None) == E.PRECISION_F32 and tv.resolve_precision("bf16x3", None) == E.PRECISION_BF16X3
    assert tv.resolve_precision("auto", torch.float16) == E.PRECISION_F16
    assert tv.resolve_precision("auto", torch.bfloat16) == E.PRECISION_BF16
    assert tv.resolve_precision("auto", torch.float32) == E.PRECISION_BF16X3 and tv.resolve_precision("auto", None) == E.PRECISION_BF16X3
    assert tv.resolve_precision("fp8", torch.float16) is None
    assert "ignored" in capsys.readouterr().out


class _Net(torch.nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(4, dtype=dtype), requires_grad=False)

    def forward(self, x):
        return x


def _job(dtype=torch.float32):
    return SimpleNamespace(sd_model=SimpleNamespace(first_stage_model=SimpleNamespace(encoder=_Net(dtype), decoder=_Net(dtype))))


ARGS = (True, 3072, 256, False, True, True, False)


@pytest.mark.parametrize("value,dtype,want", [("bf16x3", torch.float32, 0), ("f32", torch.float32, 1), ("bf16", torch.float32, 2), ("f16", torch.float32, 5),
                                              ("auto", torch.float16, 5), ("auto", torch.bfloat16, 2), ("auto", torch.float32, 0)])
def test_process_sets_the_mode_and_postprocess_restores_it(plugin, monkeypatch, capsys, value, dtype, want):
    import modules.shared as shared
    tv, E = plugin.tilevae, plugin.engine
    monkeypatch.setattr(shared.cmd_opts, "mdtile_precision", value, raising=False)
    p, s = _job(dtype), tv.Script()
    assert E.get_precision() == E.PRECISION_BF16X3
    try:
        with E.precision(E.PRECISION_BF16):          # whatever the process runs in is what comes back
            s.process(p, *ARGS)
            assert E.get_precision() == want
            out = capsys.readouterr().out
            assert sum(1 for l in out.splitlines() if l.startswith("[Tiled VAE]") and "--mdtile-precision" in l) == 1
            s.process(p, *ARGS)                       # a job that never reached postprocess: the mode before IT is kept
            assert E.get_precision() == want
            s.postprocess(p, None, True)
            assert E.get_precision() == E.PRECISION_BF16
            s.postprocess(p, None, True)              # nothing left to restore
            assert E.get_precision() == E.PRECISION_BF16
    finally:
        E.set_precision(E.PRECISION_BF16X3)


def test_disabling_the_script_restores_the_mode(plugin, monkeypatch):
    import modules.shared as shared
    tv, E = plugin.tilevae, plugin.engine
    monkeypatch.setattr(shared.cmd_opts, "mdtile_precision", "f16", raising=False)
    p, s = _job(), tv.Script()
    try:
        s.process(p, *ARGS)
        assert E.get_precision() == E.PRECISION_F16
        s.process(p, False, *ARGS[1:])
        assert E.get_precision() == E.PRECISION_BF16X3
    finally:
        s.postprocess(p, None, True)
        E.set_precision(E.PRECISION_BF16X3)


def test_without_the_option_the_mode_is_never_touched(plugin, monkeypatch, capsys):
    import modules.shared as shared
    tv, E = plugin.tilevae, plugin.engine
    monkeypatch.setattr(shared.cmd_opts, "mdtile_precision", None, raising=False)
    calls = []
    monkeypatch.setattr(E, "set_precision", lambda m: calls.append(m))
    p, s = _job(torch.float16), tv.Script()
    s.process(p, *ARGS)
    s.postprocess(p, None, True)
    s.process(p, False, *ARGS[1:])
    assert calls == []
    assert "--mdtile-precision" not in capsys.readouterr().out
    monkeypatch.delattr(shared.cmd_opts, "mdtile_precision")      # a host that never heard of the option
    s.process(p, *ARGS)
    s.postprocess(p, None, True)
    assert calls == []


def test_precision_model_puts_scheme_a_below_mode_2():
    """tools/precision_model.py on its full-width nets (mode 2 and scheme A only): scheme A is below mode 2 on all four, by the factor the end-to-end
    gate of tests/test_gpu_precision_f16.py asks on the GPU (2; the model gives 4 and more)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "precision_model.py"), "--schemes", "mode2,A"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stderr
    rows = [l for l in r.stdout.splitlines() if l.startswith("| ") and "e-" in l]
    assert len(rows) == 2, r.stdout
    m2, a = ([float(c) for c in row.strip().strip("|").split("|")[1:]] for row in rows)
    assert len(m2) == len(a) == 4
    print(r.stdout)
    for e2, ea in zip(m2, a):
        assert ea < e2 / 2, (m2, a)
