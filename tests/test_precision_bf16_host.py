"""MDTILE_PRECISION_BF16 (one bf16 MFMA per product) on the host side, no GPU needed: the C ABI accepts mode 2 and reports it, rejects
unknown modes, mdtile.precision() restores the previous mode (also on an exception), the route predicates answer for mode 2 as for the
default, and tools/asm_guard.py finds the one-term kernels in the device assembly with their three-term twins' DMA protocol."""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT


def test_mode_2_is_accepted_and_reported(built_lib):
    E = built_lib
    assert E.PRECISION_BF16 == 2
    assert E.get_precision() == E.PRECISION_BF16X3
    try:
        E.set_precision(E.PRECISION_BF16)
        assert E.get_precision() == E.PRECISION_BF16
        E.set_precision(E.PRECISION_F32)
        assert E.get_precision() == E.PRECISION_F32
        E.set_precision(E.PRECISION_BF16)
        assert E.get_precision() == E.PRECISION_BF16
    finally:
        E.set_precision(E.PRECISION_BF16X3)
    assert E.get_precision() == E.PRECISION_BF16X3


@pytest.mark.parametrize("mode", [3, -1, 4, 7])
def test_unknown_modes_are_still_rejected(built_lib, mode):
    E = built_lib
    with pytest.raises(E.MdtileError):
        E.set_precision(mode)
    assert E.get_precision() == E.PRECISION_BF16X3
    assert f"unknown mode {mode}" in E.lib().mdtile_last_error().decode()


def test_precision_context_restores_the_previous_mode(built_lib):
    E = built_lib
    with E.precision(E.PRECISION_BF16):
        assert E.get_precision() == E.PRECISION_BF16
        with E.precision(E.PRECISION_F32):
            assert E.get_precision() == E.PRECISION_F32
        assert E.get_precision() == E.PRECISION_BF16
        with E.precision(E.PRECISION_BF16):          # the mode already in force: nothing changes
            assert E.get_precision() == E.PRECISION_BF16
        assert E.get_precision() == E.PRECISION_BF16
    assert E.get_precision() == E.PRECISION_BF16X3


def test_precision_context_restores_on_an_exception(built_lib):
    E = built_lib
    with pytest.raises(KeyError):
        with E.precision(E.PRECISION_BF16):
            assert E.get_precision() == E.PRECISION_BF16
            raise KeyError("boom")
    assert E.get_precision() == E.PRECISION_BF16X3
    with pytest.raises(E.MdtileError):
        with E.precision(3):                          # rejected before the block runs; the mode is untouched
            pass
    assert E.get_precision() == E.PRECISION_BF16X3


def test_route_predicates_answer_for_mode_2_as_for_the_default(built_lib):
    """The host picks the v layout of the attention and the conv routes from the library's predicates: mode 2 runs the same routes as
    BF16X3 (its kernels are the one-term forms of the same kernels), strict fp32 does not."""
    E = built_lib
    L = E.lib()
    shapes = [(128, 128, 3, 0), (512, 512, 3, 0), (256, 512, 3, 1), (128, 3, 3, 0)]

    def routes():
        return ([E.v_channel_major_ok(C) for C in (128, 256, 512, 64)],
                [L.mdtile_conv2d_rec_supported(co, ci, k, 0) for co, ci, k, _ in shapes],
                [L.mdtile_conv2d_gn_supported(co, ci, k, up, 0) for co, ci, k, up in shapes])

    base = routes()
    with E.precision(E.PRECISION_BF16):
        assert routes() == base
    with E.precision(E.PRECISION_F32):
        assert not any(routes()[0])


def test_env_presets_keep_their_meaning(tmp_path):
    """MDTILE_CONV_MODE=f32 / MDTILE_ATTN_MODE=f32 preset the strict bits at load time exactly as before (both: PRECISION_F32; one of them:
    reported as BF16X3); selecting mode 2 afterwards clears them."""
    code = ("import sys; sys.path.insert(0, sys.argv[1]); import mdtile as E; "
            "a = E.get_precision(); ch = E.v_channel_major_ok(512); E.set_precision(2); b = E.get_precision(); "
            "print(a, int(ch), b, int(E.v_channel_major_ok(512)))")
    pkg = os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd")
    want = {("f32", "f32"): "1 0 2 1", ("f32", ""): "0 1 2 1", ("", "f32"): "0 0 2 1", ("", ""): "0 1 2 1"}
    for (conv, attn), expect in want.items():
        env = {k: v for k, v in os.environ.items() if k not in ("MDTILE_CONV_MODE", "MDTILE_ATTN_MODE")}
        if conv:
            env["MDTILE_CONV_MODE"] = conv
        if attn:
            env["MDTILE_ATTN_MODE"] = attn
        r = subprocess.run([sys.executable, "-c", code, pkg], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert r.stdout.split("\n")[-2].strip() == expect, ((conv, attn), r.stdout)


def test_asm_guard_checks_the_one_term_kernels(built_lib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asm_guard.py"), "--one-term"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    rows = {}
    for line in r.stdout.splitlines():
        m = re.match(r"^(_Z\S+)\s+\d+ instr\s+(\d+) DMA\s+\d+ barriers \(vmcnt in front: (\[[^\]]*\]), lgkm-only: \d+\)\s+(\d+) MFMA\s+ok$", line)
        if m:
            rows[m.group(1)] = (int(m.group(2)), m.group(3), int(m.group(4)))
    twins = {"k_conv3x3_rec1tILi2ELi2ELi4": "k_conv3x3_recILi2ELi2ELi4", "k_conv3x3_rec1tILi1ELi1ELi2": "k_conv3x3_recILi1ELi1ELi2",
             "k_upconv_rec1tE": "k_upconv_recE", "k_conv3x3_rec1t_stILi2": "k_conv3x3_rec_stILi2", "k_upconv_rec1t_stE": "k_upconv_rec_stE",
             "k_conv3x3_rec2_1tILi2": "k_conv3x3_rec2ILi2", "k_upconv_rec2_1tE": "k_upconv_rec2E",
             "k_conv1x1_stream1tILi2": "k_conv1x1_streamILi2", "k_conv1x1_stream1tILi4": "k_conv1x1_streamILi4",
             "k_attn_bf16x1ILi512": "k_attn_bf16x3ILi512", "k_attn_bf16x1ILi256": "k_attn_bf16x3ILi256", "k_attn_bf16x1ILi128": "k_attn_bf16x3ILi128"}

    def row(sub):
        hit = [v for k, v in rows.items() if sub in k]
        assert len(hit) == 1, (sub, r.stdout)
        return hit[0]

    for one, three in twins.items():
        d1, w1, m1 = row(one)
        d3, w3, m3 = row(three)
        assert (d1, w1) == (d3, w3), f"{one}: DMA / barrier waits {d1} {w1} differ from {three}'s {d3} {w3}"
        assert 3 * m1 == m3, f"{one}: {m1} MFMAs, its three-term twin {m3}"
