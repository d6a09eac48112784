"""Tiled VAE on several devices of one process, host side (no GPU): the --mdtile-devices parser, the preload hook that registers it, the
slot list a hook derives from VAEHook.devices, and Script.process arming both hooks."""
import argparse
import importlib.util
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT


def _peers(*missing):
    return lambda dev, peer: (dev, peer) not in missing


def test_parse_keeps_order_and_expands_all(plugin):
    parse = plugin.tilevae.parse_devices
    assert parse("0,1,3", 0, 4, _peers()) == [0, 1, 3]
    assert parse(" 0, 1 ,3 ", 0, 4, _peers()) == [0, 1, 3]
    assert parse("all", 0, 4, _peers()) == [0, 1, 2, 3]
    assert parse("all", 2, 4, _peers()) == [2, 0, 1, 3]


def test_parse_puts_the_vae_device_first(plugin):
    parse = plugin.tilevae.parse_devices
    assert parse("1,2", 0, 4, _peers()) == [0, 1, 2]
    assert parse("1", 0, 4, _peers()) == [0, 1]
    assert parse("3,1,2", 1, 4, _peers()) == [1, 3, 2]


def test_parse_keeps_repeats(plugin):
    parse = plugin.tilevae.parse_devices
    assert parse("0,0", 0, 1, _peers()) == [0, 0]
    assert parse("0,0,0,1,1", 0, 2, _peers()) == [0, 0, 0, 1, 1]


def test_parse_out_of_range_voids_the_option(plugin, capsys):
    parse = plugin.tilevae.parse_devices
    assert parse("0,4", 0, 4, _peers()) is None
    assert "no CUDA device 4" in capsys.readouterr().out
    assert parse("0,x", 0, 4, _peers()) is None
    assert "ignored" in capsys.readouterr().out


def test_parse_drops_devices_without_peer_access(plugin, capsys):
    parse = plugin.tilevae.parse_devices
    assert parse("0,1,2", 0, 4, _peers((0, 2))) == [0, 1]
    assert "cuda:2" in capsys.readouterr().out
    assert parse("0,2,2", 0, 4, _peers((0, 2))) is None          # one slot left


def test_parse_single_slot_or_unset_is_none(plugin):
    parse = plugin.tilevae.parse_devices
    assert parse("0", 0, 4, _peers()) is None
    assert parse(None, 0, 4, _peers()) is None
    assert parse("", 0, 4, _peers()) is None


def test_preload_registers_the_option():
    spec = importlib.util.spec_from_file_location("mdtile_preload", os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd", "preload.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    parser = argparse.ArgumentParser()
    mod.preload(parser)
    assert parser.parse_args(["--mdtile-devices", "0,1"]).mdtile_devices == "0,1"
    assert parser.parse_args([]).mdtile_devices is None


def test_hook_slots_put_the_vae_device_first(plugin):
    hook = plugin.tilevae.VAEHook(None, 64, is_decoder=True, fast_decoder=True, fast_encoder=True, color_fix=False)
    assert hook._slots("cuda:0") is None
    hook.devices = [1, 2]
    assert hook._slots("cuda:0") == [0, 1, 2]
    hook.devices = [2, 0, 1]
    assert hook._slots("cuda:0") == [0, 2, 1]
    hook.devices = [0, 0]
    assert hook._slots("cuda:0") == [0, 0]
    hook.devices = [0]
    assert hook._slots("cuda:0") is None
    hook.devices = [0, 1]
    assert hook._slots("cpu") is None


def test_process_arms_both_hooks_from_the_command_line(plugin, monkeypatch):
    import modules.devices as host_devices
    import modules.shared as shared
    tv = plugin.tilevae

    class Net(torch.nn.Module):
        def forward(self, x):
            return x

    enc, dec = Net(), Net()
    p = SimpleNamespace(sd_model=SimpleNamespace(first_stage_model=SimpleNamespace(encoder=enc, decoder=dec)))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "device_count", lambda: 2)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    monkeypatch.setattr(torch.cuda, "can_device_access_peer", lambda a, b: True)
    monkeypatch.setattr(host_devices, "get_optimal_device", lambda: torch.device("cuda", 1))
    monkeypatch.setattr(shared.cmd_opts, "mdtile_devices", "0", raising=False)
    s = tv.Script()
    try:
        s.process(p, True, 3072, 256, True, True, True, False)
        assert dec.forward.devices == [1, 0] and enc.forward.devices == [1, 0]     # the VAE will run on cuda:1 (no parameters here)
        assert dec.forward.devices is not enc.forward.devices
        monkeypatch.setattr(shared.cmd_opts, "mdtile_devices", None)
        s.process(p, True, 3072, 256, True, True, True, False)
        assert dec.forward.devices is None and enc.forward.devices is None
    finally:
        s.postprocess(p, None, True)
