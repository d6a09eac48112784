"""What the wrap-around tests share (tests/test_gpu_wrap.py, tests/test_gpu_torus.py, tests/test_wrap_host.py, tests/test_torus_host.py): the
bitwise comparison, the model stand-ins, the device maps of both methods, and the stub-host fixtures and engine doubles of the script-wiring
tests.  A plain module, imported by name; the fixtures below become a test module's own by `from wrap_common import host, wired`."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import blend_oracle as bo
from hostsim import stub_host as sh

PLUGIN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multidiffusion-upscaler-for-automatic1111_amd")
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
NAN = float("nan")
N, C = 2, 4
# +-0, +-inf, NaN, denormals, fp16 max, the smallest normal and values near fp32 max
SPECIALS = [0.0, -0.0, float("inf"), float("-inf"), NAN, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 3e-8, 65504.0, 1.17549435e-38, 3.0e38, -3.0e38]


# ---- on the GPU ------------------------------------------------------------------------------------------------------------------
def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def assert_bitwise(got, ref, what):
    """The NaN pattern first, then the bits of everything else."""
    got = got.detach().cpu()
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {ref.dtype} {tuple(ref.shape)}"
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{what}: NaN pattern differs ({int(torch.isnan(got).sum())} vs {int(nan.sum())} NaNs)"
    gb, rb = bits(got), bits(ref)
    z = torch.zeros((), dtype=gb.dtype)
    bad = torch.where(nan, z, gb) != torch.where(nan, z, rb)
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ bitwise; first at {i}: got {got[i].item()!r}, want {ref[i].item()!r}")


def tile_fn(t):
    return bo.synthetic_denoiser(t.float()).to(t.dtype)


def identity(t):
    return t


def on_device(t, cuda, misaligned):
    """The tensor on the device; misaligned: one element into its storage, so that no 16-byte (8-byte) vector load of it is aligned."""
    if not misaligned:
        return t.to(cuda)
    store = torch.zeros(t.numel() + 16, dtype=t.dtype, device=cuda)
    v = store[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == v.element_size() and v.is_contiguous()
    return v


def maps(E, plan, cuda):
    """Device maps of both methods: uniform weight sum; Gaussian tile weight, its weight sum, the reciprocal."""
    g = SimpleNamespace()
    g.weights = torch.zeros(plan.h, plan.w, device=cuda)
    E.weight_map_add_grid(plan, None, g.weights)
    g.tile_w = E.gaussian_weights(plan.tile_w, plan.tile_h, cuda)
    g.gsum = torch.zeros(plan.h, plan.w, device=cuda)
    E.weight_map_add_grid(plan, g.tile_w, g.gsum)
    g.rescale = E.reciprocal(g.gsum)
    return g


def make_delegate(plugin, method, W, H, tile_w, tile_h, ov, bs):
    """(delegate, processing) of one method on a W x H latent canvas, initialised as the script does, its progress bar silenced."""
    cls = plugin.multidiffusion.MultiDiffusion if method == "md" else plugin.mixtureofdiffusers.MixtureOfDiffusers
    p = sh.make_processing(W * 8, H * 8)
    d = cls(p, sh.kdiff_sampler())
    d.init_grid_bbox(tile_w, tile_h, ov, bs)
    d.init_done()
    if d.pbar is not None:
        d.pbar.close()
    d.update_pbar = lambda: None
    return d, p


def evaluate_delegate(d, method, x, shared, cuda):
    """One model evaluation of tile_fn through the delegate -> (its result, the blend restatement's map arguments after `N`)."""
    if method == "md":
        out = d.sample_one_step(x.to(cuda), None, lambda xt, b: tile_fn(xt), None)
        return out, (d.weights.cpu().numpy()[0, 0],)
    shared.sd_model.apply_model_original_md = lambda x_, t_, c_: tile_fn(x_)
    cond = {"c_crossattn": [torch.zeros(N, 77, 768, device=cuda)], "c_concat": [torch.zeros(N, 5, 1, 1, device=cuda)]}
    out = d.apply_model_hijack(x.to(cuda), torch.zeros(N, device=cuda), cond)
    return out, (None, d.get_tile_weights().cpu().numpy(), d.rescale_factor.cpu().numpy()[0, 0])


def gpu_vae_hook(plugin, cuda, is_decoder):
    """(hook on the small network on the device, its tile pad): 11 latent px for the decoder, 32 image px for the encoder."""
    from hostsim import ldm_decoder as ld
    net = (ld.make_decoder(0, small=True) if is_decoder else ld.make_encoder(0, small=True)).to(cuda)
    net.original_forward = net.forward
    ts, P = (16, 11) if is_decoder else (64, 32)
    return plugin.tilevae.VAEHook(net, ts, is_decoder=is_decoder, fast_decoder=True, fast_encoder=True, color_fix=False), P


def set_options(shared, wrap_x, wrap_y):
    """--mdtile-wrap-x / --mdtile-wrap-y on the stub host's command line: set, or gone (a host that never heard of the option)."""
    for name, on in (("mdtile_wrap_x", wrap_x), ("mdtile_wrap_y", wrap_y)):
        if on:
            setattr(shared.cmd_opts, name, True)
        elif hasattr(shared.cmd_opts, name):
            delattr(shared.cmd_opts, name)


# ---- without a GPU: the stub host and the engine's torch doubles -------------------------------------------------------------------
@pytest.fixture
def host(built_lib):
    """(plugin, shared) on the CPU stub host; neither wrap option is set before or after."""
    sh.install("cpu")
    sh.set_device("cpu")
    pl = sh.load_plugin()
    _, shared = sh.host()
    set_options(shared, False, False)
    yield pl, shared
    set_options(shared, False, False)


def gather_rects_double(x_in, rects_xy, w, h, repeat=1, tile_major=True):
    """mdtile.gather_rects in torch (the engine's contract, mdtile/__init__.py): rectangles INSIDE x_in, or an error as the kernel's host check gives."""
    H, W = x_in.shape[-2:]
    for (x, y) in rects_xy:
        assert 0 <= x and x + w <= W and 0 <= y and y + h <= H, f"rect ({x},{y},{w},{h}) outside {W}x{H}"
    cat = torch.cat([x_in[:, :, y:y + h, x:x + w] for (x, y) in rects_xy], dim=0)
    return cat.repeat_interleave(repeat, dim=0) if tile_major else cat.repeat([repeat, 1, 1, 1])


@pytest.fixture
def wired(host, monkeypatch):
    """host, with the engine calls a delegate makes at init / per batch replaced by torch doubles."""
    pl, shared = host
    monkeypatch.setattr(pl.engine, "weight_map_add_grid", lambda plan, tile_w, weights: None)
    monkeypatch.setattr(pl.engine, "gather_rects", gather_rects_double)
    return pl, shared


def delegate(pl, W, H, tile_w, tile_h, ov, bs=4, method="md"):
    """(delegate, processing) with its grid planned and nothing else initialised."""
    cls = pl.multidiffusion.MultiDiffusion if method == "md" else pl.mixtureofdiffusers.MixtureOfDiffusers
    p = sh.make_processing(W * 8, H * 8)
    d = cls(p, sh.kdiff_sampler())
    if method == "mod":
        d.get_weight = lambda w, h: torch.ones(h, w)
    d.init_grid_bbox(tile_w, tile_h, ov, bs)
    return d, p


def load_preload():
    """The plugin's preload.py as a module."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("mdtile_preload", os.path.join(PLUGIN, "preload.py"))
    preload = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(preload)
    return preload


def take(src, box, scale=1):
    """The tile of `box` cut from src with both indices mod the source's size."""
    x, y, w, h = (v * scale for v in box)
    a = src.numpy()
    return a[:, :, ((y + np.arange(h)) % a.shape[-2])[:, None], (x + np.arange(w)) % a.shape[-1]]


def cpu_vae_hook(pl, net, ts, is_decoder):
    """The Tiled VAE hook on the torch doubles of the engine."""
    import torch_engine as te
    net.original_forward = net.forward
    hook = pl.tilevae.VAEHook(net, ts, is_decoder=is_decoder, fast_decoder=True, fast_encoder=True, color_fix=False)
    hook.engine, hook._pack, hook._sp_ops = te.TorchEngine(), te.TorchConv, te.TorchSeqParOps()
    return hook


def pad_rows(z, P):
    return torch.cat([z[..., -P:, :], z, z[..., :P, :]], dim=-2)


def pad_cols(z, P):
    return torch.cat([z[..., -P:], z, z[..., :P]], dim=-1)
