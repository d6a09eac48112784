"""
The Tiled-VAE PROGRAM and its geometry helpers: upstream's task queue (scripts/tilevae.py:107-204) with the fusions the engine offers
already applied, the live-window arithmetic of the fast-mode decoder, crop_valid_region (:248-259), the slow-mode statistics collector
(GroupNormParam, :289-335), the resolved route (resolve_route: which engine call every step takes in a given mode, who applies every
norm, which forms a conv writes; VAEHook._advance executes it) and the per-tile executor state.  Pure host code: switches arrive as
arguments, no device work besides what the packed convs / the engine do when called.  scripts/tilevae.py re-exports every name here.
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch
from torch import Tensor

import mdtile


# ---------------------------------------------------------------------------------------------------------------------
# program = upstream's task queue, with the fusions the engine offers already applied
# ---------------------------------------------------------------------------------------------------------------------

class Step:
    __slots__ = ("kind", "conv", "norm", "silu", "attn", "fuse_res", "upsample", "downsample", "channels")

    def __init__(self, kind, conv=None, norm=None, silu=False, attn=None, fuse_res=False, upsample=False, downsample=False, channels=0):
        self.kind, self.conv, self.norm, self.silu, self.attn = kind, conv, norm, silu, attn
        self.fuse_res, self.upsample, self.downsample = fuse_res, upsample, downsample
        self.channels = channels      # norm steps: the GroupNorm's channel count


class AttnPack:
    """q/k/v/proj_out of one AttnBlock, packed for the engine; v is produced token-major for the PV contraction."""

    def __init__(self, attn, pack=None, engine=None):
        # the engine's own packer marks these 1x1 convs as the attention's (PRECISION_F16: they follow its arithmetic, nin_shortcut does not);
        # an injected packer (the CPU tests' torch doubles) is called as it always was
        pack = pack or (lambda conv: _pack(conv, attn_proj=True))
        self.engine = engine or mdtile
        self.q, self.k, self.v, self.proj = (pack(attn.q), pack(attn.k), pack(attn.v), pack(attn.proj_out))
        self.channels = attn.q.weight.shape[0]

    def __call__(self, h: Tensor, residual: Tensor) -> Tensor:
        B, C, H, W = h.shape
        q = self.q(h).view(B, C, H * W)
        k = self.k(h).view(B, C, H * W)
        scale = float(int(C) ** (-0.5))
        if getattr(self.engine, "v_channel_major_ok", lambda c: False)(C):
            # v like q and k: channel-major through the split-bf16 1x1 kernel; the attention prep reads it in that layout
            o = self.engine.vae_attn(q, k, self.v(h).view(B, C, H * W), scale, v_channel_major=True)
        else:
            o = self.engine.vae_attn(q, k, self.v(h, token_major=True), scale)     # softmax(q^T k / sqrt(C)) v   (attn.py:55-67)
        return self.proj(o.view(B, C, H, W), residual=residual)        # proj_out + the queue's add_res


def _pack(conv, attn_proj: bool = False) -> mdtile.PackedConv:
    if conv.stride == (2, 2):
        # ldm Downsample.conv: 3x3, stride 2, no padding (the module pads right/bottom by one itself) -> PackedConv.down2
        assert conv.kernel_size == (3, 3) and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1, f"unsupported conv {conv}"
        return mdtile.PackedConv(conv.weight.detach().float().contiguous(), None if conv.bias is None else conv.bias.detach().float())
    assert conv.stride == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1, "engine convs are stride-1 (or ldm Downsample) dense"
    k = conv.kernel_size[0]
    assert conv.kernel_size == (k, k) and conv.padding == (k // 2, k // 2), f"unsupported conv {conv}"
    return mdtile.PackedConv(conv.weight.detach().float().contiguous(),
                             None if conv.bias is None else conv.bias.detach().float(), attn_proj=attn_proj)


def _norm_params(gn):
    assert gn.num_groups == 32, "Tiled VAE hard-codes 32 groups (upstream tilevae.py:299)"
    g = gn.weight.detach().float().contiguous() if getattr(gn, "weight", None) is not None else None
    b = gn.bias.detach().float().contiguous() if getattr(gn, "bias", None) is not None else None
    return g, b


def _resblock(steps: List[Step], blk, pack):
    if blk.in_channels != blk.out_channels:
        shortcut = blk.conv_shortcut if blk.use_conv_shortcut else blk.nin_shortcut
        steps.append(Step("store_res", conv=pack(shortcut)))
    else:
        steps.append(Step("store_res"))
    steps.append(Step("norm", norm=_norm_params(blk.norm1), silu=True, channels=blk.norm1.num_channels))
    steps.append(Step("conv", conv=pack(blk.conv1)))
    steps.append(Step("norm", norm=_norm_params(blk.norm2), silu=True, channels=blk.norm2.num_channels))
    steps.append(Step("conv", conv=pack(blk.conv2), fuse_res=True))       # conv2 + add_res in one epilogue


def build_task_queue(net, is_decoder: bool = True, pack=None, engine=None) -> List[Step]:
    """Linearise an ldm Decoder exactly in upstream's order (:139-195): conv_in, mid(res, attn, res), levels top-down
    with num_res_blocks+1 resblocks (+ upsample except on level 0), norm_out, silu, conv_out.  30 norms for SD/SDXL.
    `pack` turns an nn.Conv2d into the callable a step carries and `engine` is the module the attention step calls
    (defaults: mdtile.PackedConv / mdtile; the CPU tests of the host logic inject torch doubles, tests/torch_engine.py)."""
    attn_pack = pack          # None: AttnPack uses the engine's packer with attn_proj set
    pack = pack or _pack
    steps = [Step("conv", conv=pack(net.conv_in))]

    def _mid():
        _resblock(steps, net.mid.block_1, pack)
        steps.extend([Step("store_res"), Step("norm", norm=_norm_params(net.mid.attn_1.norm), channels=net.mid.attn_1.norm.num_channels),
                      Step("attn", attn=AttnPack(net.mid.attn_1, attn_pack, engine))])
        _resblock(steps, net.mid.block_2, pack)

    if is_decoder:
        _mid()
        for lvl in reversed(range(net.num_resolutions)):
            for i in range(net.num_res_blocks + 1):
                _resblock(steps, net.up[lvl].block[i], pack)
            if lvl != 0:
                steps.append(Step("conv", conv=pack(net.up[lvl].upsample.conv), upsample=True))  # nearest-2x fused
    else:
        # encoder (upstream :155-171): levels bottom-up with num_res_blocks resblocks (+ downsample except on the last), then mid
        for lvl in range(net.num_resolutions):
            for i in range(net.num_res_blocks):
                _resblock(steps, net.down[lvl].block[i], pack)
            if lvl != net.num_resolutions - 1:
                steps.append(Step("conv", conv=pack(net.down[lvl].downsample.conv), downsample=True))
        _mid()
    if not is_decoder or not net.give_pre_end:
        steps.append(Step("norm", norm=_norm_params(net.norm_out), silu=True, channels=net.norm_out.num_channels))
        steps.append(Step("conv", conv=pack(net.conv_out)))
        if is_decoder and net.tanh_out:
            steps.append(Step("tanh"))
    return steps



def crop_valid_region(x, input_bbox, target_bbox, is_decoder):
    padded = [i * 8 if is_decoder else i // 8 for i in input_bbox]
    m = [target_bbox[i] - padded[i] for i in range(4)]
    return x[:, :, m[2]:x.size(2) + m[3], m[0]:x.size(3) + m[1]]


def live_windows(steps: List["Step"], tile_hw: Tuple[int, int], valid: Tuple[int, int, int, int]):
    """Live-window narrowing of ONE decoder tile whose GroupNorm statistics are all frozen (fast mode).

    Upstream decodes the whole padded tile and crop_valid_region (:248-259, applied at :630-632) keeps `valid` (y0, x0, y1, x1 in latent
    px relative to the tile; the padding -- 11 latent px for the decoder, :371 -- is thrown away).  With frozen statistics every layer
    behind the attention is local (3x3 convs, 1x1 convs, pointwise norm / SiLU, nearest 2x), so an output pixel further than the number
    of 3x3 convs still to come from the valid region cannot reach it and need not be computed.  The plane is narrowed where it is
    cheapest, at the upsample convs: walking the program backwards, `need` counts the 3x3 convs behind a point in pixels of that
    level; at the upsample conv that opens a level of `scale` px per latent px the plane becomes `valid` grown by
    ceil(need / scale) latent px (whole latent px: the tile's own crop and store stay in latent units), clamped to the tile, and
    the level below has to provide ceil((need + 1) / 2) px: an output pixel d px outside the valid region reads the nearest-2x
    image d - 1 .. d + 1 px outside, i.e. input pixels up to ceil((d + 1) / 2) px outside (the window's own outermost inputs come
    from the un-narrowed input image, so they are its true neighbours).  A narrowed plane is a zero-padded image of its own: its
    errors creep inwards one pixel per conv and stop at the valid region.  The walk ends at the attention (it needs every token).
    SD decoder (3 resblocks per level, conv_out): need = 7, 10, 12 px -> grow = 1, 3, 6 latent px for the 8x, 4x, 2x levels; the 1x
    level would need 13 of its 11 px of padding and stays whole.  (tests/test_vae_host_logic.py: exact and tight in float64.)

    Returns ({index of the upsample step: (y0, x0, h, w) window of ITS input plane, in input px}, final rect in latent px relative to
    the tile (y0, x0, y1, x1)) -- ({}, whole tile) when nothing can be shed."""
    th, tw = tile_hw
    whole = (0, 0, th, tw)
    ups = [i for i, s in enumerate(steps) if s.kind == "conv" and s.upsample]
    if not ups or any(s.kind == "conv" and s.downsample for s in steps):
        return {}, whole
    scale, need, grow = 1 << len(ups), 0, {}
    for i in range(len(steps) - 1, -1, -1):
        s = steps[i]
        if s.kind == "attn":
            break
        if s.kind != "conv":
            continue                       # frozen norm, SiLU, residual bookkeeping (+ 1x1 nin_shortcut), tanh: pointwise
        ks = int(getattr(s.conv, "ksize", 3))
        if s.upsample:
            grow[i] = -(-need // scale)    # whole latent px
            scale //= 2
            need = (need + ks // 2 + 1) // 2
        else:
            need += ks // 2
    vy0, vx0, vy1, vx1 = valid
    windows, cur, in_scale = {}, whole, 1
    for i in ups:
        if i in grow:
            m = grow[i]
            rect = (max(cur[0], vy0 - m), max(cur[1], vx0 - m), min(cur[2], vy1 + m), min(cur[3], vx1 + m))
            if rect != cur:
                windows[i] = ((rect[0] - cur[0]) * in_scale, (rect[1] - cur[1]) * in_scale,
                              (rect[2] - rect[0]) * in_scale, (rect[3] - rect[1]) * in_scale)
                cur = rect
        in_scale *= 2
    return windows, cur


class GroupNormParam:
    """Slow-mode collector: per-tile (var, mean) rows pooled by pixel count (upstream :289-335)."""

    def __init__(self, engine=None):
        self.engine = engine or mdtile
        self.var_list, self.mean_list, self.pixel_list = [], [], []

    def add_stats(self, var: Tensor, mean: Tensor, pixels: int):
        """The (var, mean) rows of a tile of `pixels` px."""
        self.var_list.append(var)
        self.mean_list.append(mean)
        self.pixel_list.append(pixels)

    def summary(self) -> Optional[Tuple[Tensor, Tensor]]:
        if not self.var_list:
            return None
        return self.engine.gn_pool(torch.vstack(self.mean_list), torch.vstack(self.var_list), self.pixel_list)


# ---- the resolved route: what runs at step i in a given mode, decided ONCE per sweep (VAEHook._advance executes it) ----------------
class Routed:
    """One step of a resolved route.  conv steps -- how:
      "down"            ldm Downsample (stride 2; no norm in front of it)
      "rec"             record conv; a conversion pass (taking the pending coefficients) comes first when its input is fp32
      "rec_stats"       the same, and the conv leaves get_var_mean of its output (the input of a pooled norm)
      "handover_stats"  fp32 hand-over conv applying the pending coefficients while staging + statistics from its epilogue
      "plain"           the conv's own call: applies pending coefficients only where fuses_pre_gn() says it can
      "window_f32"      "plain" for an upsample conv of the hand-over sweep: over the tile's live window where it has one
    pops_res: the conv adds the residual on top of the stack; f32_out / rec_out: the forms a "rec" conv writes -- fp32 NCHW, and a record
    image (None, "raw", or k: already activated with norm k's coefficients + SiLU).
    norm steps -- ordinal k and how:
      "epilogue"        the producing record conv has already applied it (rec_out == k there)
      "convert"         pending (a, s): the conversion pass in front of the record conv behind it applies them
      "ride"            pending (a, s): the conv behind it applies them while staging its input
      "apply"           gn_apply"""
    __slots__ = ("step", "how", "pops_res", "f32_out", "rec_out", "ordinal")

    def __init__(self, step):
        self.step, self.how, self.ordinal, self.f32_out, self.rec_out = step, None, None, True, None
        self.pops_res = step.kind == "conv" and step.fuse_res and not step.downsample


def takes_rec(step: Step, engine, rec_path: bool) -> bool:
    """The conv of `step` runs on the record kernels: the record path on, an engine with record images, a conv they take."""
    fn = getattr(step.conv, "takes_rec", None)
    return bool(rec_path and hasattr(engine, "rec_from_f32") and fn and not step.downsample and fn(step.upsample))


def pooled_site_takes_rec(step: Step, engine, rec_path: bool, slow_rec: bool) -> bool:
    """Slow mode / the estimator pass: a norm whose statistics are pooled cannot be applied by the conv that PRODUCES its input, so the
    record kernels cost an extra conversion pass (fp32 -> activated records) there.  They still win where the conv is long against its
    activation: the 512 -> 512 layers (-7 ... -9 % incl. the pass) and every upsample conv (the pass runs on the quarter-size input:
    -8 ... -21 %); at 256 / 128 input channels the pass costs more than the faster conv saves (+1 ... +8 %) -- profiles/r4z/conv_probe.log.
    conv_out (cout < 32) behind a pooled norm_out: no hand-over kernel applies a norm for so few couts, so the alternative is a norm pass
    (1R + 1W) + the exact-fp32 conv -- 3.8 ms per 2224^2 tile against 1.9 ms for conversion pass + narrow record conv (profiles/r5q:
    kernel_stats_slow.csv, 61 ms of a slow-mode 8K decode)."""
    if not (slow_rec and takes_rec(step, engine, rec_path)):
        return False
    c = step.conv
    return bool(step.upsample or (getattr(c, "cin", 0) >= 512 and getattr(c, "cout", 0) >= 512) or 0 < getattr(c, "cout", 0) < 32)


def resolve_route(steps: List[Step], engine, fuse_pre_gn: bool, rec_path: bool, slow_rec: bool, slow_stats: bool, hand_over: bool,
                  pooled=()) -> List[Routed]:
    """THE one place that decides what every step does: one Routed per step, from the program, the switches and what the engine and the
    packed convs report -- nothing of it depends on the tile.
    hand_over: the whole-tile sweep with every norm frozen.  Producers know the next norm's coefficients, so activations travel between
      the 3x3 convs as record images that the PRODUCING conv writes already normalised + SiLU'd (mdtile_rec_from_f32 behind conv_in /
      attention); a conv writes the forms its consumers read.
    else (slow mode, the estimator pass, semi-fast mode's lockstep sweep -- its frozen norms included): no producer applies a norm; the
      record kernels run behind a conversion pass where pooled_site_takes_rec says they pay, and the producer of the input of a norm
      whose ordinal is in `pooled` leaves that input's statistics where a kernel does (leaves_stats)."""
    n = len(steps)
    ordinal = {i: k for k, i in enumerate(i for i, s in enumerate(steps) if s.kind == "norm")}
    rec = [s.kind == "conv" and (takes_rec(s, engine, rec_path) if hand_over else pooled_site_takes_rec(s, engine, rec_path, slow_rec)) for s in steps]

    def rec_fed(i):          # norm i + SiLU reach the plain record conv behind them as its activated input image
        return steps[i].silu and i + 1 < n and rec[i + 1] and not steps[i + 1].upsample

    route, has_rec = [], False      # has_rec (hand-over sweep): a record image of the current value exists
    for i, s in enumerate(steps):
        r = Routed(s)
        route.append(r)
        j = i + 1            # the consumer of what steps[i] produces; residual bookkeeping (+ nin_shortcut) in between reads fp32
        while j < n and steps[j].kind == "store_res":
            j += 1
        c = steps[j] if j < n else None
        if s.kind == "norm":
            r.ordinal, r.how = ordinal[i], "apply"
            nxt = steps[i + 1] if i + 1 < n else None
            # norm + SiLU in front of a conv can stay pending as (a, s) coefficients; the frozen sweep's conversion pass is no fusion to switch off
            pending = s.silu and nxt is not None and nxt.kind == "conv" and not nxt.downsample and (fuse_pre_gn or hand_over)
            if pending and rec_fed(i):
                r.how, has_rec = ("epilogue" if has_rec else "convert"), hand_over
            elif pending and fuse_pre_gn and (hand_over or not rec[i + 1]) and nxt.conv.fuses_pre_gn(upsample2x=nxt.upsample):
                r.how = "ride"
        elif s.kind == "attn" or (s.kind == "conv" and s.downsample):
            r.how, has_rec = ("down" if s.kind == "conv" else None), False
        elif s.kind == "conv" and hand_over and rec[i] and (has_rec or s.upsample):
            if c is not None and c.kind == "norm" and rec_fed(j):
                r.rec_out = ordinal[j]
            elif c is not None and c.kind == "conv" and c.upsample and rec[j]:
                r.rec_out = "raw"
            r.how, r.f32_out, has_rec = "rec", j > i + 1 or r.rec_out is None, r.rec_out is not None
        elif s.kind == "conv" and hand_over:
            r.how, has_rec = ("window_f32" if s.upsample else "plain"), False
        elif s.kind == "conv":
            has_pre = i > 0 and route[i - 1].how in ("convert", "ride")
            wanted = slow_stats and c is not None and c.kind == "norm" and ordinal[j] in pooled
            stats_fn = getattr(s.conv, "leaves_stats", None) if wanted else None
            r.how = "rec" if rec[i] else "plain"
            if stats_fn is not None and rec[i] and stats_fn(32, upsample2x=s.upsample, rec=True):
                r.how = "rec_stats"
            elif stats_fn is not None and has_pre and not s.upsample and not rec[i] and stats_fn(32):
                r.how = "handover_stats"
    return route


class TileState:
    __slots__ = ("x", "res", "pc", "pre", "stats", "xrec")

    def __init__(self, x):
        self.x, self.res, self.pc = x, [], 0
        self.pre = None   # pending fused pre-activation: gn_coeffs of the norm just resolved, consumed by the next conv
        self.stats = None  # slow mode: (var, mean) of x, left by the conv that produced it (None: nobody has them yet)
        self.xrec = None  # the record image of x, where the producer wrote one (None: x exists as fp32 only)
