"""
Tiled VAE on the mdtile engine -- same plugin surface as upstream scripts/tilevae.py:
`Script.title/show/ui/process/postprocess` with the positional argument order
(enabled, encoder_tile_size, decoder_tile_size, vae_to_gpu, fast_decoder, fast_encoder, color_fix), and a `VAEHook`
callable that replaces `vae.decoder.forward` (upstream :739-745).

What changed underneath (MI355X-first, 288 GB HBM):
  * the ldm Decoder is compiled ONCE into a flat program (upstream's task queue, :107-195) whose steps are mdtile C-ABI
    calls: fp32-MFMA implicit-GEMM convs with fused residual add / nearest-2x upsample, fixed-statistics
    GroupNorm+SiLU in one pass, a flash-style attention kernel (no T x T matrix), crop+store into the result;
  * tiles, residuals and parked activations never leave the GPU (upstream's .cpu()/.to(device) ping-pong, :534-642,
    exists only to fit small VRAM);
  * GroupNorm semantics are upstream's: statistics frozen from a down-sampled latent in fast mode (:542-563, :464-505)
    or pooled across tiles at every norm in slow mode (:320-335) -- NOT the untiled network's.
Both directions run on the engine: the decoder (latent -> image, pad 11) and the encoder (image -> latent moments, pad 32,
stride-2 `Downsample` convs, optional `color_fix` semi-fast mode: statistics frozen only up to the first downsample,
upstream :492-496).
"""
from __future__ import annotations

import contextlib
from time import time
from typing import Dict, List, Optional, Tuple

import torch
from torch import Tensor

import modules.scripts as scripts
import modules.devices as devices
from modules.shared import state

import mdtile


import os as _os
# GroupNorm + SiLU fused into the following 3x3 conv's input staging (engine: mdtile_conv2d_gn).  MDTILE_FUSE_GN=0 keeps the
# separate one-pass GroupNorm+SiLU kernel (A/B measurements, debugging).
FUSE_PRE_GN = _os.environ.get("MDTILE_FUSE_GN", "1") != "0"
# fast mode with every norm frozen: activations travel between the 3x3 convs as split-bf16 record images that the PRODUCING
# conv writes already normalised + SiLU'd (engine: mdtile_conv2d_rec); MDTILE_REC=0 keeps the fp32 hand-over (A/B, debugging)
TILE_BATCH = int(_os.environ.get("MDTILE_TILE_BATCH", "4"))     # fast mode: tiles of equal shape per sweep (see vae_tile_forward); 4 = the four
# corners / top-bottom edges / left-right edges / interior tiles of a 4 x 4 grid each go as ONE stack (3 left a single-tile sweep per group: profiles/r5d)
REC_PATH = _os.environ.get("MDTILE_REC", "1") != "0"
# slow mode and the estimator pass: the record kernels at the pooled-statistics sites where they pay (VAEHook._pooled_site_takes_rec); 0 = fp32 hand-over
SLOW_REC = _os.environ.get("MDTILE_SLOW_REC", "1") != "0"
# slow mode: the conv that produces a pooled norm's input leaves that input's (var, mean) from its own epilogue where such a kernel exists
# (PackedConv.leaves_stats); 0 = a statistics pass over every tile at every norm (A/B, debugging)
SLOW_STATS = _os.environ.get("MDTILE_SLOW_STATS", "1") != "0"
# fast-mode decoder tiles shed their dead border where the resolution doubles (live_windows below); 0 = decode the whole padded tile
LIVE_WINDOW = _os.environ.get("MDTILE_LIVE_WINDOW", "1") != "0"
# multi-GPU fast mode: run the GroupNorm estimator sequence-parallel across the ranks (mdtile/seqpar.py); 0 = every rank
# repeats the whole estimator (no communication, but 1 of every rank's ~3 work units at 8 GPUs)
SP_ESTIMATOR = _os.environ.get("MDTILE_SP_ESTIMATOR", "1") != "0"


def get_rcmd_enc_tsize() -> int:
    """Upstream picks by VRAM (:79-87); every MI355X has 288 GB, i.e. the top bucket."""
    return 3072 if torch.cuda.is_available() else 512


def get_rcmd_dec_tsize() -> int:
    """Upstream: 256 for > 30 GB, 64 off-GPU (:90-99)."""
    return 256 if torch.cuda.is_available() else 64


# the program (task queue with the engine's fusions), its resolved route, live-window arithmetic, crop_valid_region, GroupNormParam, TileState
from tile_utils.vae_program import (AttnPack, GroupNormParam, Routed, Step, TileState, _norm_params, _pack, _resblock,      # noqa: E402,F401
                                    build_task_queue, crop_valid_region, live_windows, pooled_site_takes_rec, resolve_route)


# ---------------------------------------------------------------------------------------------------------------------
# GroupNorm statistics (upstream :207-245; the slow-mode collector GroupNormParam, :289-361, lives in tile_utils/vae_program.py)
# ---------------------------------------------------------------------------------------------------------------------
def get_var_mean(input: Tensor, num_groups: int, eps: float = 1e-6) -> Tuple[Tensor, Tensor]:
    return mdtile.gn_stats(input, num_groups)


def custom_group_norm(input, num_groups, mean, var, weight=None, bias=None, eps=1e-6, silu: bool = False):
    return mdtile.gn_apply(input, mean, var, weight, bias, num_groups, eps, silu)


def _on_device(d: torch.device):
    """torch.cuda.device(d), or nothing off the GPU (the CPU tests' torch doubles of the engine)."""
    return torch.cuda.device(d) if d.type == "cuda" else contextlib.nullcontext()


# ---------------------------------------------------------------------------------------------------------------------
# one process, several devices: the device list (preload.py: --mdtile-devices)
# ---------------------------------------------------------------------------------------------------------------------
def with_vae_device_first(slots: List[int], vae_device: int) -> List[int]:
    """Slot 0 is the VAE's own device: moved to the front (its first entry), or put there when the list lacks it; the order of the
    others is kept."""
    slots = list(slots)
    if vae_device in slots:
        slots.remove(vae_device)
    return [vae_device] + slots


def parse_devices(value: Optional[str], vae_device: int, device_count: int, can_access_peer) -> Optional[List[int]]:
    """The value of --mdtile-devices ("0,1,3" or "all") -> VAEHook.devices, or None (one device).  Repeats are kept (a device may fill
    several slots); the VAE's device becomes slot 0 (with_vae_device_first).  An index that is no CUDA device makes the whole option void
    (warning); a device whose memory the VAE's device cannot read (can_access_peer(vae_device, d) false) is dropped (warning); fewer than
    two slots left give None.  Pure: the caller passes torch.cuda.device_count() and torch.cuda.can_device_access_peer."""
    if value is None or not str(value).strip():
        return None
    value = str(value).strip()
    if value.lower() == "all":
        slots = list(range(device_count))
    else:
        try:
            slots = [int(v) for v in value.split(",") if v.strip()]
        except ValueError:
            print(f"[Tiled VAE]: --mdtile-devices {value!r} is not a comma-separated list of CUDA indices; the option is ignored")
            return None
    bad = [d for d in slots if not 0 <= d < device_count]
    if bad:
        print(f"[Tiled VAE]: --mdtile-devices {value!r}: no CUDA device {bad[0]} ({device_count} visible); the option is ignored")
        return None
    no_peer = sorted({d for d in slots if d != vae_device and not can_access_peer(vae_device, d)})
    if no_peer:
        print(f"[Tiled VAE]: --mdtile-devices: cuda:{vae_device} cannot read the memory of {', '.join(f'cuda:{d}' for d in no_peer)}; "
              "dropped from the list")
        slots = [d for d in slots if d not in no_peer]
    slots = with_vae_device_first(slots, vae_device)
    return slots if len(slots) > 1 else None


PRECISION_NAMES = {"bf16x3": mdtile.PRECISION_BF16X3, "f32": mdtile.PRECISION_F32, "bf16": mdtile.PRECISION_BF16, "f16": mdtile.PRECISION_F16}


def resolve_precision(value, param_dtype) -> Optional[int]:
    """The value of --mdtile-precision -> a mdtile.PRECISION_* mode, or None (option absent: the mode is never touched).  "auto" follows the dtype
    of the decoder's parameters: float16 -> F16, bfloat16 -> BF16, anything else (float32, no parameters) -> BF16X3.  Pure."""
    if value is None or not str(value).strip():
        return None
    value = str(value).strip().lower()
    if value == "auto":
        return {torch.float16: mdtile.PRECISION_F16, torch.bfloat16: mdtile.PRECISION_BF16}.get(param_dtype, mdtile.PRECISION_BF16X3)
    if value not in PRECISION_NAMES:
        print(f"[Tiled VAE]: --mdtile-precision {value!r} is none of {', '.join(PRECISION_NAMES)}, auto; the option is ignored")
        return None
    return PRECISION_NAMES[value]


def _cmd_line_precision(net) -> Optional[int]:
    """--mdtile-precision (preload.py) for the VAE whose decoder is `net`; None when the option is not set."""
    import modules.shared as shared
    value = getattr(shared.cmd_opts, "mdtile_precision", None)
    if not value:
        return None
    p = next(net.parameters(), None)
    return resolve_precision(value, None if p is None else p.dtype)


def _cmd_line_wrap_x() -> bool:
    """--mdtile-wrap-x (preload.py): the canvas is closed in x; False on a host that never heard of the option."""
    import modules.shared as shared
    return bool(getattr(shared.cmd_opts, "mdtile_wrap_x", False))


def _cmd_line_wrap_y() -> bool:
    """--mdtile-wrap-y (preload.py): the canvas is closed in y; False on a host that never heard of the option."""
    import modules.shared as shared
    return bool(getattr(shared.cmd_opts, "mdtile_wrap_y", False))


def _cmd_line_devices(net) -> Optional[List[int]]:
    """--mdtile-devices (preload.py) for the hooks of `net` (the VAE's decoder); None when the option is not set."""
    import modules.shared as shared
    value = getattr(shared.cmd_opts, "mdtile_devices", None)
    if not value:
        return None
    if not torch.cuda.is_available():
        print("[Tiled VAE]: --mdtile-devices needs CUDA devices; the option is ignored")
        return None
    p = next(net.parameters(), None)
    dev = p.device if p is not None and p.device.type == "cuda" else torch.device(devices.get_optimal_device())
    if dev.type != "cuda":
        return None
    index = dev.index if dev.index is not None else torch.cuda.current_device()
    return parse_devices(value, index, torch.cuda.device_count(), torch.cuda.can_device_access_peer)


# ---------------------------------------------------------------------------------------------------------------------
# cross-faded tile borders (preload.py: --mdtile-vae-seam-blend)
# ---------------------------------------------------------------------------------------------------------------------
SEAM_BLEND_MAX = 88      # the decoder's padding: 11 latent px


def seam_grid(in_bboxes, out_bboxes, RH: int, RW: int, band: int, is_decoder: bool = True):
    """The legality rules of mdtile_vae_assemble_blend (include/mdtile.h) on the host, for tiles whose padded output is their input bbox
    scaled: ((rows, cols), None) when the row-major tile list is a grid that admits `band` px per side of every border, else
    (None, reason).  Pure."""
    n = len(out_bboxes)
    if band < 1:
        return None, f"band {band} is smaller than 1"
    if n == 0 or len(in_bboxes) != n:
        return None, "no tiles"
    cols = next((i for i in range(1, n) if out_bboxes[i][2] != out_bboxes[0][2]), n)
    rows = n // cols
    if rows * cols != n:
        return None, f"{n} tiles are no grid of {cols} columns"
    for i, (ib, ob) in enumerate(zip(in_bboxes, out_bboxes)):
        r, c = divmod(i, cols)
        oc, orow = out_bboxes[c], out_bboxes[r * cols]
        if not (ob[0] == oc[0] and ob[1] == oc[1] and ob[2] == orow[2] and ob[3] == orow[3]
                and ob[0] == (0 if c == 0 else out_bboxes[i - 1][1]) and ob[2] == (0 if r == 0 else out_bboxes[i - cols][3])
                and (c < cols - 1 or ob[1] == RW) and (r < rows - 1 or ob[3] == RH) and ob[1] > ob[0] and ob[3] > ob[2]):
            return None, f"tile {i}: its out box {tuple(ob)} does not lie on the {rows} x {cols} grid (hole or overlap)"
        nbx, nby = (c > 0) + (c < cols - 1), (r > 0) + (r < rows - 1)
        w, h = ob[1] - ob[0], ob[3] - ob[2]
        if w < band * nbx:
            return None, f"tile {i}: {w} px wide, " + ("its two column bands overlap" if nbx == 2 and w >= band else "the band is wider than the tile")
        if h < band * nby:
            return None, f"tile {i}: {h} px tall, " + ("its two row bands overlap" if nby == 2 and h >= band else "the band is taller than the tile")
        m = [ob[k] - (ib[k] * 8 if is_decoder else ib[k] // 8) for k in range(4)]
        if m[0] < 0 or m[2] < 0 or m[1] > 0 or m[3] > 0:
            return None, f"tile {i}: inconsistent bboxes (margins {m})"
        if (c > 0 and m[0] < band) or (c < cols - 1 and -m[1] < band) or (r > 0 and m[2] < band) or (r < rows - 1 and -m[3] < band):
            return None, f"tile {i}: margin smaller than the band {band} (margins {m[0]} {-m[1]} {m[2]} {-m[3]})"
    return (rows, cols), None


def _cmd_line_seam_blend() -> Optional[int]:
    """--mdtile-vae-seam-blend (preload.py): image px per side of a tile border, or None (not set, or out of range: one line)."""
    import modules.shared as shared
    value = getattr(shared.cmd_opts, "mdtile_vae_seam_blend", None)
    if value is None:
        return None
    if not isinstance(value, int) or isinstance(value, bool) or not 1 <= value <= SEAM_BLEND_MAX:
        print(f"[Tiled VAE]: --mdtile-vae-seam-blend {value!r} is not in 1 .. {SEAM_BLEND_MAX} image px; the option is ignored")
        return None
    return value


# ---------------------------------------------------------------------------------------------------------------------
# decode only the tiles an inpaint mask touches (preload.py: --mdtile-vae-inpaint-skip)
# ---------------------------------------------------------------------------------------------------------------------
def _cmd_line_vae_inpaint_skip() -> bool:
    """--mdtile-vae-inpaint-skip (preload.py); False on a host that never heard of the option."""
    import modules.shared as shared
    return bool(getattr(shared.cmd_opts, "mdtile_vae_inpaint_skip", False))


def inpaint_skip_refusal(p, is_decoder: bool, all_frozen: bool, seam_set: bool, world: int, wrap: bool, size) -> Tuple[Optional[str], object]:
    """The decision list of --mdtile-vae-inpaint-skip up to the mask itself: (the first reason the skip does not apply, None), or
    (None, the job's overlay mask as an "L" image of `size` = (8 w, 8 h) of this call's latent).  Every attribute of the host's processing
    object is read with getattr: what they mean is the webui's StableDiffusionProcessingImg2Img as remembered, not something this
    extension can verify.  Pure apart from the mask's conversion."""
    if not is_decoder:
        return "this is the encoder (the init image is encoded in full)", None
    if not all_frozen:
        return "not every norm is frozen (the fast decoder is off, or its estimator fell back to slow mode)", None
    if seam_set:
        return "a seam blend is set (--mdtile-vae-seam-blend): a band next to a skipped tile would need that tile's decoded padding", None
    if world > 1:
        return "the decode is sharded over processes (one per GPU)", None
    mask = getattr(p, "mask_for_overlay", None)
    if mask is None:
        return "the job has no overlay mask (mask_for_overlay): not an inpaint job", None
    if not getattr(p, "overlay_images", None):
        return "the job has no overlay images: nothing says that the host pastes the original back", None
    if getattr(p, "inpaint_full_res", False):
        return "inpaint area is 'only masked' (inpaint_full_res): the overlay mask belongs to the whole picture, the decode to the crop", None
    if getattr(p, "color_corrections", None):
        return "the host's colour correction is on: it reads the whole decoded image", None
    if wrap:
        return "wrap-around is on (--mdtile-wrap-x / --mdtile-wrap-y): the decode runs on a padded canvas", None
    try:
        mask = mask if getattr(mask, "mode", None) == "L" else mask.convert("L")
        mask_size = tuple(mask.size)
    except Exception as e:     # not an image at all
        return f"the overlay mask cannot be read as an image ({type(e).__name__})", None
    if mask_size != tuple(size):
        return f"the overlay mask is {mask_size[0]} x {mask_size[1]} px, the decoded image {size[0]} x {size[1]}", None
    return None, mask


class VAEHook:

    def __init__(self, net, tile_size, is_decoder: bool, fast_decoder: bool, fast_encoder: bool, color_fix: bool,
                 to_gpu: bool = False):
        # (signature == upstream's, :364-372.)  engine / _pack / _sp_ops: the mdtile module, the conv packer and the
        # sequence-parallel ops the hook talks to.  The product leaves the defaults (the HIP engine, GPU only); the CPU tests of
        # this host logic overwrite the three attributes with torch doubles (tests/torch_engine.py).
        self.engine = mdtile
        self._pack = None
        self._sp_ops = None
        self.net = net
        self.tile_size = tile_size
        self.is_decoder = is_decoder
        self.fast_mode = (fast_encoder and not is_decoder) or (fast_decoder and is_decoder)
        self.color_fix = color_fix and not is_decoder
        self.to_gpu = to_gpu
        self.pad = 11 if is_decoder else 32
        self._program: Optional[List[Step]] = None
        self.last_seconds = None
        self.shard = (0, 1)   # (rank, world): process-per-GPU runs decode tiles rank, rank+world, ... (mdtile/sharding.py)
        # process-per-GPU runs: the rank whose call returns the ASSEMBLED image, as upstream's single tensor (:630-656) -- the other
        # ranks' tile rectangles travel to it in one grouped exchange; None leaves every rank with only its own tiles filled in
        self.gather_to: Optional[int] = None
        # one process, several devices (what a webui process can use; preload.py: --mdtile-devices): CUDA device indices, one per SLOT,
        # e.g. [0, 1, 2, 3].  Slot 0 is the VAE's own device (put in front when the list lacks it); the tiles are dealt to the slots by
        # area, each slot with its own copy of the packed weights and of the statistics, in every mode (vae_tile_forward: one _Lane per
        # slot).  A device may fill several slots (functional runs on one GPU).
        self.devices: Optional[List[int]] = None
        self.last_tile_slots: Optional[List[int]] = None    # the slot that decoded each tile in the last call
        # decoder only (preload.py: --mdtile-vae-seam-blend): cross-fade every tile border over this many image px per side, out of the
        # padding crop_valid_region throws away (mdtile_vae_assemble_blend).  Every finished tile then lives until the assembly (at 8K /
        # tile 256 about 16 x 59 MB).  0: upstream's edge-to-edge paste, nothing below changes.
        self.seam_blend: int = 0
        # decoder only (preload.py: --mdtile-vae-inpaint-skip): the job's processing object.  vae_tile_forward then decodes only the
        # tiles whose out box the job's overlay mask touches and fills the others from the init image (_inpaint_skip: when, and when
        # not).  None: every tile is decoded, nothing below changes.  Script.postprocess drops the reference.
        self.inpaint_job = None
        self.last_tiles_run: Optional[int] = None           # tiles decoded in the last call (all of them without the skip)
        self._skip_said = False                             # the "not applied" line is printed once per job (a hook lives one job)

    def __call__(self, x):
        original_device = next(self.net.parameters()).device
        try:
            if self.to_gpu:
                self.net = self.net.to(devices.get_optimal_device())
            B, C, H, W = x.shape
            P = self.pad
            # each axis decides for itself: a canvas no larger than two pads along one axis leaves that axis as it is
            pad_x, pad_y = _cmd_line_wrap_x() and W > 2 * P, _cmd_line_wrap_y() and H > 2 * P
            if not (pad_x or pad_y):
                return self._forward(x)
            # the canvas closed in x: every conv would zero-pad at the left and right border; instead the input is padded by the tile pad
            # with the columns of the OTHER edge and runs through the unchanged path; the padding's share of the result is cut off again.
            # The columns next to the seam thus see their true neighbours up to P input px away -- the approximation every interior
            # tile border already gets (upstream's pad of 11 latent / 32 image px).  Closed in y: the same with rows, AFTER the columns, so
            # that on a torus the corners of the padded input come from the diagonal neighbour.
            if pad_x:
                x = torch.cat([x[..., W - P:], x, x[..., :P]], dim=-1)
            if pad_y:
                x = torch.cat([x[..., H - P:, :], x, x[..., :P, :]], dim=-2)
            out = self._forward(x)
            cut = 8 * P if self.is_decoder else P // 8
            if pad_x:
                out = out[..., cut:out.shape[-1] - cut]
            if pad_y:
                out = out[..., cut:out.shape[-2] - cut, :]
            return out.contiguous()
        finally:
            self.net = self.net.to(original_device)

    def _forward(self, x):
        """The body of upstream's __call__ (:375-388): untiled when the input is tiny, else the tiled sweep."""
        B, C, H, W = x.shape
        if max(H, W) <= self.pad * 2 + self.tile_size:
            print("[Tiled VAE]: the input size is tiny and unnecessary to tile.")
            return self.net.original_forward(x)
        return self.vae_tile_forward(x)

    # ---- geometry (host ints via the C ABI) -------------------------------------------------------------------------
    def get_best_tile_size(self, lowerbound, upperbound):
        """Upstream's helper (:390-403): the smallest multiple of 32 / 16 / 8 / 4 / 2 above `lowerbound` that still fits under
        `upperbound`.  The split itself lives behind the C ABI (mdtile_vae_split_tiles uses the same function)."""
        return self.engine.vae_best_tile_size(lowerbound, upperbound)

    def split_tiles(self, h, w):
        return self.engine.vae_split_tiles(h, w, self.tile_size, self.is_decoder)

    def _out_shape(self, z: Tensor, channels: int) -> Tuple[int, int, int, int]:
        """The result's shape for the input z: 8x its size (decoder) or an eighth of it (encoder)."""
        N, _, height, width = z.shape
        return (N, channels, height * 8, width * 8) if self.is_decoder else (N, channels, height // 8, width // 8)

    # ---- program ------------------------------------------------------------------------------------------------------
    def program(self) -> List[Step]:
        dev = next(self.net.parameters()).device
        if self._program is None or self._program_dev != dev:
            self._program = build_task_queue(self.net, self.is_decoder, self._pack, self.engine)
            self._program_dev = dev
        return self._program

    def _route(self, steps: List[Step], hand_over: bool, pooled=()) -> List[Routed]:
        """resolve_route under the switches as they stand NOW: once per vae_tile_forward call and lane program, once more for the estimator
        pass, never kept across calls (a switch or the engine's precision mode may change between two calls)."""
        return resolve_route(steps, self.engine, FUSE_PRE_GN, REC_PATH, SLOW_REC, SLOW_STATS, hand_over, pooled)

    def _pooled_site_takes_rec(self, s: Step) -> bool:
        """The pooled-statistics site of conv step `s` runs on the record kernels (pooled_site_takes_rec: the rule and its measurements)."""
        return pooled_site_takes_rec(s, self.engine, REC_PATH, SLOW_REC)

    def _advance(self, route: List[Routed], st: TileState, norm=None, frozen=None, windows=None):
        """THE executor: advance one tile (or one stack of tiles) along its resolved route --
          neither keyword     to its next GroupNorm (exclusive), or to the end; the statistics a conv leaves of its output go to st.stats;
          norm=(var, mean)    st stands at a norm the sweep has just resolved: through that norm alone (every tile, before any moves on);
          frozen=(stats, coefs)  every norm resolved, (var, mean) and gn_coeffs by ordinal (upstream's single sweep, :578-642): to the end;
                              windows (live_windows): the upsample convs listed there compute only that window of their input plane."""
        E = self.engine
        while st.pc < len(route):
            r = route[st.pc]
            s = r.step
            if s.kind == "norm" and frozen is None and norm is None:
                return
            if s.kind != "store_res":
                st.stats = None                               # (var, mean) describe the tensor that is about to be replaced
            if s.kind == "store_res":
                st.res.append(st.x if s.conv is None else s.conv(st.x))
            elif s.kind == "norm":
                var, mean = norm if frozen is None else frozen[0][r.ordinal]
                if r.how in ("convert", "ride"):
                    # norm + SiLU ride on the conv's input staging (or its conversion pass): only the per-channel (a, s) pair is formed here
                    st.pre = E.gn_coeffs(mean, var, s.norm[0], s.norm[1], st.x.shape[1], 32, 1e-6) if frozen is None else frozen[1][r.ordinal]
                elif r.how == "apply":
                    keep = st.res and st.res[-1] is st.x          # identity shortcut: the residual aliases the pre-norm tensor
                    st.x = E.gn_apply(st.x, mean, var, s.norm[0], s.norm[1], 32, 1e-6, s.silu, out=None if keep else st.x)
                if frozen is None:
                    st.pc += 1
                    return
            elif s.kind == "conv":
                residual = st.res.pop() if r.pops_res else None
                if r.how in ("rec", "rec_stats") and st.xrec is None:
                    # fp32 in front of a record conv: one conversion pass, a pending norm + SiLU fused into it (the pair equals the fp32 hand-over
                    # kernel to fp32 rounding: a fused residual enters the accumulation first here, (res + sum) + bias)
                    st.xrec = E.rec_from_f32(st.x, st.pre)
                if r.how == "down":
                    st.x, st.xrec = s.conv.down2(st.x), None
                elif r.how == "rec_stats":
                    (st.x, st.stats), st.xrec = s.conv.call_rec_stats(st.xrec, residual=residual, upsample2x=s.upsample, groups=32), None
                elif r.how == "handover_stats":
                    st.x, st.stats = s.conv.call_stats(st.x, st.pre, residual=residual, groups=32)
                elif r.how == "rec":
                    win = windows.get(st.pc) if windows else None
                    st.x, st.xrec = s.conv.call_rec(st.xrec, residual=residual, upsample2x=s.upsample, want_f32=r.f32_out, want_rec=r.rec_out is not None,
                                                    rec_coef=None if r.rec_out in (None, "raw") else frozen[1][r.rec_out], **({"window": win} if win else {}))
                elif r.how == "window_f32" and windows and windows.get(st.pc):
                    assert residual is None and st.pre is None      # ldm Upsample: no norm in front, no skip connection into it
                    st.x, st.xrec = self._upconv_window_f32(s.conv, st.x, windows[st.pc]), None
                else:
                    st.x, st.xrec = s.conv(st.x, residual=residual, upsample2x=s.upsample, pre_gn=st.pre), None
                st.pre = None
            elif s.kind == "attn":
                st.x, st.xrec = s.attn(st.x, st.res.pop()), None
            elif s.kind == "tanh":
                st.x = E.tanh(st.x)
            st.pc += 1

    def _tile_batch_that_fits(self, N: int, tile_hw: Tuple[int, int], dev) -> int:
        """Tiles of one shape per sweep (TILE_BATCH at most): what 60 % of the free device memory holds.  Peak of one tile: about five
        live tensors (residual, fp32 activation, two record images, conv output) of 4 B x 128 channels at the widest level -- 8x the
        latent tile for the decoder, the image tile itself for the encoder."""
        if TILE_BATCH <= 1 or torch.device(dev).type != "cuda":
            return max(1, TILE_BATCH)
        h, w = tile_hw
        px = h * w * (64 if self.is_decoder else 1)
        per_tile = 5 * 4 * 128 * px * N
        free, _total = torch.cuda.mem_get_info(dev)
        # blocks torch's caching allocator holds but has handed to nobody are as good as free for the next sweep (after the first decode,
        # or a UNet run, the driver-level figure alone can be tiny on cards smaller than the 288 GB this was developed on)
        free += max(0, torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev))
        tb = max(1, min(TILE_BATCH, int(0.6 * free // max(per_tile, 1))))
        if tb < TILE_BATCH and not getattr(self, "_said_tb", False):
            self._said_tb = True
            print(f"[Tiled VAE]: {tb} instead of {TILE_BATCH} tiles per sweep ({free / 2**30:.1f} GiB free, {per_tile / 2**30:.1f} GiB per {h}x{w} tile)")
        return tb

    @staticmethod
    def _upconv_window_f32(conv, x: Tensor, window) -> Tensor:
        """The window form of an upsample conv that is NOT on the record kernels (exact-fp32 mode, channel counts they do not take): the
        fp32 hand-over kernel over the window plus the conv's own 1 px halo of real neighbours, the halo's outputs cut off afterwards --
        per kept pixel the same arithmetic as the whole-plane call (mdtile_upconv2d_rec_window does this without the two copies)."""
        B, _, H, W = x.shape
        y0s, x0s, h, w = window
        y0s = [int(y0s)] * B if isinstance(y0s, int) else [int(v) for v in y0s]
        x0s = [int(x0s)] * B if isinstance(x0s, int) else [int(v) for v in x0s]
        out, b0 = None, 0
        while b0 < B:                                     # runs of images with one origin (the N latents of one stacked tile)
            b1 = b0 + 1
            while b1 < B and (y0s[b1], x0s[b1]) == (y0s[b0], x0s[b0]):
                b1 += 1
            y0, x0 = y0s[b0], x0s[b0]
            ya, yb, xa, xb = max(y0 - 1, 0), min(y0 + h + 1, H), max(x0 - 1, 0), min(x0 + w + 1, W)
            y = conv(x[b0:b1, :, ya:yb, xa:xb].contiguous(), upsample2x=True)
            oy, ox = 2 * (y0 - ya), 2 * (x0 - xa)
            if out is None:
                out = torch.empty((B, y.shape[1], 2 * h, 2 * w), dtype=y.dtype, device=y.device)
            out[b0:b1] = y[:, :, oy:oy + 2 * h, ox:ox + 2 * w]
            b0 = b1
        return out

    def _live_plan(self, steps: List[Step], in_bbox, out_bbox, grow=(0, 0, 0, 0)):
        """(windows, narrowed input bbox) of one decoder tile for _advance / crop_store -- ({}, in_bbox) when live-window narrowing does
        not apply (switched off, encoder).  grow (left, right, top, bottom; latent px): the valid rectangle grown by what the cross-faded
        assembly reads beyond the out box (seam_blend), clamped to the tile -- narrowing is exact for the rectangle it is given."""
        if not (LIVE_WINDOW and self.is_decoder):
            return {}, tuple(in_bbox)
        x1, x2, y1, y2 = in_bbox
        ox1, ox2, oy1, oy2 = out_bbox
        if any(v % 8 for v in (ox1, ox2, oy1, oy2)):
            return {}, tuple(in_bbox)
        valid = (max(oy1 // 8 - y1 - grow[2], 0), max(ox1 // 8 - x1 - grow[0], 0), min(oy2 // 8 - y1 + grow[3], y2 - y1), min(ox2 // 8 - x1 + grow[1], x2 - x1))
        windows, (ry0, rx0, ry1, rx1) = live_windows(steps, (y2 - y1, x2 - x1), valid)
        return windows, (x1 + rx0, x1 + rx1, y1 + ry0, y1 + ry1)

    @torch.no_grad()
    def estimate_group_norm(self, z: Tensor, steps: List[Step]) -> Optional[List[Tuple[Tensor, Tensor]]]:
        """Fast mode: run the program on the down-sampled latent and freeze (var, mean) at every norm (:464-505).
        Returns None (-> slow mode) if a NaN shows up, as upstream."""
        st = TileState(z)
        frozen = []
        n_norm = sum(1 for s in steps if s.kind == "norm")
        route = self._route(steps, hand_over=False, pooled=range(n_norm))      # every norm's statistics come from this pass itself
        if self.color_fix:
            # semi-fast encoder mode (upstream :492-496): the estimate stops at the first downsample; only the norms before
            # it are frozen, the others are pooled across the tiles as in slow mode
            first_down = next((i for i, s in enumerate(steps) if s.kind == "conv" and s.downsample), len(steps))
            n_norm = sum(1 for s in steps[:first_down] if s.kind == "norm")
        while True:
            self._advance(route, st)
            if st.pc >= len(steps):
                break
            # (the conv that produced st.x has left its statistics where a kernel does that in its epilogue: TileState.stats)
            var, mean = st.stats if st.stats is not None else self.engine.gn_stats(st.x, 32)
            frozen.append((var, mean))
            if len(frozen) == n_norm:
                break
            self._advance(route, st, norm=(var, mean))
        # upstream tests the activation for NaN after every norm (:487-490) and falls back to slow mode; a NaN anywhere upstream of a
        # norm poisons that norm's statistics, so ONE test of the frozen (var, mean) rows at the end sees the same events without a
        # host sync per norm
        if frozen and bool(torch.isnan(torch.stack([v.sum() + m.sum() for v, m in frozen])).any().item()):
            print("Nan detected in fast mode estimation. Fast mode disabled.")
            return None
        return frozen

    def _pooled_across_ranks(self, gp: "GroupNormParam", dev, interrupted: bool = False):
        """Slow mode on several GPUs: all-reduce(sum) of [sum px*mean, sum px*var, sum px] (2*B*32+1 floats) per barrier, on the
        job's data plane (the engine's RCCL communicator when the process has one, mdtile/sharding.py).
        Returns (pooled or None, any rank interrupted).  The interrupt rides in the `head` exchange every rank enters at every pooled
        barrier: a rank that saw state.interrupted keeps walking the barriers (with no tiles) until it has said so HERE, and all ranks
        leave the lockstep loop together -- a rank that simply left would pair its next collective (the 2-float agreement in front of
        the gather) with its peers' `head` and hang them in allreduce_stats."""
        from mdtile import sharding
        BG = None
        if gp.var_list and not interrupted:
            px = torch.tensor(gp.pixel_list, dtype=torch.float32, device=dev).unsqueeze(1)
            sm, sv, sp = (torch.vstack(gp.mean_list) * px).sum(0), (torch.vstack(gp.var_list) * px).sum(0), px.sum().view(1)
            BG = sm.numel()
        # who still has tiles at this barrier, and how wide the statistics rows are (ranks without tiles contribute zeros)
        head = sharding.comm_allreduce_sum(torch.tensor([1.0 if BG else 0.0, float(BG or 0), 1.0 if interrupted else 0.0], dtype=torch.float64, device=dev))
        if head[2].item() > 0.0:
            return None, True
        if head[0].item() == 0.0:
            return None, False
        if BG is None:
            BG = int(round(head[1].item() / head[0].item()))
            sm, sv, sp = torch.zeros(BG, device=dev), torch.zeros(BG, device=dev), torch.zeros(1, device=dev)
        return sharding.allreduce_stats(sm, sv, sp), False

    # ---- one process, several devices ------------------------------------------------------------------------------------------------
    def _slots(self, dev) -> Optional[List[int]]:
        """self.devices with the VAE's own device as slot 0 (with_vae_device_first); None: one device."""
        dev = torch.device(dev)
        if not self.devices or dev.type != "cuda":
            return None
        slots = with_vae_device_first([int(i) for i in self.devices], dev.index if dev.index is not None else torch.cuda.current_device())
        return slots if len(slots) > 1 else None

    def _slot_program(self, index: int) -> List[Step]:
        """The task queue with its weights packed on CUDA device `index`, for slots 1 and up.  Cached on the VAE module: A1111 makes new
        hooks for every generation, and a program is a deep copy + re-pack of the whole VAE.  The key holds every parameter's (data_ptr,
        _version), so an in-place weight load (load_state_dict into the same module: how A1111 swaps a VAE) rebuilds it."""
        import copy
        net = self.net
        key = tuple((p.data_ptr(), p._version) for p in net.parameters())
        cache = getattr(net, "_mdtile_slot_programs", None)
        if cache is None:
            cache = net._mdtile_slot_programs = {}
        hit = cache.get(index)
        if hit is not None and hit[0] == key:
            return hit[1]
        d = torch.device("cuda", index)
        if next(net.parameters()).device != d:
            # the copy leaves out what the plugin hangs on the module: the hooks (with their packed programs) and this cache
            memo = {id(v): None for k, v in vars(net).items() if k in ("forward", "original_forward", "_mdtile_slot_programs")}
            net = copy.deepcopy(net, memo).to(d)
        with torch.cuda.device(d):
            steps = build_task_queue(net, self.is_decoder, self._pack, self.engine)
        cache[index] = (key, steps)
        return steps

    # ---- the tile sweep (upstream vae_tile_forward, :507-656) ------------------------------------------------------------------------
    # vae_tile_forward is the ONE driver: split, estimator, deal the tiles to lanes (one for one device or a rank, one per device slot),
    # run ONE of two sweeps over the lanes, then one tail (_collect):
    #   _sweep_frozen      every norm frozen (fast mode): each tile runs start to finish on its own -- stacked by shape on the record path
    #   _sweep_lockstep    slow mode / color_fix: all tiles advance from norm to norm, statistics pooled at each one
    class _Lane:
        """The tiles of one vae_tile_forward call that one device sweeps -- all of them (one device), this rank's (VAEHook.shard) or one
        device slot's (VAEHook.devices) -- with that device's program, input and frozen statistics, and what the sweeps leave: the tiles'
        state, their live windows, the NaN flags, the interrupt.  keep_tiles (several lanes): finished tiles are kept for
        mdtile_vae_assemble instead of being cropped into the lane's canvas."""

        def __init__(self, hook, z, in_bboxes, out_bboxes, mine: List[int], steps: List[Step], frozen, keep_tiles: bool):
            self.hook, self.z, self.in_bboxes, self.out_bboxes, self.mine = hook, z, in_bboxes, out_bboxes, mine
            self.steps, self.frozen, self.device = steps, frozen, z.device
            self.route = None       # steps resolved for the sweep this call runs (VAEHook._route)
            self.tiles = {i: TileState(self.gather(i)) for i in mine}
            self.result = None
            self.kept = [] if keep_tiles else None      # (tile, its input bbox, output bbox) of every finished tile
            self.nan_flags = []
            self.live = {}          # tile -> (windows of its upsample convs, the input bbox of what is left of it): live_windows
            self.interrupted = False
            self.seam = None        # (band, rows, cols) when this call's tiles are kept for mdtile_vae_assemble_blend (VAEHook.seam_blend)

        def seam_grow(self, i: int):
            """Latent px by which tile i's valid rectangle grows on (left, right, top, bottom): ceil(band / 8) where it has a neighbour."""
            if self.seam is None:
                return (0, 0, 0, 0)
            band, rows, cols = self.seam
            r, c = divmod(i, cols)
            g = -(-band // 8)
            return (g if c > 0 else 0, g if c < cols - 1 else 0, g if r > 0 else 0, g if r < rows - 1 else 0)

        def gather(self, i: int) -> Tensor:
            """The input of tile i, cut out of z."""
            x1, x2, y1, y2 = self.in_bboxes[i]
            return self.hook.engine.gather_rect(self.z, x1, y1, x2 - x1, y2 - y1)

        def finish(self, i: int):
            """crop_valid_region + `result[...] = tile` of one finished tile (upstream :630-632; the canvas appears with the first one), or
            the tile kept for the assembly."""
            hook, x = self.hook, self.tiles[i].x
            in_bbox = self.live[i][1] if i in self.live else self.in_bboxes[i]
            if self.kept is None and self.result is None:
                self.result = torch.zeros(hook._out_shape(self.z, x.shape[1]), device=self.device, dtype=torch.float32)
            self.nan_flags.append(torch.isnan(x).all())       # upstream tests every tile (:626); here ONE host read per call
            if self.kept is None:
                hook.engine.crop_store(x, in_bbox, self.out_bboxes[i], self.result, hook.is_decoder)
            else:
                self.kept.append((x, in_bbox, self.out_bboxes[i]))
            self.tiles[i] = None

    def _sweep_frozen(self, lane: "VAEHook._Lane"):
        """Every norm is already resolved: each tile runs start to finish on its own (upstream: one sweep, :578-642).  A generator that yields
        after every chunk (stack of tiles, or single tile) it has issued: vae_tile_forward drains the lanes' generators in turns."""
        E, z, tiles, steps, frozen = self.engine, lane.z, lane.tiles, lane.steps, lane.frozen
        N, dev = z.shape[0], z.device
        use_rec = REC_PATH and hasattr(E, "rec_from_f32")
        coefs = [E.gn_coeffs(mean, var, s.norm[0], s.norm[1], s.channels, 32, 1e-6)
                 for s, (var, mean) in zip((s for s in steps if s.kind == "norm"), frozen)]
        if use_rec:
            for i in lane.mine:
                lane.live[i] = self._live_plan(steps, lane.in_bboxes[i], lane.out_bboxes[i], lane.seam_grow(i))
        if use_rec and TILE_BATCH > 1:
            # Tiles of one shape go through the sweep TOGETHER (stacked along the batch axis, TILE_BATCH at a time).  Upstream
            # walks them one by one (:578-642); with frozen statistics they are independent, so the result is the same -- but
            # a conv launch over one tile fills the 256 CUs in ceil(items / 256) rounds and the last round is mostly empty
            # (256 -> 256 at 1112^2: 4 900 items = 19.1 rounds, 4 % idle; 512 -> 512 at 278^2: 2.5 rounds, 16 % idle).
            # 288 GB of HBM hold several tiles' activations at once (4 tiles of 278^2: ~53 GB).
            # Tiles stack by (shape, window SIZES of their narrowed upsample convs): each tile keeps its own window ORIGIN
            # (mdtile_upconv2d_rec_window takes one per image), so e.g. the interior tiles of every row share their launches.  A chunk
            # runs start to finish in ONE pass.
            rep_cache: Dict[int, tuple] = {1: (frozen, coefs)}

            def rep(T):                          # frozen statistics / coefficient rows of a T-deep stack (built once per depth)
                if T not in rep_cache:
                    rep_cache[T] = ([(v.repeat(T), m.repeat(T)) for v, m in frozen], [c.repeat(T, 1, 1) for c in coefs])
                return rep_cache[T]

            def regather(chunk):                 # inputs that were folded into a stacked copy: cut them out of z again
                for i in chunk:                  # (tiles of the chunk that already FINISHED -- an OOM inside finish() -- are None: left alone)
                    if tiles[i] is not None:
                        tiles[i].x = lane.gather(i)

            def run_stack(chunk):
                T = len(chunk)
                xb = tiles[chunk[0]].x if T == 1 else torch.cat([tiles[i].x for i in chunk], dim=0)     # (4-channel latent tiles: KBs)
                if T > 1:
                    for i in chunk:
                        tiles[i].x = None          # the stacked copy is the live one
                w0 = lane.live[chunk[0]][0]
                wins = {k: ([lane.live[i][0][k][0] for i in chunk for _ in range(N)], [lane.live[i][0][k][1] for i in chunk for _ in range(N)], w[2], w[3])
                        for k, w in w0.items()} if w0 else None
                stack = TileState(xb)
                self._advance(lane.route, stack, frozen=rep(T), windows=wins)
                for t, i in enumerate(chunk):
                    tiles[i].x = stack.x[t * N:(t + 1) * N]
                    lane.finish(i)

            groups: Dict[tuple, List[int]] = {}
            for i in lane.mine:
                groups.setdefault(tuple(tiles[i].x.shape[2:]) + tuple((k, w[2], w[3]) for k, w in sorted(lane.live[i][0].items())), []).append(i)
            for key in sorted(groups, key=lambda kk: -len(groups[kk])):
                ids = groups[key]
                tb = self._tile_batch_that_fits(N, key[:2], dev)
                if len(key) > 2 and tb * N > 8:       # the group carries narrowed windows (key = shape + window entries):
                    tb = max(1, 8 // N)               # mdtile_upconv2d_rec_window keeps 8 window origins per launch
                c0 = 0
                while c0 < len(ids):
                    if state.interrupted:
                        lane.interrupted = True
                        return
                    chunk = [i for i in ids[c0:c0 + tb] if tiles[i] is not None]      # (after an OOM retry: not the tiles that finished)
                    if not chunk:
                        c0 += tb
                        continue
                    try:
                        run_stack(chunk)
                    except torch.cuda.OutOfMemoryError:
                        if len(chunk) == 1:
                            raise
                        print(f"[Tiled VAE]: {len(chunk)} stacked tiles do not fit in VRAM, continuing one tile per sweep")
                        torch.cuda.empty_cache()
                        regather(chunk)
                        tb = 1
                        continue
                    c0 += tb
                    yield chunk
            return
        for i in lane.mine:
            if state.interrupted:
                lane.interrupted = True
                return
            self._advance(lane.route, tiles[i], frozen=(frozen, coefs), windows=lane.live[i][0] if use_rec else None)
            lane.finish(i)
            yield [i]

    @staticmethod
    def _lockstep_order(lanes: List["VAEHook._Lane"], forward: bool):
        """(lane, tile) in the order _sweep_lockstep advances them to the next norm: every lane walks its tiles forward or reversed (the
        zig-zag); several lanes take turns, one tile each, so that no device waits while another's tiles are issued."""
        orders = [(lane, () if lane.interrupted else lane.mine if forward else lane.mine[::-1]) for lane in lanes]
        for r in range(max((len(o) for _, o in orders), default=0)):
            for lane, o in orders:
                if r < len(o):
                    yield lane, o[r]

    def _sweep_lockstep(self, lanes: List["VAEHook._Lane"]) -> None:
        """Slow mode: all tiles advance in lockstep from norm to norm, the statistics pooled over the tiles (and ranks) at each one
        (upstream :289-361, :578-642 zig-zag); semi-fast (color_fix): the first len(frozen) norms use the frozen statistics instead.
        Each tile's (var, mean) rows go to lane 0's device and are pooled in the order the one-device sweep visits the tiles, and the pooled
        pair goes back to every lane: with several lanes (device slots) the same rows in the same order as on one device, the same bits."""
        E, world = self.engine, self.shard[1]
        lane0 = lanes[0]
        dev0 = lane0.device
        n_frozen = 0 if lane0.frozen is None else len(lane0.frozen)
        forward, k_norm = True, 0
        while True:
            use_frozen = k_norm < n_frozen
            rows = {}                                    # tile -> its (var, mean, pixels) on its lane's device
            for lane, i in self._lockstep_order(lanes, forward):
                if state.interrupted:
                    for ln in lanes:
                        ln.interrupted = True
                    break
                st = lane.tiles[i]
                with _on_device(lane.device):
                    self._advance(lane.route, st)
                    if st.pc < len(lane.steps) and not use_frozen:
                        rows[i] = (*(st.stats if st.stats is not None else E.gn_stats(st.x, 32)), st.x.shape[2] * st.x.shape[3])
            if lane0.interrupted and world == 1:
                return
            # several ranks: an interrupted rank runs no more tiles but keeps walking the norms to the next POOLED barrier, where the
            # `head` exchange tells every rank (see _pooled_across_ranks) -- all of them leave this loop at the same barrier
            if use_frozen:
                # a frozen norm is no barrier upstream (the tile runs straight through it): no pooling, no collective,
                # no change of the zig-zag direction.  A later pooled norm always exists in this branch.
                for lane in lanes:
                    with _on_device(lane.device):
                        for i in (() if lane.interrupted else lane.mine):
                            self._advance(lane.route, lane.tiles[i], norm=lane.frozen[k_norm])
                k_norm += 1
                continue
            # (copied only now: a copy between two devices makes each one's stream wait for the other's, which inside the loop above would
            # tie every slot to the tiles issued before it on slot 0)
            gp = GroupNormParam(E)
            for i in sorted(rows, reverse=not forward):
                var, mean, px = rows[i]
                gp.add_stats(var.to(dev0), mean.to(dev0), px)
            with _on_device(dev0):
                if world == 1:
                    pooled = gp.summary()
                else:
                    pooled, any_interrupted = self._pooled_across_ranks(gp, dev0, lane0.interrupted)
                    if any_interrupted:
                        lane0.interrupted = True
                        return
            k_norm += 1
            for lane in lanes:
                with _on_device(lane.device):
                    if pooled is None:
                        for i in lane.mine:
                            lane.finish(i)
                        continue
                    var, mean = pooled[0].to(lane.device), pooled[1].to(lane.device)
                    for i in lane.mine:
                        self._advance(lane.route, lane.tiles[i], norm=(var, mean))
            if pooled is None:
                return
            forward = not forward

    # ---- decode only the tiles an inpaint mask touches ------------------------------------------------------------------------------
    def _inpaint_skip(self, z: Tensor, out_bboxes, all_frozen: bool, seam_set: bool):
        """--mdtile-vae-inpaint-skip for this call: (one flag per tile, the fill image's bytes on z's device or None), or None when the skip
        does not apply -- the full decode then runs, bit for bit as without the option, and ONE line per job names the first reason
        (inpaint_skip_refusal's list, then: every tile active, or none).
        The premise is the host's overlay paste: for an inpaint job the webui pastes the original image back over the result wherever the
        overlay mask is zero, so what the decoder writes there is thrown away.  A tile whose out box holds no non-zero mask byte is not
        decoded; its box is filled from the job's init image -- p.init_images[0] when there is exactly one, "RGB" (or "L", converted) and of
        the decoded size; its bytes on the device are reused when p.init_image_bytes_md holds that very image -- as byte / 127.5 - 1, or
        with 0.0 when there is no such image.  The fill exists so that previews, the NaN test and --mdtile-color-fix see a sane image; a
        host that rounds (x + 1) / 2 * 255 gets every byte back exactly, the webui's truncating astype(uint8) gets 63 of the 256 values one
        level low, which the overlay hides.  An interrupt that leaves fewer tiles finished than are active pastes what finished and fills
        the rest (_collect)."""
        p = self.inpaint_job
        N, _, h, w = z.shape
        size = (8 * w, 8 * h)
        why, mask = inpaint_skip_refusal(p, self.is_decoder, all_frozen, seam_set, self.shard[1], _cmd_line_wrap_x() or _cmd_line_wrap_y(), size)
        active = None
        if why is None:
            from tile_utils.utils import image_to_device
            active = self.engine.mask_activity_u8(image_to_device(mask).to(z.device).contiguous(), out_bboxes)
            n_active = sum(1 for a in active if a)
            if n_active == len(active):
                why = f"the mask touches all {len(active)} tiles"
            elif n_active == 0:
                why = "the mask touches no tile"
        if why is not None:
            if not self._skip_said:
                self._skip_said = True
                print(f"[Tiled VAE]: --mdtile-vae-inpaint-skip not applied: {why}")
            return None
        fill = None
        images = getattr(p, "init_images", None)
        if isinstance(images, (list, tuple)) and len(images) == 1 and getattr(images[0], "mode", None) in ("RGB", "L") \
                and tuple(getattr(images[0], "size", ())) == size:
            from tile_utils.utils import image_to_device
            kept = getattr(p, "init_image_bytes_md", None)
            if images[0].mode == "RGB" and kept is not None and kept[0] is images[0] and tuple(kept[1].shape) == (size[1], size[0], 3):
                fill = kept[1]
            else:
                fill = image_to_device(images[0] if images[0].mode == "RGB" else images[0].convert("RGB"))
            fill = fill.to(z.device).contiguous()
        return active, fill

    @torch.no_grad()
    def vae_tile_forward(self, z: Tensor) -> Tensor:
        t0 = time()
        net = self.net
        dev = next(net.parameters()).device
        dtype = next(net.parameters()).dtype
        E = self.engine
        E.require_device(dev)      # the HIP engine: raises unless the VAE sits on the GPU (no CPU path exists)
        z = z.detach().to(device=dev, dtype=torch.float32).contiguous()
        N, _, height, width = z.shape
        net.last_z_shape = z.shape
        print(f"[Tiled VAE]: input_size: {z.shape}, tile_size: {self.tile_size}, padding: {self.pad}")
        in_bboxes, out_bboxes = self.split_tiles(height, width)
        steps = self.program()
        rank, world = self.shard
        slots = self._slots(dev)
        if slots and world > 1:
            raise RuntimeError("[Tiled VAE]: VAEHook.devices (one process, several devices) and a process-per-GPU shard cannot be combined")
        seam = None
        if self.seam_blend and self.is_decoder and len(in_bboxes) > 1:
            if world > 1:
                raise RuntimeError("[Tiled VAE]: VAEHook.seam_blend (cross-faded tile borders) and a process-per-GPU shard (VAEHook.shard) cannot "
                                   "be combined: the root would need its neighbours' padding")
            grid, why = seam_grid(in_bboxes, out_bboxes, height * 8, width * 8, int(self.seam_blend), True)
            if grid is None:
                print(f"[Tiled VAE]: seam blend of {self.seam_blend} px does not fit this tile grid ({why}); tiles are pasted edge to edge")
            else:
                seam = (int(self.seam_blend), *grid)

        frozen = None
        if self.fast_mode:
            zs = E.vae_fast_input(z, self.tile_size)
            print(f"[Tiled VAE]: Fast mode enabled, estimating group norm parameters on {zs.shape[3]} x {zs.shape[2]} image")
            if world > 1 and SP_ESTIMATOR and self.is_decoder and zs.shape[2] >= 2 * world:
                # the estimator is one untiled pass: split it by rows across the ranks instead of repeating it on each
                from mdtile import seqpar
                frozen = seqpar.estimate_group_norm_sp(steps, zs, seqpar.BandComm(rank, world), self._sp_ops or seqpar.EngineOps(), FUSE_PRE_GN)
            else:
                frozen = self.estimate_group_norm(zs, steps)
        n_norm = sum(1 for s in steps if s.kind == "norm")
        all_frozen = frozen is not None and len(frozen) == n_norm

        # one lane for one device or this rank, one per device slot (the slots after the first with their own program and copies of z and
        # of the frozen statistics); the tiles dealt by area (mdtile/sharding.py: deal_tiles), the same list on every rank
        from mdtile import sharding
        devs = [torch.device("cuda", i) for i in slots] if slots else [dev]
        # (the decision needs the estimator's outcome, and the masks the host computes after Script.process: made here, once per call)
        skip = self._inpaint_skip(z, out_bboxes, all_frozen, seam is not None) if self.inpaint_job is not None else None
        if skip is None:
            owner = sharding.deal_tiles(in_bboxes, len(devs) if slots else world)
        else:
            # only the active tiles are gathered, dealt and swept; a skipped tile belongs to no lane (-1)
            run = [i for i, a in enumerate(skip[0]) if a]
            owner = [-1] * len(in_bboxes)
            for i, o in zip(run, sharding.deal_tiles([in_bboxes[i] for i in run], len(devs))):
                owner[i] = o
            print(f"[Tiled VAE]: decoding {len(run)} of {len(in_bboxes)} tiles (inpaint mask)")
        self.last_tile_slots = list(owner) if world == 1 else None
        lanes = []
        for k, d in enumerate(devs):
            with _on_device(d):
                lane_steps = steps if k == 0 else self._slot_program(d.index)
                lane_frozen = frozen if k == 0 or frozen is None else [(v.to(d), m.to(d)) for v, m in frozen]
                mine = [i for i, o in enumerate(owner) if o == (k if slots else rank)]
                lanes.append(VAEHook._Lane(self, z if k == 0 else z.to(d), in_bboxes, out_bboxes, mine, lane_steps, lane_frozen,
                                           keep_tiles=bool(slots) or seam is not None or skip is not None))
                lanes[-1].seam = seam
                # every norm frozen: the hand-over sweep; else the lockstep sweep, the statistics of the norms behind the frozen ones pooled
                lanes[-1].route = self._route(lane_steps, all_frozen, () if all_frozen else range(len(frozen or ()), n_norm))
        self.last_tiles_run = sum(len(lane.mine) for lane in lanes)
        if all_frozen:
            sweeps = [(lane, self._sweep_frozen(lane)) for lane in lanes]
            while sweeps:                                # one chunk of every lane per round: no device waits while another's list is issued
                still = []
                for lane, sweep in sweeps:
                    with _on_device(lane.device):
                        if next(sweep, None) is not None:
                            still.append((lane, sweep))
                sweeps = still
        else:
            self._sweep_lockstep(lanes)
        return self._collect(lanes, owner, dtype, t0, None if skip is None else skip[1], skip is not None)

    def _collect(self, lanes: List["VAEHook._Lane"], owner: List[int], dtype, t0, fill=None, sparse: bool = False) -> Tensor:
        """The result on lane 0's device: the tiles kept by several lanes read into one image (mdtile_vae_assemble, peer reads, after lane
        0's stream has waited for the other devices' -- events, no host synchronize), the NaN test of the image (upstream :633-634), the
        gather of the other ranks' rectangles, upstream's interrupt results (:644-650); one host synchronize at the end.
        sparse (the inpaint skip, _inpaint_skip): the kept tiles are the active ones only; mdtile_vae_assemble_sparse pastes them and fills
        every other out box from `fill` (the init image's bytes on lane 0's device, or None: 0.0).  After an interrupt the tiles that
        finished are pasted and the rest filled, active or not."""
        from mdtile import sharding
        z, dev, result = lanes[0].z, lanes[0].device, lanes[0].result
        rank, world = self.shard
        interrupted = any(lane.interrupted for lane in lanes)
        kept = [t for lane in lanes if lane.kept for t in lane.kept]
        with _on_device(dev):
            for lane in lanes[1:]:
                if lane.device != dev:
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream(lane.device))
                    torch.cuda.current_stream(dev).wait_event(ev)
            seam = lanes[0].seam
            if kept and seam is not None and (interrupted or len(kept) != len(owner)):
                print(f"[Tiled VAE]: interrupted with {len(kept)} of {len(owner)} tiles finished; no seam blend, the finished tiles are pasted edge to edge")
                seam = None
            if kept and seam is not None:
                # (the lanes finish their tiles in their own order: row-major again, as the grid wants them)
                kept.sort(key=lambda t: (t[2][2], t[2][0]))
                result = torch.empty(self._out_shape(z, kept[0][0].shape[1]), device=dev, dtype=torch.float32)
                self.engine.vae_assemble_blend(kept, seam[1], seam[2], result, seam[0], self.is_decoder)
            elif kept and sparse:
                # the tiles that were decoded (after an interrupt: those that finished), every other out box filled (sparse: the inpaint skip)
                done = {tuple(ob) for _, _, ob in kept}
                result = torch.empty(self._out_shape(z, kept[0][0].shape[1]), device=dev, dtype=torch.float32)
                self.engine.vae_assemble_sparse(kept, [ob for ob in lanes[0].out_bboxes if tuple(ob) not in done],
                                                fill if fill is not None and fill.shape[-1] == result.shape[1] else None, result)
            elif kept:
                result = torch.zeros(self._out_shape(z, kept[0][0].shape[1]), device=dev, dtype=torch.float32)
                self.engine.vae_assemble(kept, result, self.is_decoder)
            flags = [f.to(dev) for lane in lanes for f in lane.nan_flags]
            nan_seen = bool(flags) and bool(torch.stack(flags).any().item())
            if world > 1 and self.gather_to is not None:
                # The gather below is a grouped exchange EVERY rank must enter (or none): a rank that was interrupted, or whose NaN check
                # raises, would leave the others -- and the root's receives -- waiting for ever.  So the ranks first agree on both flags (one
                # small all-reduce), then skip the gather together / raise together.  Upstream tests every tile of the image it returns
                # (tilevae.py:633-634): with the flags summed the root sees a NaN found on any rank.
                agree = torch.tensor([1.0 if interrupted else 0.0, 1.0 if nan_seen else 0.0], dtype=torch.float32, device=dev)
                sharding.comm_allreduce_sum(agree)
                interrupted, nan_seen = (v > 0.0 for v in agree.tolist())
            if nan_seen:
                devices.test_for_nans(torch.full((1,), float("nan")), "vae")     # raises the host's NansException (or not: --disable-nan-check)
            if world > 1 and self.gather_to is not None and not interrupted:
                if result is None and rank == self.gather_to:
                    result = torch.zeros(self._out_shape(z, 3 if self.is_decoder else 2 * int(getattr(self.net, "z_channels", 4))), device=dev,
                                         dtype=torch.float32)
                if result is not None:
                    sharding.gather_tiles_to_root(result, lanes[0].out_bboxes, lambda i: owner[i], rank, self.gather_to)
            if result is not None and dev.type == "cuda":
                torch.cuda.synchronize(dev)              # (several lanes: the assembly has read every lane's tiles, which may go now)
        self.last_seconds = time() - t0
        if result is None:                               # interrupted before any tile finished (upstream :644-650)
            if not self.is_decoder:
                raise RuntimeError("[Tiled VAE]: interrupted before any encoder tile finished")
            from modules import sd_vae_approx
            return torch.cat([torch.nn.functional.interpolate(sd_vae_approx.cheap_approximation(x).unsqueeze(0), scale_factor=8,
                                                              mode="nearest-exact") for x in z], dim=0).to(dev, dtype=dtype)
        if dev.type == "cuda":
            where = f" on {len(lanes)} device slots" if len(lanes) > 1 else ""
            print(f"[Tiled VAE]: Done in {self.last_seconds:.3f}s{where}, max VRAM alloc {torch.cuda.max_memory_allocated(dev) / 2**20:.3f} MB")
        return result.to(dtype)


class Script(scripts.Script):

    def __init__(self):
        self.hooked = False
        self._prev_precision = None      # the engine's mode before --mdtile-precision replaced it (None: not replaced); postprocess puts it back

    def _restore_precision(self):
        if self._prev_precision is not None:
            mdtile.set_precision(self._prev_precision)
            self._prev_precision = None

    def title(self):
        return "Tiled VAE"

    def show(self, is_img2img):
        return scripts.AlwaysVisible

    def ui(self, is_img2img):
        import gradio as gr
        tab = "t2i" if not is_img2img else "i2i"
        uid = lambda name: f"MD-{tab}-{name}"  # noqa: E731
        with gr.Accordion("Tiled VAE", open=False, elem_id=f"MDV-{tab}"):
            with gr.Row():
                enabled = gr.Checkbox(label="Enable Tiled VAE", value=False, elem_id=uid("enable"))
                vae_to_gpu = gr.Checkbox(label="Move VAE to GPU (if possible)", value=True, elem_id=uid("vae2gpu"))
            with gr.Row():
                encoder_tile_size = gr.Slider(label="Encoder Tile Size", minimum=256, maximum=4096, step=16,
                                              value=get_rcmd_enc_tsize(), elem_id=uid("enc-size"))
                decoder_tile_size = gr.Slider(label="Decoder Tile Size", minimum=48, maximum=512, step=16,
                                              value=get_rcmd_dec_tsize(), elem_id=uid("dec-size"))
            with gr.Row():
                fast_encoder = gr.Checkbox(label="Fast Encoder", value=True, elem_id=uid("fastenc"))
                color_fix = gr.Checkbox(label="Fast Encoder Color Fix", value=False, elem_id=uid("fastenc-colorfix"))
                fast_decoder = gr.Checkbox(label="Fast Decoder", value=True, elem_id=uid("fastdec"))
        return [enabled, encoder_tile_size, decoder_tile_size, vae_to_gpu, fast_decoder, fast_encoder, color_fix]

    def process(self, p, enabled: bool, encoder_tile_size: int, decoder_tile_size: int, vae_to_gpu: bool,
                fast_decoder: bool, fast_encoder: bool, color_fix: bool):
        vae = p.sd_model.first_stage_model
        decoder = vae.decoder
        if not enabled:
            if self.hooked:
                for net in (decoder, getattr(vae, "encoder", None)):
                    if net is not None and isinstance(net.forward, VAEHook):
                        net.forward.net = None
                        net.forward.inpaint_job = None
                        net.forward = net.original_forward
            self.hooked = False
            self._restore_precision()
            return
        mode = _cmd_line_precision(decoder)
        if mode is None:
            self._restore_precision()      # (the option went away between two jobs; without it the mode is never touched)
        else:
            prev = mdtile.get_precision()
            if self._prev_precision is None:
                self._prev_precision = prev      # (a job that never reached postprocess: keep what was there before IT)
            mdtile.set_precision(mode)
            names = {v: k for k, v in PRECISION_NAMES.items()}
            print(f"[Tiled VAE]: --mdtile-precision: matrix-core arithmetic {names.get(mode, mode)} for this job (was {names.get(prev, prev)})")
        if not hasattr(decoder, "original_forward"):
            decoder.original_forward = decoder.forward
        self.hooked = True
        slots = _cmd_line_devices(decoder)
        decoder.forward = VAEHook(decoder, decoder_tile_size, is_decoder=True, fast_decoder=fast_decoder,
                                  fast_encoder=fast_encoder, color_fix=color_fix, to_gpu=vae_to_gpu)
        decoder.forward.devices = None if slots is None else list(slots)
        seam_px = _cmd_line_seam_blend()
        if seam_px is not None:                 # the decoder only: the encoder's 4 latent px of padding leave no ramp worth having
            decoder.forward.seam_blend = seam_px
            p.extra_generation_params["Tiled VAE seam blend"] = seam_px
        if _cmd_line_vae_inpaint_skip():        # the decoder only; nothing of the job is read here (the host computes its masks in p.init())
            decoder.forward.inpaint_job = p
            p.extra_generation_params["Tiled VAE inpaint skip"] = True
        encoder = vae.encoder
        if not hasattr(encoder, "original_forward"):
            encoder.original_forward = encoder.forward
        encoder.forward = VAEHook(encoder, encoder_tile_size, is_decoder=False, fast_decoder=fast_decoder,
                                  fast_encoder=fast_encoder, color_fix=color_fix, to_gpu=vae_to_gpu)
        encoder.forward.devices = None if slots is None else list(slots)

    def postprocess(self, p, processed, enabled: bool, *args):
        self._restore_precision()
        if not enabled:
            return
        vae = p.sd_model.first_stage_model
        for net in (vae.decoder, getattr(vae, "encoder", None)):
            if net is not None and isinstance(net.forward, VAEHook):
                net.forward.net = None
                net.forward.inpaint_job = None
                net.forward = net.original_forward
