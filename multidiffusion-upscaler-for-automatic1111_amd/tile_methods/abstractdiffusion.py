"""
Delegate base class of the tiling methods -- same role, attribute names and method names as upstream
tile_methods/abstractdiffusion.py, so that the Script (scripts/tilediffusion.py) and third-party monkey patches
land on the same surface.  Everything numerical is delegated to the mdtile engine:

    weights / grid init   upstream :24-28, :173-186   -> mdtile.Plan + mdtile_weight_map_add_grid
    custom bbox rects      upstream :194-215            -> host ints here, maps in the subclasses
    reset_buffer           upstream :97-102             -> nothing to clear: the blend is gather-formulated

    ControlNet / StableSR  upstream :475-588            -> mdtile_gather_rects (slice + cat + repeat in one launch, no tile caches)
    Noise Inversion        upstream :591-747            -> host Euler inversion loop around get_noise (= the blend) and
                                                           mdtile_noise_inverse_blend for the renoise composite (:651-676)
"""
from __future__ import annotations

from types import MethodType
from typing import Dict, List, Optional

import torch
from torch import Tensor

from modules import devices, shared
from modules.shared import state
from modules.processing import opt_f

import mdtile
from tile_utils.utils import (BBox, BBoxSettings, BlendMode, Condition, CustomBBox, NoiseInverseCache, Prompt, get_retouch_mask, grid_shift,
                              lattice_shift, load_region_mask, region_mask_sources, region_rect, shifted_bboxes)

try:  # isinstance targets; absent in a bare test host
    from modules.sd_samplers_kdiffusion import KDiffusionSampler
except Exception:  # pragma: no cover
    KDiffusionSampler = ()
try:
    from modules.sd_samplers_timesteps import CompVisSampler
except Exception:  # pragma: no cover
    CompVisSampler = ()


class AbstractDiffusion:

    # why get_noise never skips tiles (--mdtile-inpaint-skip)
    NOISE_INVERSION_FULL = "Noise Inversion's own evaluations (get_noise) stay full-canvas"
    # why get_noise never moves the grid (--mdtile-grid-shift)
    NOISE_INVERSION_UNSHIFTED = "Noise Inversion's own evaluations (get_noise) follow no sampler step"
    # why get_noise never jitters the grid (--mdtile-grid-jitter)
    NOISE_INVERSION_UNJITTERED = "Noise Inversion's own evaluations (get_noise) follow no sampler step"

    def __init__(self, p, sampler):
        self.method = type(self).__name__
        self.p = p
        self.pbar = None
        self.sampler_name = p.sampler_name
        self.sampler_raw = sampler
        self.sampler = sampler

        if self.is_kdiff and not hasattr(self, "is_edit_model"):
            cfg = self.sampler.model_wrap_cfg
            self.is_edit_model = (shared.sd_model.cond_stage_key == "edit" and cfg.image_cfg_scale is not None
                                  and cfg.image_cfg_scale != 1.0)

        # latent canvas
        self.w: int = int(p.width // opt_f)
        self.h: int = int(p.height // opt_f)
        self.x_buffer: Optional[Tensor] = None   # kept for API compatibility; holds the last blended result
        # sum of tile / background-region weights per latent pixel, fp32 on the device
        self.weights: Tensor = torch.zeros((1, 1, self.h, self.w), device=devices.device, dtype=torch.float32)

        self.step_count = 0
        self.inner_loop_count = 0
        self.kdiff_step = -1

        # grid tiling
        self.enable_grid_bbox = False
        self.plan: Optional[mdtile.Plan] = None
        self.tile_w = self.tile_h = self.tile_bs = self.num_tiles = self.num_batches = None
        self.batched_bboxes: List[List[BBox]] = []
        # --mdtile-wrap-x: the canvas closed in x (init_grid_bbox); wrap_ext = columns by which the last tile column passes the right edge
        self.wrap_x = False
        self.wrap_ext = 0
        # --mdtile-wrap-y: the same for the rows; wrap_ext_y = rows by which the last tile row passes the bottom edge.  Both: a torus
        self.wrap_y = False
        self.wrap_ext_y = 0
        self._wrap_copies: Dict[str, tuple] = {}
        # --mdtile-grid-shift: the wrapped grid moves by step_shift() every sampler step (init_grid_bbox decides; only on a plan that wraps)
        self.grid_shift = False
        self._shift_at: Optional[tuple] = None       # (sampler step, (sx, sy), the step's boxes): every evaluation of one step shares them
        self._shift_notes: set = set()
        # --mdtile-grid-jitter: the plain grid is laid anew every sampler step (init_grid_bbox decides what the geometry allows, step_lattice the rest)
        self.grid_jitter = False
        self.jitter_max_batches = 0                  # most tile batches a step's lattice can have: the progress bar is sized from it
        self._lattice_at: Optional[tuple] = None     # (sampler step, mdtile.Lattice, the step's boxes): every evaluation of one step shares them
        self._jitter_notes: set = set()
        # --mdtile-inpaint-skip: decided on the job's first full-size evaluation (inpaint_skip), when the host has computed p.nmask
        self.skip_mode: Optional[str] = None         # None = not decided yet | "full" | "sparse" | "empty" (the mask touches no tile) | "lattice" (below)
        self.sparse_plan: Optional[mdtile.Plan] = None
        self.sparse_batched_bboxes: List[List[BBox]] = []
        self._skip_notes: set = set()
        # --mdtile-jitter-inpaint-skip: the skip under the jittered grid.  skip_mode "lattice": the active set is another one
        # every step, decided in step_lattice from the job's mask (uploaded once, kept here) and that step's lattice
        self.skip_mask: Optional[Tensor] = None
        self._subset_at: Optional[tuple] = None      # (sampler step, mdtile.LatticeSubset | mdtile.Lattice, its boxes | None): shared like _lattice_at
        self._bar_budget = 0                         # tile batches per step the progress bar was sized with (init_done)

        # region prompt control
        self.enable_custom_bbox = False
        self.custom_bboxes: List[CustomBBox] = []
        self.cond_basis = None
        self.uncond_basis = None
        self.draw_background = True
        self.causal_layers = None
        # --mdtile-wrap-regions: regions on a canvas that wraps (init_custom_bbox decides).  self.weights then stays the GRID's map
        # in plan coordinates and region_w holds the background regions' weight sum on the canvas: the blend adds them per pixel, every step
        self.wrap_regions = False
        self.region_w: Optional[Tensor] = None
        # --mdtile-jitter-regions: regions under the jittered grid (init_custom_bbox decides).  self.weights keeps the fixed grid's
        # sum WITH the regions (Noise Inversion's own evaluations and every other fixed-grid evaluation of the job need it), region_w holds the
        # background regions' sum alone: the lattice blend adds it to the step's grid sum per pixel
        self.jitter_regions = False
        # mask regions (--mdtile-region-masks / p.mdtile_region_masks): at least one region is a painted mask, its rectangle the
        # mask's bounding box and its CustomBBox.cover the pixels it counts for.  The evaluation's blend then goes through blend_mask_regions
        self.mask_regions = False
        self.mask_region_indices: set = set()        # keys of bbox_settings whose region is a painted mask, the dropped ones included

        # optional extensions, armed by the init_* calls of the Script
        self.noise_inverse_enabled = False
        self.sample_img2img_original = None
        self.enable_controlnet = False
        self.controlnet_script = None
        self.control_params = None
        self.org_control_tensor_batch = None
        self.enable_stablesr = False
        self.stablesr_script = None
        self.stablesr_tensor = None

    # ------------------------------------------------------------------------------------------------ host plumbing
    @property
    def is_kdiff(self) -> bool:
        return bool(KDiffusionSampler) and isinstance(self.sampler_raw, KDiffusionSampler)

    @property
    def is_ddim(self) -> bool:
        return bool(CompVisSampler) and isinstance(self.sampler_raw, CompVisSampler)

    def update_pbar(self):
        if self.pbar is None:
            return
        if self.pbar.n >= self.pbar.total:
            self.pbar.close()
        elif self.step_count == state.sampling_step:
            self.inner_loop_count += 1
            if self.inner_loop_count < self.total_bboxes:
                self.pbar.update()
        else:
            self.step_count = state.sampling_step
            self.inner_loop_count = 0

    def reset_buffer(self, x_in: Tensor):
        """Upstream zero-fills an accumulator here (:97-102).  The engine's blend writes every output pixel exactly
        once from a gather, so there is nothing to clear; kept because subclasses / other extensions call it."""
        return None

    def init_done(self):
        if self.enable_custom_bbox and not self.wrap_regions:
            self._refuse_wrap_x_with(self.REGIONS, self.WRAP_REGIONS_HINT)
        if self.wrap_regions and self.noise_inverse_enabled and not self.enable_grid_bbox and self.noise_inverse_renoise_strength > 0:
            raise RuntimeError("[Tiled Diffusion] --mdtile-wrap-regions cannot be combined with Noise Inversion's renoise composite when only "
                               "regions are painted (no background): mdtile_noise_inverse_blend lays its regions on a plain canvas. Draw the "
                               "background, or set the renoise strength to 0.")
        self.total_bboxes = 0
        if self.enable_grid_bbox:
            # --mdtile-grid-jitter: a step's lattice may have a column and a row more than the grid at rest; the bar must not overrun
            moves = self.grid_jitter and (not self.enable_custom_bbox or self.jitter_regions)
            self.total_bboxes += max(self.num_batches, self.jitter_max_batches) if moves else self.num_batches
        if self.enable_custom_bbox:
            self.total_bboxes += len(self.custom_bboxes)
        assert self.total_bboxes > 0, "Nothing to paint! No background to draw and no custom bboxes were provided."
        self._bar_budget = self.total_bboxes
        try:
            from tqdm import tqdm
            self.pbar = tqdm(total=self.total_bboxes * state.sampling_steps, desc=f"{self.method} Sampling: ",
                             disable=getattr(shared.cmd_opts, "mdtile_quiet", False))
        except Exception:  # pragma: no cover
            self.pbar = None

    # ------------------------------------------------------------------------------------------------ cond dict access
    def _tcond_key(self, cond_dict) -> str:
        return "crossattn" if "crossattn" in cond_dict else "c_crossattn"

    def get_tcond(self, cond_dict) -> Tensor:
        t = cond_dict[self._tcond_key(cond_dict)]
        return t[0] if isinstance(t, list) else t

    def set_tcond(self, cond_dict, tcond: Tensor):
        key = self._tcond_key(cond_dict)
        cond_dict[key] = [tcond] if isinstance(cond_dict[key], list) else tcond

    def _icond_key(self, cond_dict) -> str:
        return "c_adm" if shared.sd_model.model.conditioning_key in ("crossattn-adm", "adm") else "c_concat"

    def get_icond(self, cond_dict) -> Tensor:
        i = cond_dict[self._icond_key(cond_dict)]
        return i[0] if isinstance(i, list) else i

    def set_icond(self, cond_dict, icond: Tensor):
        key = self._icond_key(cond_dict)
        cond_dict[key] = [icond] if isinstance(cond_dict[key], list) else icond

    def _vcond_key(self, cond_dict) -> Optional[str]:
        return "vector" if "vector" in cond_dict else None

    def get_vcond(self, cond_dict) -> Optional[Tensor]:
        return cond_dict.get(self._vcond_key(cond_dict))

    def set_vcond(self, cond_dict, vcond: Optional[Tensor]):
        key = self._vcond_key(cond_dict)
        if key is not None:
            cond_dict[key] = vcond

    def make_cond_dict(self, cond_in, tcond: Tensor, icond: Tensor, vcond: Tensor = None):
        out = cond_in.copy()
        self.set_tcond(out, tcond)
        self.set_icond(out, icond)
        self.set_vcond(out, vcond)
        return out

    def slice_icond(self, icond: Tensor, bbox: BBox) -> Tensor:
        """img2img image-conditioning follows the tile (it has the latent's spatial size); txt2img's dummy does not."""
        if tuple(icond.shape[2:]) == (self.h, self.w):
            return self.extended_x(icond, "icond")[bbox.slicer]      # grid tiles of a wrap plan and --mdtile-wrap-regions regions may pass the edge
        return icond

    # ------------------------------------------------------------------------------------------------ grid
    def get_tile_weights(self):
        """Per-tile weight: scalar 1.0 (MultiDiffusion) or a [tile_h, tile_w] map (Mixture of Diffusers)."""
        return 1.0

    @staticmethod
    def wrap_x_requested() -> bool:
        """--mdtile-wrap-x (preload.py); False on a host that never heard of the option."""
        return bool(getattr(shared.cmd_opts, "mdtile_wrap_x", False))

    @staticmethod
    def wrap_y_requested() -> bool:
        """--mdtile-wrap-y (preload.py); False on a host that never heard of the option."""
        return bool(getattr(shared.cmd_opts, "mdtile_wrap_y", False))

    @staticmethod
    def wrap_regions_requested() -> bool:
        """--mdtile-wrap-regions (preload.py); False on a host that never heard of the option."""
        return bool(getattr(shared.cmd_opts, "mdtile_wrap_regions", False))

    @staticmethod
    def inpaint_skip_requested() -> bool:
        """--mdtile-inpaint-skip (preload.py); False on a host that never heard of the option."""
        return bool(getattr(shared.cmd_opts, "mdtile_inpaint_skip", False))

    @staticmethod
    def grid_shift_requested() -> bool:
        """--mdtile-grid-shift (preload.py); False on a host that never heard of the option."""
        return bool(getattr(shared.cmd_opts, "mdtile_grid_shift", False))

    @staticmethod
    def grid_jitter_requested() -> bool:
        """--mdtile-grid-jitter (preload.py); False on a host that never heard of the option."""
        return bool(getattr(shared.cmd_opts, "mdtile_grid_jitter", False))

    @staticmethod
    def jitter_regions_requested() -> bool:
        """--mdtile-jitter-regions (preload.py); False on a host that never heard of the option."""
        return bool(getattr(shared.cmd_opts, "mdtile_jitter_regions", False))

    @staticmethod
    def jitter_inpaint_skip_requested() -> bool:
        """--mdtile-jitter-inpaint-skip (preload.py); False on a host that never heard of the option."""
        return bool(getattr(shared.cmd_opts, "mdtile_jitter_inpaint_skip", False))

    def init_grid_bbox(self, tile_w: int, tile_h: int, overlap: int, tile_bs: int):
        self.enable_grid_bbox = True
        self.requested_tile_bs = int(tile_bs)
        self.requested_grid = (int(tile_w), int(tile_h), int(overlap))
        self.skip_mode, self.sparse_plan, self.sparse_batched_bboxes = None, None, []      # a new grid: the mask is read again
        self.skip_mask, self._subset_at = None, None
        # clamps (tile <= canvas; overlap <= min(requested tile) - 4), origins and batching all happen in the plan
        self.wrap_x = False
        if self.wrap_x_requested():
            if min(int(tile_w), self.w) >= self.w:
                print(f"[Tiled Diffusion] --mdtile-wrap-x ignored: the tile ({tile_w} latent px) is as wide as the canvas ({self.w}), it would meet "
                      "itself across the seam; the plain grid is used.")
            else:
                self.wrap_x = True
        self.wrap_y = False
        if self.wrap_y_requested():      # each axis decides for itself: a tile as tall as the canvas drops wrap-y only
            if min(int(tile_h), self.h) >= self.h:
                print(f"[Tiled Diffusion] --mdtile-wrap-y ignored: the tile ({tile_h} latent px) is as tall as the canvas ({self.h}), it would meet "
                      "itself across the seam; the rows of the plain grid are used.")
            else:
                self.wrap_y = True
        self.grid_shift, self._shift_at = False, None
        if self.grid_shift_requested():
            if self.wrap_x or self.wrap_y:
                self.grid_shift = True
            else:
                print("[Tiled Diffusion] --mdtile-grid-shift ignored: the grid does not wrap around (--mdtile-wrap-x / --mdtile-wrap-y), there is no "
                      "circle to move it on; the grid stays where it is.")
        self.plan = mdtile.Plan(self.w, self.h, tile_w, tile_h, overlap, tile_bs, clamp=True, wrap_x=self.wrap_x, wrap_y=self.wrap_y)
        # wrap-x: tiles that span the seam end at x + w > W; the Python slices below cut them from a copy of their source that repeats its
        # first `wrap_ext` columns behind the last one (extended_x)
        self.wrap_ext = max((b[0] + b[2] - self.w for b in self.plan.bboxes), default=0) if self.wrap_x else 0
        self.wrap_ext_y = max((b[1] + b[3] - self.h for b in self.plan.bboxes), default=0) if self.wrap_y else 0
        if self.grid_shift:      # a shifted tile may start at the last column / row: the whole tile size, fixed for the job (the copies stay valid)
            self.wrap_ext = self.plan.tile_w if self.wrap_x else 0
            self.wrap_ext_y = self.plan.tile_h if self.wrap_y else 0
        self._wrap_copies = {}
        if self.wrap_x or self.wrap_y:
            if getattr(self.p, "extra_generation_params", None) is None:
                self.p.extra_generation_params = {}
            if self.wrap_x:
                self.p.extra_generation_params["Tiled Diffusion wrap x"] = True
            if self.wrap_y:
                self.p.extra_generation_params["Tiled Diffusion wrap y"] = True
            if self.grid_shift:
                self.p.extra_generation_params["Tiled Diffusion grid shift"] = True
        self.tile_w, self.tile_h = self.plan.tile_w, self.plan.tile_h
        self.num_tiles, self.num_batches, self.tile_bs = self.plan.num_tiles, self.plan.num_batches, self.plan.tile_bs
        tile_weights = self.get_tile_weights()
        mdtile.weight_map_add_grid(self.plan, tile_weights if isinstance(tile_weights, Tensor) else None, self.weights)
        self.batched_bboxes = [[BBox(*b) for b in batch] for batch in self.plan.batches]
        self._init_grid_jitter()

    def extended_x(self, t: Tensor, slot: str, scale: int = 1) -> Tensor:
        """wrap-x: cat(t, t[..., :E]) with E = scale * wrap_ext, so that the slice / rectangle of a tile that spans the seam is contiguous in
        it (the columns past the right edge are the first ones again).  Built once per source tensor and kept under `slot` while the source
        stays the same object with the same content version; any other plan returns t itself.
        wrap-y: the copy then gains its own first scale * wrap_ext_y rows behind the last one -- rows AFTER columns, so the corner block of a
        tile that spans both seams is the source's top-left corner."""
        E, Ey = self.wrap_ext * scale, self.wrap_ext_y * scale
        if E <= 0 and Ey <= 0:
            return t
        hit = self._wrap_copies.get(slot)
        if hit is not None and hit[0] is t and hit[1] == t._version:
            return hit[2]
        ext = torch.cat([t, t[..., :E]], dim=-1) if E > 0 else t
        if Ey > 0:
            ext = torch.cat([ext, ext[..., :Ey, :]], dim=-2)
        ext = ext.contiguous()
        self._wrap_copies[slot] = (t, t._version, ext)
        return ext

    # ---- --mdtile-grid-shift: the wrapped grid displaced cyclically, anew every sampler step ---------------------------------
    def job_seed(self) -> int:
        """The job's first seed: p.all_seeds[0], else p.seed, else 0."""
        seeds = getattr(self.p, "all_seeds", None)
        seed = seeds[0] if seeds else getattr(self.p, "seed", None)
        try:
            return int(seed)
        except (TypeError, ValueError):
            return 0

    def step_shift(self, own_evaluation: Optional[str] = None):
        """((sx, sy), the boxes of this evaluation).  With the option active: tile_utils.grid_shift of the job's seed and state.sampling_step on
        the axes that wrap, 0 on the others, and the plan's boxes displaced by it; every evaluation made while the counter keeps its value (cond
        and uncond calls, the slices of a --lowvram batch) gets the same pair, so that CFG subtracts two results of one tiling.
        own_evaluation: an evaluation that never moves the grid names itself here -> shift (0, 0), with one line per job."""
        if not self.grid_shift:
            return (0, 0), self.batched_bboxes
        if own_evaluation is not None:
            if own_evaluation not in self._shift_notes:
                self._shift_notes.add(own_evaluation)
                print(f"[Tiled Diffusion] --mdtile-grid-shift not applied: {own_evaluation}; they run on the grid where it is.")
            return (0, 0), self.batched_bboxes
        step = int(state.sampling_step)
        if self._shift_at is None or self._shift_at[0] != step:
            seed = self.job_seed()
            sx = grid_shift(seed, step, 0, self.w) if self.wrap_x else 0
            sy = grid_shift(seed, step, 1, self.h) if self.wrap_y else 0
            self._shift_at = (step, (sx, sy), shifted_bboxes(self.batched_bboxes, sx, sy, self.w, self.h))
        return self._shift_at[1], self._shift_at[2]

    # ---- --mdtile-grid-jitter: the plain grid laid anew every sampler step, tiles pushed inside the canvas ---------------------
    def _jitter_note(self, reason: str):
        """One line per job and reason why the fixed grid runs although the option is set."""
        if reason not in self._jitter_notes:
            self._jitter_notes.add(reason)
            print(f"[Tiled Diffusion] --mdtile-grid-jitter not applied: {reason}; the grid stays where it is.")

    NO_BACKGROUND_TO_MOVE = "--mdtile-jitter-regions has no grid to move, no background is drawn (the regions are painted where they are)"

    def _jitter_regions_alone(self) -> bool:
        """--mdtile-jitter-regions without --mdtile-grid-jitter means nothing: one line per job says so."""
        if not self.jitter_regions_requested() or self.grid_jitter_requested():
            return False
        if "alone" not in self._jitter_notes:
            self._jitter_notes.add("alone")
            print("[Tiled Diffusion] --mdtile-jitter-regions ignored: it only acts together with --mdtile-grid-jitter; the grid stays where it is.")
        return True

    def _jitter_inpaint_skip_alone(self) -> bool:
        """--mdtile-jitter-inpaint-skip without --mdtile-grid-jitter or without --mdtile-inpaint-skip means nothing: one line per job says so."""
        if not self.jitter_inpaint_skip_requested() or (self.grid_jitter_requested() and self.inpaint_skip_requested()):
            return False
        if "skip alone" not in self._jitter_notes:
            self._jitter_notes.add("skip alone")
            missing = " and ".join(o for o, on in (("--mdtile-grid-jitter", self.grid_jitter_requested()),
                                                   ("--mdtile-inpaint-skip", self.inpaint_skip_requested())) if not on)
            print(f"[Tiled Diffusion] --mdtile-jitter-inpaint-skip ignored: it only acts together with both --mdtile-grid-jitter and "
                  f"--mdtile-inpaint-skip ({missing} is not set); the job runs as without it.")
        return True

    def jitter_inpaint_skip_active(self) -> bool:
        """The three options are set and the geometry lets this job's grid move."""
        return self.grid_jitter and self.inpaint_skip_requested() and self.jitter_inpaint_skip_requested()

    def _init_grid_jitter(self):
        """What the geometry decides, once the plan is made: a canvas that wraps, no axis able to move, more batches than the lattice carries."""
        self.grid_jitter, self._lattice_at, self.jitter_max_batches = False, None, 0
        self._jitter_inpaint_skip_alone()
        if not self.grid_jitter_requested():
            self._jitter_regions_alone()
            return
        if self.wrap_x or self.wrap_y:
            return self._jitter_note("the canvas wraps around on an axis (--mdtile-wrap-x / --mdtile-wrap-y): use --mdtile-grid-shift there")
        plan = self.plan
        if plan.tile_w >= self.w and plan.tile_h >= self.h:
            return self._jitter_note(f"the tile ({plan.tile_w} x {plan.tile_h} latent px) spans the canvas ({self.w} x {self.h}), no axis can move")
        # the most tiles a shift can give: shift 1 on every moving axis
        at_most = mdtile.Lattice(self.w, self.h, *self.requested_grid, self.requested_tile_bs, 1, 1)
        if at_most.num_batches > mdtile.MAX_BATCHES:
            return self._jitter_note(f"up to {at_most.num_tiles} tiles make {at_most.num_batches} batches at tile batch size {self.requested_tile_bs}, more "
                                     f"than the {mdtile.MAX_BATCHES} a lattice carries (raise the tile batch size)")
        self.grid_jitter, self.jitter_max_batches = True, at_most.num_batches

    def step_lattice(self, own_evaluation: Optional[str] = None, skip: str = "full"):
        """(lattice, its boxes in batches) of this evaluation with --mdtile-grid-jitter applied, or None: the fixed grid runs.  The shifts are
        tile_utils.lattice_shift of the job's seed and state.sampling_step on the axes that move; every evaluation made while the counter keeps its
        value (cond and uncond calls, the slices of a --lowvram batch) gets the same lattice, so that CFG subtracts two results of one tiling.
        own_evaluation: an evaluation that never moves the grid names itself here; skip: what --mdtile-inpaint-skip decided for it.  Each reason
        is printed once per job.
        skip "lattice" (--mdtile-jitter-inpaint-skip): the first element is the step's mdtile.LatticeSubset and the boxes are its active tiles'
        -- or the full lattice where every tile is active (or the active ones make too many batches), or boxes None where none is: the caller
        returns a copy of its input and calls no model."""
        if not self.grid_jitter:
            return None
        if own_evaluation is not None:
            return self._jitter_note(own_evaluation)
        if not self.jitter_regions and (self.enable_custom_bbox or not self.draw_background):
            if self.mask_regions and self.jitter_regions_requested():
                return self._jitter_note(self.MASK_REGIONS_FIXED_GRID)
            if self.jitter_regions_requested() and not self.draw_background:
                return self._jitter_note(self.NO_BACKGROUND_TO_MOVE)
            return self._jitter_note("region prompt control is enabled (custom regions, or no background to draw)")
        if skip not in ("full", "lattice"):
            return self._jitter_note(f"--mdtile-inpaint-skip decided \"{skip}\" for this job (tiles are skipped on the fixed grid)")
        step = int(state.sampling_step)
        if self._lattice_at is None or self._lattice_at[0] != step:
            seed = self.job_seed()
            stride_x, stride_y = self.plan.tile_w - self.plan.overlap, self.plan.tile_h - self.plan.overlap
            sx = lattice_shift(seed, step, 0, stride_x) if self.plan.tile_w < self.w else 0
            sy = lattice_shift(seed, step, 1, stride_y) if self.plan.tile_h < self.h else 0
            lat = mdtile.Lattice(self.w, self.h, *self.requested_grid, self.requested_tile_bs, sx, sy)
            self._lattice_at = (step, lat, [[BBox(*b) for b in batch] for batch in lat.batches])
            if getattr(self.p, "extra_generation_params", None) is None:
                self.p.extra_generation_params = {}
            self.p.extra_generation_params["Tiled Diffusion grid jitter"] = True
            if self.jitter_regions:
                self.p.extra_generation_params["Tiled Diffusion jitter regions"] = True
        if skip == "lattice":
            return self._step_subset(step)
        return self._lattice_at[1], self._lattice_at[2]

    def _step_subset(self, step: int):
        """The active tiles of this step's lattice under the job's mask: decided once per sampler step, next to the lattice itself."""
        if self._subset_at is None or self._subset_at[0] != step:
            lat, boxes = self._lattice_at[1], self._lattice_at[2]
            flags, slot = mdtile.lattice_activity(lat, self.skip_mask)
            Ta, T = sum(1 for a in flags if a), len(flags)
            if "first step" not in self._skip_notes:
                self._skip_notes.add("first step")
                print(f"[Tiled Diffusion] inpaint mask touches {Ta} of {T} tiles of the first step's grid (the grid and the count change every step)")
            self.p.extra_generation_params["Tiled Diffusion jitter inpaint skip"] = True
            batches = -(-Ta // max(1, self.requested_tile_bs))
            if Ta == 0:
                grid, boxes = lat, None
            elif Ta == T:
                grid = lat
            elif batches > mdtile.MAX_BATCHES:      # the full lattice passed this limit in _init_grid_jitter with its own, larger, tile batches
                self._skip_note(f"a step's {Ta} touched tiles make {batches} batches at tile batch size {self.requested_tile_bs}, more than the "
                                f"{mdtile.MAX_BATCHES} a lattice subset carries (raise the tile batch size)")
                grid = lat
            else:
                grid = mdtile.LatticeSubset(lat, flags, self.requested_tile_bs, slot)
                boxes = [[BBox(*b) for b in batch] for batch in grid.batches]
            self._subset_at = (step, grid, boxes)
            # the progress bar follows the calls actually made: this step's batches instead of the budget it was sized with
            self.total_bboxes = len(boxes) if boxes is not None else 0
            if self.pbar is not None:
                self.pbar.total += self.total_bboxes - self._bar_budget
                self.pbar.refresh()
        return self._subset_at[1], self._subset_at[2]

    # ---- --mdtile-inpaint-skip: only the tiles the job's latent mask touches ------------------------------------------------------------
    def _skip_note(self, reason: str):
        """One line per job and reason why every tile runs although the option is set."""
        if reason not in self._skip_notes:
            self._skip_notes.add(reason)
            print(f"[Tiled Diffusion] --mdtile-inpaint-skip not applied: {reason}; every tile runs.")

    def _inpaint_mask(self) -> Optional[Tensor]:
        """p.nmask as fp32 [P, H, W] on the device, or None (with the reason noted) when the job has no mask of the latent's size."""
        m = getattr(self.p, "nmask", None)
        if not isinstance(m, Tensor):
            self._skip_note("the job has no inpaint mask (p.nmask)")
            return None
        if m.dim() == 4 and m.shape[0] == 1:
            m = m[0]
        if m.dim() == 2:
            m = m.unsqueeze(0)
        if m.dim() != 3 or tuple(m.shape[-2:]) != (self.h, self.w):
            self._skip_note(f"the mask has size {tuple(getattr(self.p, 'nmask').shape)}, not [{self.h}, {self.w}] / [P, {self.h}, {self.w}] / "
                            f"[1, P, {self.h}, {self.w}]")
            return None
        return m.to(device=devices.device, dtype=torch.float32).contiguous()

    def inpaint_skip(self, own_evaluation: Optional[str] = None) -> str:
        """How this full-size evaluation runs: "full" (every tile), "sparse" (self.sparse_plan / self.sparse_batched_bboxes: the tiles the mask
        touches), "empty" (it touches none: the model is not called) or "lattice" (--mdtile-jitter-inpaint-skip with the grid moving: step_lattice
        decides the active tiles of every step's lattice).  Decided once per job, on the first evaluation that asks -- the host
        computes p.nmask after the delegate is built.  own_evaluation: an evaluation that always runs full-canvas names itself here."""
        if not self.inpaint_skip_requested():
            return "full"
        if own_evaluation is not None:
            self._skip_note(own_evaluation)
            return "full"
        if self.skip_mode is None:
            self.skip_mode = self._decide_inpaint_skip()
        return self.skip_mode

    def _decide_inpaint_skip(self) -> str:
        if self.enable_custom_bbox or not self.draw_background or not self.enable_grid_bbox or self.plan is None:
            self._skip_note("custom regions (region prompt control) are enabled")
            return "full"
        if self.wrap_x or self.wrap_y:
            self._skip_note("the canvas wraps around (--mdtile-wrap-x / --mdtile-wrap-y)")
            return "full"
        mask = self._inpaint_mask()
        if mask is None:
            return "full"
        if self.jitter_inpaint_skip_active():      # the grid moves: which tiles the mask touches is asked of every step's lattice (step_lattice)
            self.skip_mask = mask
            return "lattice"
        active = mdtile.tile_activity(self.plan, mask)
        Ta, T = sum(1 for a in active if a), len(active)
        print(f"[Tiled Diffusion] inpaint mask touches {Ta} of {T} tiles")
        if Ta == T:
            return "full"
        if Ta == 0:
            if self.pbar is not None:       # no model call will be made
                self.pbar.close()
                self.pbar = None
            return "empty"
        batches = -(-Ta // max(1, self.requested_tile_bs))
        if batches > mdtile.MAX_BATCHES:      # a sparse plan has no packed form; the full path packs any number of batches into one buffer
            self._skip_note(f"the {Ta} touched tiles make {batches} batches at tile batch size {self.requested_tile_bs}, more than the "
                            f"{mdtile.MAX_BATCHES} a sparse plan carries (raise the tile batch size)")
            return "full"
        self.sparse_plan = self.plan.subset(active, self.requested_tile_bs)
        self.sparse_batched_bboxes = [[BBox(*b) for b in batch] for batch in self.sparse_plan.batches]
        self.total_bboxes = self.sparse_plan.num_batches      # the progress bar follows the calls actually made
        if self.pbar is not None:
            self.pbar.total = self.total_bboxes * state.sampling_steps
            self.pbar.refresh()
        return "sparse"

    REGIONS = "custom regions (region prompt control)"
    WRAP_REGIONS_HINT = " Or pass --mdtile-wrap-regions: region control on the closed canvas, with regions that may cross the seam."

    def _refuse_wrap_x_with(self, what: str, hint: str = ""):
        if self.wrap_x or self.wrap_y:
            opts = " / ".join(o for o, on in (("--mdtile-wrap-x", self.wrap_x), ("--mdtile-wrap-y", self.wrap_y)) if on)
            raise RuntimeError(f"[Tiled Diffusion] {opts} cannot be combined with {what}: the wrap-around blend has no "
                               "region path. Turn one of them off." + hint)

    MASK_REGIONS_FIXED_GRID = "a region is a painted mask (mask regions are not combined with --mdtile-jitter-regions)"

    def _mask_region(self, number: int, src, blend_mode: str, feather_ratio: float):
        """(x, y, w, h, cover, feather) of the region painted in mask `src`, or None when the mask covers no latent pixel: the rectangle is the
        bounding box of the coverage (the one small copy to the host per region and job), cover and feather come from mdtile.mask_region."""
        mask = load_region_mask(src)
        if mask.shape[0] < self.h or mask.shape[1] < self.w:
            raise RuntimeError(f"[Tiled Diffusion] the mask of region {number} ({mask.shape[1]} x {mask.shape[0]} px) is smaller than the latent canvas "
                               f"({self.w} x {self.h}) on an axis: paint it at the size of the image (or any size from the latent canvas up).")
        cover, box = mdtile.mask_cover_u8(mask, self.w, self.h)
        x0, y0, x1, y1, count = box.tolist()
        if count == 0:
            print(f"[Tiled Diffusion] region {number} dropped: its mask covers no pixel of the {self.w} x {self.h} latent canvas.")
            return None
        fg = BlendMode(blend_mode) == BlendMode.FOREGROUND
        ratio = max(min(feather_ratio, 1.0), 0.0)      # CustomBBox's clamp
        rcover, feather = mdtile.mask_region(cover, x0, y0, x1 - x0, y1 - y0, ratio if fg else None)
        return x0, y0, x1 - x0, y1 - y0, rcover, feather

    def _record_mask(self, index: int, name: Optional[str]):
        """extra_generation_params["Tiled Diffusion"]["Region control"]["Region k"]["mask"] = the file name or "<image>" of a mask that takes part;
        a mask that covered nothing (name None) dropped its region and is not recorded."""
        info = (getattr(self.p, "extra_generation_params", None) or {}).get("Tiled Diffusion")
        region = info.get("Region control", {}).get(f"Region {index + 1}") if isinstance(info, dict) else None
        if isinstance(region, dict):
            if name is None:
                region.pop("mask", None)
            else:
                region["mask"] = name

    def init_custom_bbox(self, bbox_settings: Dict[int, BBoxSettings], draw_background: bool, causal_layers: bool):
        masks = region_mask_sources(self.p, [i for i, s in bbox_settings.items() if s.enable])
        if masks and (self.wrap_x or self.wrap_y):
            opts = " / ".join(o for o, on in (("--mdtile-wrap-x", self.wrap_x), ("--mdtile-wrap-y", self.wrap_y)) if on)
            raise RuntimeError(f"[Tiled Diffusion] mask regions (--mdtile-region-masks / p.mdtile_region_masks) cannot be combined with {opts}, with or "
                               "without --mdtile-wrap-regions: the masked blend runs on a plain canvas only. Turn one of them off.")
        if masks and self.noise_inverse_enabled:
            raise RuntimeError("[Tiled Diffusion] mask regions (--mdtile-region-masks / p.mdtile_region_masks) cannot be combined with Noise Inversion: "
                               "its renoise composite and its own evaluations know rectangles only. Turn one of them off.")
        self.mask_region_indices = set(masks)
        wrap_regions = self.wrap_regions_requested()
        if wrap_regions and not (self.wrap_x or self.wrap_y):
            print("[Tiled Diffusion] --mdtile-wrap-regions ignored: no axis of the canvas wraps around (--mdtile-wrap-x / --mdtile-wrap-y); the "
                  "regions are laid on the plain canvas.")
            wrap_regions = False
        if not wrap_regions:
            self._refuse_wrap_x_with(self.REGIONS, self.WRAP_REGIONS_HINT)
        self.wrap_regions = wrap_regions
        self.jitter_regions = False
        self.enable_custom_bbox = True
        self.causal_layers = causal_layers
        self.draw_background = draw_background
        if not draw_background:
            self.enable_grid_bbox = False
            self.weights.zero_()

        self.custom_bboxes = []
        for index, s in bbox_settings.items():
            enable, fx, fy, fw, fh, prompt, neg, blend_mode, feather_ratio, seed = s
            if enable and index in masks:      # a painted mask: fx, fy, fw, fh are ignored, the rectangle is the mask's bounding box
                made = self._mask_region(index + 1, masks[index][0], blend_mode, feather_ratio)
                self._record_mask(index, masks[index][1] if made is not None else None)
                if made is not None:
                    x, y, w, h, cover, feather = made
                    self.custom_bboxes.append(CustomBBox(x, y, w, h, prompt, neg, blend_mode, feather_ratio, seed, cover=cover, feather=feather))
                    self.custom_bboxes[-1].index = index
                continue
            if not enable or fx > 1.0 or fy > 1.0 or fw <= 0.0 or fh <= 0.0:
                continue
            x, y, w, h = region_rect(fx, fy, fw, fh, self.w, self.h, wrap_regions and self.wrap_x, wrap_regions and self.wrap_y)
            self.custom_bboxes.append(CustomBBox(x, y, w, h, prompt, neg, blend_mode, feather_ratio, seed))
            self.custom_bboxes[-1].index = index      # the region's key in bbox_settings: the noise hijack finds its rectangle and cover by it
        self.mask_regions = any(b.cover is not None for b in self.custom_bboxes)
        if not self.custom_bboxes:
            self.enable_custom_bbox = False
            self.wrap_regions = False
            return
        if wrap_regions:
            self.region_w = torch.zeros((1, 1, self.h, self.w), device=devices.device, dtype=torch.float32)
            # a region that crosses a seam ends at x + w > W (y + h > H): the extended copies the Python slices cut from (extended_x: image
            # conditioning, ControlNet hints, StableSR) grow to the largest overhang of a tile or a region
            self.wrap_ext = max([self.wrap_ext] + [b.x + b.w - self.w for b in self.custom_bboxes])
            self.wrap_ext_y = max([self.wrap_ext_y] + [b.y + b.h - self.h for b in self.custom_bboxes])
            self._wrap_copies = {}
            if getattr(self.p, "extra_generation_params", None) is None:
                self.p.extra_generation_params = {}
            self.p.extra_generation_params["Tiled Diffusion wrap regions"] = True
        # --mdtile-jitter-regions applies when init_grid_bbox decided that this job's grid moves and there is a background to move.  Fixed-grid
        # evaluations still happen in such a job (Noise Inversion's own, the hires pass of another size), so self.weights and the premultiplied
        # region weights are kept as they are and region_w is built beside them
        if self.jitter_regions_requested() and not self._jitter_regions_alone():
            if self.mask_regions:
                if self.grid_jitter:
                    self._jitter_note(self.MASK_REGIONS_FIXED_GRID)
            elif not draw_background:
                self._jitter_note(self.NO_BACKGROUND_TO_MOVE)
            elif self.grid_jitter:
                self.jitter_regions = True
                self.region_w = torch.zeros((1, 1, self.h, self.w), device=devices.device, dtype=torch.float32)
        self._init_region_conds()

    def _init_region_conds(self):
        """Per-region prompt conditioning via the host's prompt parser (skipped when the host has none, e.g. tests)."""
        p = self.p
        if not hasattr(p, "all_prompts") or getattr(shared.sd_model, "cond_stage_model", None) is None:
            return
        prompts = p.all_prompts[:p.batch_size]
        neg_prompts = p.all_negative_prompts[:p.batch_size]
        for bbox in self.custom_bboxes:
            bbox.cond, bbox.extra_network_data = Condition.get_custom_cond(prompts, bbox.prompt, p.steps, p.styles)
            bbox.uncond = Condition.get_uncond(Prompt.append_prompt(neg_prompts, bbox.neg_prompt), p.steps, p.styles)
        self.cond_basis = Condition.get_cond(prompts, p.steps)
        self.uncond_basis = Condition.get_uncond(neg_prompts, p.steps)

    def blend_plan(self) -> mdtile.Plan:
        """The grid plan, or -- when only custom regions are painted and no grid was initialised -- a one-tile plan that
        merely carries the canvas size for the blend launch."""
        if self.plan is None:
            self.plan = mdtile.Plan(self.w, self.h, self.w, self.h, 0, 1, clamp=True)
        return self.plan

    def region_specs(self, outs: List[Tensor], raw: bool = False) -> List[mdtile.RegionSpec]:
        """Pair every custom bbox with its model output for the fused blend launch.  raw: the weights of the lattice path (region_weights)."""
        specs = []
        for bbox, out, wgt in zip(self.custom_bboxes, outs, self.region_weights(raw)):
            mode = mdtile.REGION_FG if bbox.blend_mode == BlendMode.FOREGROUND else mdtile.REGION_BG
            specs.append(mdtile.RegionSpec(bbox.x, bbox.y, bbox.w, bbox.h, mode, out, wgt, cover=bbox.cover))
        return specs

    def gather_region(self, x_in: Tensor, bbox: CustomBBox) -> Tensor:
        """The region's tile of x_in; --mdtile-wrap-regions: cut on the circle, so a region that crosses a seam is one dense tensor."""
        if self.wrap_regions:
            return mdtile.gather_rect_wrap(x_in, bbox.x, bbox.y, bbox.w, bbox.h, wrap_x=self.wrap_x, wrap_y=self.wrap_y)
        return mdtile.gather_rect(x_in, bbox.x, bbox.y, bbox.w, bbox.h)

    def add_region_weight(self, bbox: CustomBBox, rect_w: Optional[Tensor]):
        """A background region's weight (rect_w None: 1.0) into the weight sum: self.weights, or with --mdtile-wrap-regions the canvas map region_w;
        with --mdtile-jitter-regions both -- self.weights for the fixed-grid evaluations, region_w for the lattice blend.
        A mask region counts where it covers: the caller hands its cover as 0.0 / 1.0 floats (MultiDiffusion) or its Gaussian times the cover."""
        if self.wrap_regions:
            mdtile.weight_map_add_rect_wrap(self.region_w, bbox.x, bbox.y, bbox.w, bbox.h, rect_w, 1.0, wrap_x=self.wrap_x, wrap_y=self.wrap_y)
        else:
            mdtile.weight_map_add_rect(self.weights, bbox.x, bbox.y, bbox.w, bbox.h, rect_w, 1.0)
            if self.jitter_regions:
                mdtile.weight_map_add_rect(self.region_w, bbox.x, bbox.y, bbox.w, bbox.h, rect_w, 1.0)

    def blend_wrap_regions(self, method: int, tile_outs: List[Tensor], region_outs: List[Tensor], x_in: Tensor, shift) -> Tensor:
        """--mdtile-wrap-regions: grid (displaced by this step's shift) and regions in one launch; the weight sum is formed in the kernel from
        the grid's map and region_w, and Mixture of Diffusers' region weights go in raw."""
        N, C = x_in.shape[:2]
        tile_w = self.get_tile_weights() if method == mdtile.METHOD_MOD and tile_outs else None
        return mdtile.blend_wrap_regions(self.plan, method, tile_outs, N, C, regions=self.region_specs(region_outs),
                                         grid_w=self.weights if tile_outs else None, region_w=self.region_w, sx=shift[0], sy=shift[1],
                                         tile_w=tile_w, dtype=x_in.dtype, device=x_in.device)

    def blend_lattice_regions(self, method: int, lattice, tile_outs: List[Tensor], region_outs: List[Tensor], x_in: Tensor) -> Tensor:
        """--mdtile-jitter-regions: the step's lattice and the regions in one launch; the weight sum is formed in the kernel from the lattice
        integers and region_w, and Mixture of Diffusers' region weights go in raw."""
        N, C = x_in.shape[:2]
        has_bg = any(b.blend_mode != BlendMode.FOREGROUND for b in self.custom_bboxes)
        return mdtile.blend_lattice_regions(lattice, method, tile_outs, N, C, regions=self.region_specs(region_outs, raw=True),
                                            region_w=self.region_w if has_bg else None,
                                            tile_w=self.get_tile_weights() if method == mdtile.METHOD_MOD else None)

    def region_weights(self, raw: bool = False) -> List[Optional[Tensor]]:
        """Per region: feather mask (foreground) or the method's background weight (None = 1.0).  raw: what the lattice path takes
        (--mdtile-jitter-regions) -- the same here, MultiDiffusion's background weight is the scalar 1.0 either way."""
        return [b.feather_mask if b.blend_mode == BlendMode.FOREGROUND else None for b in self.custom_bboxes]

    # ---- region-prompt forwards (upstream :232-451) --------------------------------------------------------------------
    def reconstruct_custom_cond(self, org_cond, custom_cond, custom_uncond, bbox: CustomBBox):
        """(region prompt tensor, region negative-prompt tensor, image conditioning cut to the region) at the sampler's step."""
        icond = self.slice_icond(self.get_icond(org_cond), bbox) if isinstance(org_cond, dict) else None
        step = self.sampler.model_wrap_cfg.step
        return Condition.reconstruct_cond(custom_cond, step), Condition.reconstruct_uncond(custom_uncond, step), icond

    def _region_forward(self, forward_func, x, sigma, org_cond, tcond, icond, bbox_id, n_control):
        self.set_custom_controlnet_tensors(bbox_id, n_control)
        self.set_custom_stablesr_tensors(bbox_id)
        cond = self.make_cond_dict(org_cond, tcond, icond, self.get_vcond(org_cond)) if isinstance(org_cond, dict) else tcond
        return forward_func(x, sigma, cond=cond)

    def _split_forward(self, forward_func, x_tile, sigma_in, org_cond, first, second, icond, bbox_id, tail_repeats_second=False):
        """Two model calls for prompt tensors of different token length (they cannot be concatenated); rows beyond the two chunks
        (edit models: a second uncond copy) reuse the second result."""
        n1, n2 = first.shape[0], second.shape[0]
        x_out = torch.zeros_like(x_tile)
        ic1 = icond[:n1] if icond is not None and icond.shape[0] >= n1 + n2 else icond
        ic2 = icond[n1:n1 + n2] if icond is not None and icond.shape[0] >= n1 + n2 else icond
        x_out[:n1] = self._region_forward(forward_func, x_tile[:n1], sigma_in[:n1], org_cond, first, ic1, bbox_id, n1)
        out2 = self._region_forward(forward_func, x_tile[n1:n1 + n2], sigma_in[n1:n1 + n2], org_cond, second, ic2, bbox_id, n2)
        x_out[n1:n1 + n2] = out2
        if tail_repeats_second and x_tile.shape[0] > n1 + n2:
            x_out[n1 + n2:] = out2
        return x_out

    def kdiff_custom_forward(self, x_tile: Tensor, sigma_in: Tensor, original_cond, bbox_id: int, bbox: CustomBBox,
                             forward_func):
        """One region evaluated with its own prompt under a k-diffusion sampler.  The host's CFG denoiser feeds either the whole
        [cond, uncond(, uncond)] batch at once or slices of it (batch_cond_uncond off, --lowvram / --medvram, prompts of different
        token length); the region's tensors are sliced the same way (upstream :246-427)."""
        step = self.sampler.model_wrap_cfg.step
        if self.kdiff_step != step:               # first region call of a sampler step: forget the per-step progress
            self.kdiff_step = step
            self.kdiff_step_bbox = [-1] * len(self.custom_bboxes)
            self.tensor, self.uncond, self.image_cond_in = {}, {}, {}
            # the GLOBAL prompts only tell how the host batches this step
            self.real_tensor = Condition.reconstruct_cond(self.cond_basis, step)
            self.real_uncond = Condition.reconstruct_uncond(self.uncond_basis, step)
            self.a = [0] * len(self.custom_bboxes)
        same_len_global = self.real_tensor.shape[1] == self.real_uncond.shape[1]
        edit = bool(getattr(self, "is_edit_model", False))

        if self.kdiff_step_bbox[bbox_id] != step:
            self.kdiff_step_bbox[bbox_id] = step
            tensor, uncond, icond = self.reconstruct_custom_cond(original_cond, bbox.cond, bbox.uncond, bbox)
            if same_len_global and shared.batch_cond_uncond:
                # the whole batch is in x_tile
                if tensor.shape[1] == uncond.shape[1]:
                    cond = torch.cat([tensor, uncond, uncond] if edit else [tensor, uncond])
                    return self._region_forward(forward_func, x_tile, sigma_in, original_cond, cond, icond, bbox_id, x_tile.shape[0])
                return self._split_forward(forward_func, x_tile, sigma_in, original_cond, tensor, uncond, icond, bbox_id, tail_repeats_second=edit)
            self.tensor[bbox_id], self.uncond[bbox_id], self.image_cond_in[bbox_id] = tensor, uncond, icond

        # partial batches: rows [a, b) of the virtual [tensor, uncond(, uncond)] stack
        tensor, uncond, icond = self.tensor[bbox_id], self.uncond[bbox_id], self.image_cond_in[bbox_id]
        a = self.a[bbox_id]
        b = a + x_tile.shape[0]
        self.a[bbox_id] = b
        nt, nu = tensor.shape[0], uncond.shape[0]
        if same_len_global:
            # segments of the stack covered by [a, b): (source, lo, hi)
            stack = [(tensor, 0, nt), (uncond, nt, nt + nu)] + ([(uncond, nt + nu, nt + 2 * nu)] if edit else [])
            parts = [src[max(a, lo) - lo:min(b, hi) - lo] for src, lo, hi in stack if max(a, lo) < min(b, hi)]
            if len(parts) == 1 or all(p_.shape[1] == parts[0].shape[1] for p_ in parts):
                cond = parts[0] if len(parts) == 1 else torch.cat(parts)
                return self._region_forward(forward_func, x_tile, sigma_in, original_cond, cond, icond, bbox_id, x_tile.shape[0])
            first, second = parts[0], torch.cat(parts[1:])
            return self._split_forward(forward_func, x_tile, sigma_in, original_cond, first, second, icond, bbox_id)
        # global prompts of different length: the host runs cond and uncond in separate calls, so do the regions
        if a < nt:
            cond = tensor[a:b] if not edit else torch.cat([tensor[a:b], uncond])
            return self._region_forward(forward_func, x_tile, sigma_in, original_cond, cond, icond, bbox_id, x_tile.shape[0])
        return self._region_forward(forward_func, x_tile, sigma_in, original_cond, uncond, icond, bbox_id, uncond.shape[0])

    def ddim_custom_forward(self, x: Tensor, cond_in, bbox: CustomBBox, ts: Tensor, forward_func, *args, **kwargs):
        """One region under a CompVis (DDIM / PLMS) sampler: cond and uncond travel as two arguments and are concatenated later,
        so the negative prompt is padded with its last token vector / truncated to the prompt's length (upstream :429-451)."""
        tcond, uncond, icond = self.reconstruct_custom_cond(cond_in, bbox.cond, bbox.uncond, bbox)
        if uncond.shape[1] < tcond.shape[1]:
            uncond = torch.hstack([uncond, uncond[:, -1:].repeat([1, tcond.shape[1] - uncond.shape[1], 1])])
        elif uncond.shape[1] > tcond.shape[1]:
            uncond = uncond[:, :tcond.shape[1]]
        if icond is not None:
            cond, uc = self.make_cond_dict(cond_in, tcond, icond), self.make_cond_dict(cond_in, uncond, icond)
        else:
            cond, uc = tcond, uncond
        return forward_func(x, cond, ts, unconditional_conditioning=uc, *args, **kwargs)

    # ---- ControlNet (upstream :454-544) ---------------------------------------------------------------------------------
    # Upstream crops every hint into per-batch tile stacks at init (optionally parked on the CPU) and re-assembles / repeats /
    # uploads them at every model call.  Here the full hints stay where they are and one mdtile_gather_rects launch per hint
    # produces the sliced + repeated tensor when a batch is switched in -- nothing is cached.
    def init_controlnet(self, controlnet_script, control_tensor_cpu: bool):
        self.enable_controlnet = True
        self.controlnet_script = controlnet_script
        self.control_tensor_cpu = control_tensor_cpu      # accepted for the UI's sake: there are no tile caches to park
        self.control_params = None
        self.org_control_tensor_batch = None
        self.prepare_controlnet_tensors()

    def reset_controlnet_tensors(self):
        if not self.enable_controlnet or self.org_control_tensor_batch is None:
            return
        for param, hint in zip(self.control_params, self.org_control_tensor_batch):
            param.hint_cond = hint

    def prepare_controlnet_tensors(self, refresh: bool = False):
        """Remember the network's control params and their ORIGINAL hints (full canvas, opt_f x the latent grid)."""
        if not refresh and self.control_params is not None:
            return
        if not self.enable_controlnet or self.controlnet_script is None:
            return
        net = getattr(self.controlnet_script, "latest_network", None)
        if net is None or not hasattr(net, "control_params"):
            return
        self.control_params = net.control_params
        hints = []
        for param in self.control_params:
            h = param.hint_cond
            hints.append(h.unsqueeze(0) if h.dim() == 3 else h)
        self.org_control_tensor_batch = hints

    def _hint_on_device(self, hint: Tensor) -> Tensor:
        return hint if hint.device.type == "cuda" else hint.to(devices.device)

    def switch_controlnet_tensors(self, batch_id: int, x_batch_size: int, tile_batch_size: int, is_denoise: bool = False,
                                  batched_bboxes: Optional[List[List[BBox]]] = None):
        """batched_bboxes: the box list whose batch `batch_id` is switched in (default: the grid's; with tile skipping the active batches)."""
        if not self.enable_controlnet or not self.org_control_tensor_batch:
            return
        bboxes = (self.batched_bboxes if batched_bboxes is None else batched_bboxes)[batch_id]
        rects = [(b.x * opt_f, b.y * opt_f) for b in bboxes]
        w, h = bboxes[0].w * opt_f, bboxes[0].h * opt_f
        for k, (param, hint) in enumerate(zip(self.control_params, self.org_control_tensor_batch)):
            hint = self._hint_on_device(self.extended_x(hint, f"hint{k}", opt_f)).contiguous()
            if self.is_kdiff:      # every tile's x_batch_size copies are consecutive (tile-major model batch)
                param.hint_cond = mdtile.gather_rects(hint[:1], rects[:tile_batch_size], w, h, repeat=x_batch_size, tile_major=True)
            else:                  # DDIM: the tile stack as a whole, repeated for cond + uncond (once when only denoising)
                param.hint_cond = mdtile.gather_rects(hint, rects, w, h, repeat=x_batch_size if is_denoise else x_batch_size * 2, tile_major=False)

    def set_custom_controlnet_tensors(self, bbox_id: int, repeat_size: int):
        if not self.enable_controlnet or not self.org_control_tensor_batch or not self.custom_bboxes:
            return
        bbox = self.custom_bboxes[bbox_id]
        for k, (param, hint) in enumerate(zip(self.control_params, self.org_control_tensor_batch)):
            hint = self._hint_on_device(self.extended_x(hint, f"hint{k}", opt_f)).contiguous()      # a region that crosses a seam is contiguous in the copy
            param.hint_cond = mdtile.gather_rects(hint, [(bbox.x * opt_f, bbox.y * opt_f)], bbox.w * opt_f, bbox.h * opt_f,
                                                  repeat=repeat_size, tile_major=False)

    # ---- StableSR (upstream :547-588) --------------------------------------------------------------------------------------
    def init_stablesr(self, stablesr_script):
        if stablesr_script.stablesr_model is None:
            return
        self.stablesr_script = stablesr_script

        def set_image_hook(latent_image: Tensor):
            self.enable_stablesr = True
            self.stablesr_tensor = latent_image

        stablesr_script.stablesr_model.set_image_hooks["TiledDiffusion"] = set_image_hook

    def _stablesr_live(self) -> bool:
        return self.enable_stablesr and self.stablesr_script is not None and self.stablesr_script.stablesr_model is not None \
            and self.stablesr_tensor is not None

    def reset_stablesr_tensors(self):
        if self._stablesr_live():
            self.stablesr_script.stablesr_model.latent_image = self.stablesr_tensor

    def switch_stablesr_tensors(self, batch_id: int, batched_bboxes: Optional[List[List[BBox]]] = None):
        if not self._stablesr_live():
            return
        bboxes = (self.batched_bboxes if batched_bboxes is None else batched_bboxes)[batch_id]
        t = self.extended_x(self.stablesr_tensor, "stablesr").contiguous()
        self.stablesr_script.stablesr_model.latent_image = mdtile.gather_rects(t, [(b.x, b.y) for b in bboxes], bboxes[0].w, bboxes[0].h)

    def set_custom_stablesr_tensors(self, bbox_id: int):
        if not self._stablesr_live() or not self.custom_bboxes:
            return
        bbox = self.custom_bboxes[bbox_id]
        t = self.extended_x(self.stablesr_tensor, "stablesr").contiguous()
        self.stablesr_script.stablesr_model.latent_image = mdtile.gather_rect(t, bbox.x, bbox.y, bbox.w, bbox.h)

    # ---- Noise Inversion (upstream :591-747) -----------------------------------------------------------------------------
    def init_noise_inverse(self, steps: int, retouch: float, get_cache_callback, set_cache_callback, renoise_strength: float,
                           renoise_kernel: int):
        self.noise_inverse_enabled = True
        self.noise_inverse_steps = steps
        self.noise_inverse_retouch = float(retouch)
        self.noise_inverse_renoise_strength = float(renoise_strength)
        self.noise_inverse_renoise_kernel = int(renoise_kernel)
        if self.sample_img2img_original is None:
            self.sample_img2img_original = self.sampler_raw.sample_img2img
        self.sampler_raw.sample_img2img = MethodType(self.sample_img2img, self.sampler_raw)
        self.noise_inverse_set_cache = set_cache_callback
        self.noise_inverse_get_cache = get_cache_callback

    def renoise_mask(self, p, size) -> Optional[Tensor]:
        """[H, W] weight of fresh noise: where the guided filter says the input image has detail, scaled by the renoise strength
        (upstream :607-621).  An RGB init image goes up as its interleaved bytes and is made grey on the GPU; any other mode is converted
        on the host first; an image the script has just upscaled on the engine is still on the device and is not uploaded again.  Filter and
        resize both run on the engine (mdtile_retouch_mask, mdtile_renoise_resize)."""
        if self.noise_inverse_renoise_strength <= 0:
            return None
        import numpy as np
        img = p.init_images[0]
        kept = getattr(p, "init_image_bytes_md", None)      # (image, its bytes on the device) left by the script's upscale
        if kept is not None and kept[0] is img:
            pixels = kept[1]
        else:
            pixels = np.asarray(img if img.mode == "RGB" else img.convert("L"))
        m = get_retouch_mask(pixels, self.noise_inverse_renoise_kernel)     # module attribute, looked up per call (tests replace it)
        m = torch.as_tensor(m).to(devices.device, torch.float32).contiguous()
        return mdtile.renoise_resize(m, size, self.noise_inverse_renoise_strength)

    def _cached_inversion(self, p, prompts) -> Optional[Tensor]:
        c = self.noise_inverse_get_cache()
        if c is None:
            return None
        same = (c.model_hash == p.sd_model.sd_model_hash and c.noise_inversion_steps == self.noise_inverse_steps
                and len(c.prompts) == len(prompts) and all(a == b for a, b in zip(c.prompts, prompts))
                and abs(c.retouch - self.noise_inverse_retouch) < 0.01 and c.x0.shape == p.init_latent.shape
                and torch.abs(c.x0.to(p.init_latent.device) - p.init_latent).sum() < 100)
        return c.xt if same else None

    def sample_img2img(self, sampler, p, x: Tensor, noise: Tensor, conditioning, unconditional_conditioning, steps=None,
                       image_conditioning=None):
        """Replacement of the sampler's sample_img2img: the img2img start noise is the noise that INVERTS the init image
        (tiled Euler inversion through get_noise), mixed with fresh noise where the image has detail (upstream :606-681)."""
        from modules import sd_samplers_common
        renoise_mask = self.renoise_mask(p, tuple(noise.shape[-2:]))
        prompts = p.all_prompts[:p.batch_size]
        latent = self._cached_inversion(p, prompts)
        if latent is not None:
            print("[Tiled Diffusion] checkpoint, image, prompts, inversion steps and retouch are unchanged: "
                  "Noise Inversion reuses the latent of the previous run.")
            latent = latent.to(noise.device)
        else:
            shared.state.job_count += 1
            latent = self.find_noise_for_image_sigma_adjustment(sampler.model_wrap, self.noise_inverse_steps, prompts)
            shared.state.nextjob()
            self.noise_inverse_set_cache(p.init_latent.clone().cpu(), latent.clone().cpu(), prompts)
        adjusted_steps, _ = sd_samplers_common.setup_img2img_steps(p, steps)
        sigmas = sampler.get_sigmas(p, adjusted_steps)
        inverse_noise = latent - (p.init_latent / sigmas[0])
        if renoise_mask is not None:
            # :655-676 -- one engine launch.  With the grid disabled the job's noise is first re-weighted by the regions.
            regions = []
            if not self.enable_grid_bbox:
                for b in self.custom_bboxes:
                    fg = b.blend_mode == BlendMode.FOREGROUND
                    regions.append((b.x, b.y, b.w, b.h, mdtile.REGION_FG if fg else mdtile.REGION_BG,
                                    b.feather_mask.to(device=noise.device, dtype=torch.float32).contiguous() if fg else None))
            combined = mdtile.noise_inverse_blend(noise.float().contiguous(), inverse_noise.float().contiguous(),
                                                  renoise_mask.float().contiguous(), regions).to(noise.dtype)
        else:
            combined = inverse_noise
        return self.sample_img2img_original(p, x, combined, conditioning, unconditional_conditioning, steps, image_conditioning)

    @torch.no_grad()
    def find_noise_for_image_sigma_adjustment(self, dnw, steps: int, prompts: List[str]) -> Tensor:
        """Euler inversion of the init latent over `steps` sigmas, every model call tiled through get_noise (upstream :683-743,
        after the host's img2imgalt script)."""
        import k_diffusion as K
        from modules import sd_samplers_common
        assert self.p.sampler_name == "Euler"
        x = self.p.init_latent
        s_in = x.new_ones([x.shape[0]])
        skip = 1 if shared.sd_model.parameterization == "v" else 0
        sigmas = dnw.get_sigmas(steps).flip(0)
        cond = self.p.sd_model.get_learned_conditioning(prompts)
        if isinstance(cond, Tensor):     # SD1 / SD2
            cond_in = self.make_cond_dict({"c_crossattn": [], "c_concat": []}, cond, self.p.image_conditioning)
        else:                            # SDXL
            cond_in = self.make_cond_dict({"crossattn": None, "vector": None, "c_concat": []}, cond["crossattn"],
                                          self.p.image_conditioning, cond["vector"])
        state.sampling_steps = steps
        try:
            from tqdm import tqdm
            bar = tqdm(total=steps, desc="Noise Inversion")
        except Exception:  # pragma: no cover
            bar = None
        for i in range(1, len(sigmas)):
            if state.interrupted:
                return x
            state.sampling_step += 1
            sigma_in = torch.cat([sigmas[i] * s_in])
            c_out, c_in = [K.utils.append_dims(k, x.ndim) for k in dnw.get_scalings(sigma_in)[skip:]]
            t = dnw.sigma_to_t(sigma_in) / self.noise_inverse_retouch
            eps = self.get_noise(x * c_in, t, cond_in, steps - i)
            denoised = x + eps * c_out
            d = (x - denoised) / sigmas[i]            # Euler step towards the next (larger) sigma
            x = x + d * (sigmas[i] - sigmas[i - 1])
            sd_samplers_common.store_latent(x)
            del sigma_in, c_out, c_in, t, eps, denoised, d
            if bar is not None:
                bar.update(1)
        if bar is not None:
            bar.close()
        return x / sigmas[-1]

    def get_noise(self, x_in: Tensor, sigma_in: Tensor, cond_in, step: int) -> Tensor:
        raise NotImplementedError
