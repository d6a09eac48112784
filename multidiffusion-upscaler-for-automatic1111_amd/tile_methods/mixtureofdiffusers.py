"""
Mixture-of-Diffusers delegate (https://github.com/albarji/mixture-of-diffusers) on the mdtile engine.

Same hijack surface as upstream tile_methods/mixtureofdiffusers.py: `shared.sd_model.apply_model` is replaced by
`apply_model_hijack`, which blends per-tile eps predictions with Gaussian tile weights that were pre-normalised by the
weight-sum map (`rescale_factor = 1 / weights`, upstream :29-36).  The per-tile `w = tile_weights * rescale[slicer]`,
`x_buffer[slicer] += out * w` loop (:122-126), Gaussian background regions (:152-153) and the feather composite
(:154-175) run as ONE mdtile_blend launch; there is no final division (:177-179).
"""
from __future__ import annotations

from typing import List, Optional

import torch
from torch import Tensor

from modules import devices, extra_networks, shared
from modules.shared import state

import mdtile
from tile_methods.abstractdiffusion import AbstractDiffusion
from tile_utils.utils import BlendMode, Condition, gaussian_weights


class MixtureOfDiffusers(AbstractDiffusion):

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.custom_weights: List[Optional[Tensor]] = []   # per region: Gaussian [1,1,h,w] (background) or None
        self.raw_custom_weights: List[Optional[Tensor]] = []   # --mdtile-jitter-regions: the same Gaussians, never premultiplied (the lattice path)
        self.get_weight = gaussian_weights
        self.rescale_factor: Optional[Tensor] = None

    # ---- hijack ---------------------------------------------------------------------------------------------------
    def hook(self):
        if not hasattr(shared.sd_model, "apply_model_original_md"):
            shared.sd_model.apply_model_original_md = shared.sd_model.apply_model
        shared.sd_model.apply_model = self.apply_model_hijack

    @staticmethod
    def unhook():
        if hasattr(shared.sd_model, "apply_model_original_md"):
            shared.sd_model.apply_model = shared.sd_model.apply_model_original_md
            del shared.sd_model.apply_model_original_md

    # ---- weights --------------------------------------------------------------------------------------------------
    def get_tile_weights(self) -> Tensor:
        if not hasattr(self, "tile_weights"):
            self.tile_weights = self.get_weight(self.tile_w, self.tile_h)
        return self.tile_weights

    def init_custom_bbox(self, *args):
        super().init_custom_bbox(*args)
        for bbox in self.custom_bboxes:
            if bbox.blend_mode == BlendMode.BACKGROUND:
                cw = self.get_weight(bbox.w, bbox.h)
                if bbox.cover is not None:
                    # a mask region counts where it covers: Gaussian * cover (exact: * 0.0 or * 1.0).  init_done multiplies it by the reciprocal map,
                    # which may be inf under a pixel nobody paints: 0 * inf = NaN there -- at a pixel the region does not cover, which the masked
                    # blend never reads
                    cw = cw * bbox.cover.to(torch.float32)
                self.add_region_weight(bbox, cw)
                self.custom_weights.append(cw.unsqueeze(0).unsqueeze(0))
                self.raw_custom_weights.append(cw.clone().unsqueeze(0).unsqueeze(0) if self.jitter_regions else None)
            else:
                self.custom_weights.append(None)
                self.raw_custom_weights.append(None)

    def init_done(self):
        super().init_done()
        # Gaussian weights can be ~1e-10: normalise up front (inf where nothing is painted, exactly as upstream)
        self.rescale_factor = mdtile.reciprocal(self.weights)
        if self.wrap_regions:      # the weight sum changes with the grid's shift: the region weights stay raw, the blend divides per pixel
            return
        for bbox_id, bbox in enumerate(self.custom_bboxes):
            if bbox.blend_mode == BlendMode.BACKGROUND:
                mdtile.rect_mul_canvas(self.custom_weights[bbox_id], self.rescale_factor, bbox.x, bbox.y, bbox.w, bbox.h)

    def region_weights(self, raw: bool = False):
        """raw: the Gaussians as they were made, for the lattice path (--mdtile-jitter-regions); else premultiplied by rescale_factor (init_done)."""
        bg = self.raw_custom_weights if raw else self.custom_weights
        return [b.feather_mask if b.blend_mode == BlendMode.FOREGROUND else bg[i] for i, b in enumerate(self.custom_bboxes)]

    # ---- the hot path ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def apply_model_hijack(self, x_in: Tensor, t_in: Tensor, cond, noise_inverse_step: int = -1):
        c_in = cond
        N, C, H, W = x_in.shape
        if (H, W) != (self.h, self.w):
            self.reset_controlnet_tensors()
            return shared.sd_model.apply_model_original_md(x_in, t_in, c_in)
        x_in = x_in.contiguous()

        # --mdtile-inpaint-skip: only the tiles the job's mask touches run (the sparse plan); the host discards the result everywhere else
        skip = self.inpaint_skip(self.NOISE_INVERSION_FULL if noise_inverse_step >= 0 else None)
        # --mdtile-grid-jitter (plain grids only, never with the sparse plan; with regions only under --mdtile-jitter-regions): this step's lattice
        # and its pushed-in boxes, or None
        jitter = self.step_lattice(self.NOISE_INVERSION_UNJITTERED if noise_inverse_step >= 0 else None, skip)
        if skip == "empty":
            return x_in.clone()      # a fresh tensor, as every other path returns: the caller may work on the result in place
        plan, batched_bboxes = (self.sparse_plan, self.sparse_batched_bboxes) if skip == "sparse" else (self.plan, self.batched_bboxes)
        # --mdtile-grid-shift (wrap-around plans only, so never with the sparse plan; with regions only under --mdtile-wrap-regions): this
        # step's displacement and its boxes
        sx = sy = 0
        if self.grid_shift:
            (sx, sy), batched_bboxes = self.step_shift(self.NOISE_INVERSION_UNSHIFTED if noise_inverse_step >= 0 else None)
        if jitter is not None:
            lattice, batched_bboxes = jitter
            if batched_bboxes is None:      # --mdtile-jitter-inpaint-skip: the mask touches no tile of this step's grid
                return x_in.clone()
        # --mdtile-jitter-inpaint-skip: the step's active tiles only, in compact batches (step_lattice hands the full lattice where all are active)
        lattice_subset = jitter is not None and isinstance(lattice, mdtile.LatticeSubset)

        tile_outs: List[Tensor] = []
        if self.draw_background:
            # K2, one launch
            if lattice_subset:
                x_tiles = mdtile.gather_all_lattice_sparse(lattice, x_in)
            elif jitter is not None:
                x_tiles = mdtile.gather_all_lattice(lattice, x_in)
            else:
                x_tiles = mdtile.gather_all_shift(plan, x_in, sx, sy) if self.grid_shift else mdtile.gather_all(plan, x_in)
            for batch_id, bboxes in enumerate(batched_bboxes):
                if state.interrupted:
                    return x_in
                n = len(bboxes)
                t_tile = torch.cat([t_in] * n, dim=0)
                if isinstance(c_in, dict):
                    tcond = torch.cat([self.get_tcond(c_in)] * n, dim=0)
                    icond = torch.cat([self.slice_icond(self.get_icond(c_in), b) for b in bboxes], dim=0)
                    vc = self.get_vcond(c_in)
                    vcond = torch.cat([vc] * n, dim=0) if vc is not None else None
                    c_tile = self.make_cond_dict(c_in, tcond, icond, vcond)
                else:
                    print(">> [WARN] not supported, make an issue on github!!")
                    c_tile = c_in
                self.switch_controlnet_tensors(batch_id, N, n, is_denoise=True, batched_bboxes=batched_bboxes)
                self.switch_stablesr_tensors(batch_id, batched_bboxes)
                out = shared.sd_model.apply_model_original_md(x_tiles[batch_id], t_tile, c_tile)
                tile_outs.append(out.to(x_in.dtype).contiguous())
                self.update_pbar()

        region_outs: List[Tensor] = []
        for bbox_id, bbox in enumerate(self.custom_bboxes):
            if not self.p.disable_extra_networks:
                with devices.autocast():
                    extra_networks.activate(self.p, bbox.extra_network_data)
            x_tile = self.gather_region(x_in, bbox)
            if noise_inverse_step < 0:
                out = self.custom_apply_model(x_tile, t_in, c_in, bbox_id, bbox)
            else:
                tcond = Condition.reconstruct_cond(bbox.cond, noise_inverse_step)
                icond = self.slice_icond(self.get_icond(c_in), bbox)
                c_out = self.make_cond_dict(c_in, tcond, icond, self.get_vcond(c_in))
                out = shared.sd_model.apply_model(x_tile, t_in, cond=c_out)
            region_outs.append(out.to(x_in.dtype).contiguous())
            self.update_pbar()
            if not self.p.disable_extra_networks:
                with devices.autocast():
                    extra_networks.deactivate(self.p, bbox.extra_network_data)

        if skip == "sparse":      # live pixels as the full blend has them, x_in everywhere else (no regions on this path)
            self.x_buffer = mdtile.blend_sparse(plan, mdtile.METHOD_MOD, tile_outs, N, C, fill=x_in, tile_w=self.get_tile_weights(),
                                                rescale=self.rescale_factor)
            return self.x_buffer
        if jitter is not None:    # every tile where its lattice box lies, the Gaussian in lattice coordinates; the step's sum and reciprocal in the kernel
            if lattice_subset:           # live pixels as the full lattice blend has them, x_in everywhere else (no regions on this path)
                self.x_buffer = mdtile.blend_lattice_sparse(lattice, mdtile.METHOD_MOD, tile_outs, N, C, fill=x_in, tile_w=self.get_tile_weights())
            elif self.jitter_regions:    # then the regions, where they are, their Gaussians raw: only the grid moves
                self.x_buffer = self.blend_lattice_regions(mdtile.METHOD_MOD, lattice, tile_outs, region_outs, x_in)
            else:
                self.x_buffer = mdtile.blend_lattice(lattice, mdtile.METHOD_MOD, tile_outs, N, C, tile_w=self.get_tile_weights())
            return self.x_buffer
        if self.wrap_regions:     # the grid where this step's shift puts it, then the regions where they lie on the closed canvas
            self.x_buffer = self.blend_wrap_regions(mdtile.METHOD_MOD, tile_outs, region_outs, x_in, (sx, sy))
            return self.x_buffer
        if self.grid_shift:       # the blend of the plan, stored (sy, sx) further on the circle
            self.x_buffer = mdtile.blend_shift(plan, mdtile.METHOD_MOD, tile_outs, N, C, sx=sx, sy=sy, tile_w=self.get_tile_weights(),
                                               rescale=self.rescale_factor)
            return self.x_buffer
        if self.mask_regions:     # a region enters a pixel only where its mask covers it; every other region is its whole rectangle
            self.x_buffer = mdtile.blend_mask_regions(self.blend_plan(), mdtile.METHOD_MOD, tile_outs, N, C,
                                                      tile_w=self.get_tile_weights() if tile_outs else None, rescale=self.rescale_factor,
                                                      regions=self.region_specs(region_outs), dtype=x_in.dtype, device=x_in.device)
            return self.x_buffer
        # K4 + K6 + K7 in one launch; pixels nobody paints stay 0, as upstream
        self.x_buffer = mdtile.blend(self.blend_plan(), mdtile.METHOD_MOD, tile_outs, N, C, tile_w=self.get_tile_weights() if tile_outs else None,
                                     rescale=self.rescale_factor, regions=self.region_specs(region_outs),
                                     dtype=x_in.dtype, device=x_in.device)
        return self.x_buffer

    def custom_apply_model(self, x_in, t_in, c_in, bbox_id, bbox) -> Tensor:
        if self.is_kdiff:
            return self.kdiff_custom_forward(x_in, t_in, c_in, bbox_id, bbox,
                                             forward_func=shared.sd_model.apply_model_original_md)

        def forward_func(x, c, ts, unconditional_conditioning, *args, **kwargs) -> Tensor:
            merged = {}
            for key in c:   # cond + uncond batched the way p_sample_ddim does
                if isinstance(c[key], list):
                    merged[key] = [torch.cat([unconditional_conditioning[key][i], c[key][i]]) for i in range(len(c[key]))]
                else:
                    merged[key] = torch.cat([unconditional_conditioning[key], c[key]])
            return shared.sd_model.apply_model_original_md(x, ts, merged)

        return self.ddim_custom_forward(x_in, c_in, bbox, ts=t_in, forward_func=forward_func)

    @torch.no_grad()
    def get_noise(self, x_in: Tensor, sigma_in: Tensor, cond_in, step: int) -> Tensor:
        return self.apply_model_hijack(x_in, sigma_in, cond=cond_in, noise_inverse_step=step)
