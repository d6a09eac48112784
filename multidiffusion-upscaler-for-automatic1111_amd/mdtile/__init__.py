"""
mdtile -- ctypes binding of libmdtile.so (include/mdtile.h) for the PyTorch-ROCm host.

PyTorch is plumbing here: it owns device memory and the HIP stream; every hot-path computation happens in the
hand-written gfx950 kernels behind the C ABI.  There is NO CPU / eager-torch fallback: if the shared library is
missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_size_t, c_void_p
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmdtile.so")

OK, E_ARG, E_HIP, E_LIMIT = 0, -1, -2, -3
DT_F32, DT_F16, DT_BF16 = 0, 1, 2
METHOD_MD, METHOD_MOD = 0, 1
REGION_BG, REGION_FG = 0, 1
RESAMPLE_NEAREST, RESAMPLE_LANCZOS = 0, 1
BLEND_PARTIAL, BLEND_TILE_RANGE, BLEND_PACKED = 1, 2, 4
BLEND_KERNEL_PLAIN, BLEND_KERNEL_LDS = 0, 1
CONV_UPSAMPLE2X = 1
CONV_REC_ONE_BLOCK, CONV_REC_TWO_BLOCKS = 4, 8      # call_rec(family=...): name the record-conv kernel family (tests / probes); 0 = per launch
CONV_EXACT_F32 = 2
CONV_REC_X_F16, CONV_REC_Y_F16 = 32, 64      # PRECISION_F16: the input record / the record output of a record conv is the fp16 form (RecImage.fmt)
CONV_W_F16, CONV_ATTN_PROJ = 128, 256        # PRECISION_F16: the hand-over conv gets the fp16 weight plane; a 1x1 conv is q / k / v / proj_out of the attention
REC_BF16X2, REC_F16 = 0, 1                   # RecImage.fmt: bf16 (hi, lo) split | fp16 in the hi half (activated records written in PRECISION_F16)
ATTN_EXACT_F32 = 1
ATTN_V_CHANNEL_MAJOR = 2
MAX_BATCHES, MAX_REGIONS = 320, 16
VAE_ASSEMBLE_CHUNK = 32
VAE_BLEND_CHUNK = 16
MASK_ACTIVITY_MAX_BOXES = 4096
VAE_SPARSE_MAX_BOXES = 4096
VAE_FILL_CHUNK = 128

_DTYPES = {torch.float32: DT_F32, torch.float16: DT_F16, torch.bfloat16: DT_BF16}


class MdtileError(RuntimeError):
    pass


class _Region(ctypes.Structure):
    _fields_ = [("x", c_int), ("y", c_int), ("w", c_int), ("h", c_int), ("mode", c_int), ("_pad", c_int),
                ("out", c_void_p), ("weight", c_void_p)]


class _MaskRegion(ctypes.Structure):
    _fields_ = [("r", _Region), ("cover", c_void_p)]


class _P2P(ctypes.Structure):
    _fields_ = [("peer", c_int), ("send", c_void_p), ("send_bytes", c_size_t), ("recv", c_void_p), ("recv_bytes", c_size_t)]


class _VaeTile(ctypes.Structure):
    _fields_ = [("tile", c_void_p), ("th", c_int), ("tw", c_int), ("in_bbox4", c_int * 4), ("out_bbox4", c_int * 4)]


class _BlendArgs(ctypes.Structure):
    _fields_ = [("method", c_int), ("dtype", c_int), ("N", c_int), ("C", c_int), ("flags", c_int),
                ("tile_lo", c_int), ("tile_hi", c_int), ("row_lo", c_int), ("row_hi", c_int),
                ("d_weights", c_void_p), ("d_tile_w", c_void_p), ("d_rescale", c_void_p), ("d_x_out", c_void_p)]


class _WrapRegions(ctypes.Structure):
    _fields_ = [("regions", POINTER(_Region)), ("num_regions", c_int), ("d_grid_w", c_void_p), ("d_region_w", c_void_p), ("sx", c_int), ("sy", c_int)]


class _Lattice(ctypes.Structure):
    _fields_ = [(n, c_int) for n in ("w", "h", "tile_w", "tile_h", "overlap", "stride_x", "stride_y", "sx", "sy", "cols", "rows", "num_tiles",
                                     "num_batches", "tile_bs")]


class _LatticeRegions(ctypes.Structure):
    _fields_ = [("regions", POINTER(_Region)), ("num_regions", c_int), ("d_region_w", c_void_p)]


class _LatticeSubset(ctypes.Structure):
    _fields_ = [("lat", _Lattice), ("num_active", c_int), ("num_batches", c_int), ("tile_bs", c_int), ("d_slot", c_void_p)]


# every symbol include/mdtile.h declares: name -> (restype, argtypes)
_IP = POINTER(c_int)
_SIGNATURES = {
    "mdtile_version": (c_int, []),
    "mdtile_last_error": (c_char_p, []),
    "mdtile_set_precision": (c_int, [c_int]),
    "mdtile_get_precision": (c_int, []),
    "mdtile_plan_create": (c_void_p, [c_int] * 7),
    "mdtile_plan_create_wrap_x": (c_void_p, [c_int] * 6),
    "mdtile_plan_wrap_x": (c_int, [c_void_p]),
    "mdtile_plan_create_wrap": (c_void_p, [c_int] * 8),
    "mdtile_plan_wrap_y": (c_int, [c_void_p]),
    "mdtile_plan_destroy": (None, [c_void_p]),
    "mdtile_plan_info": (c_int, [c_void_p, _IP]),
    "mdtile_plan_bboxes": (c_int, [c_void_p, _IP]),
    "mdtile_gaussian_weights": (c_int, [c_int, c_int, c_void_p, c_void_p]),
    "mdtile_feather_mask": (c_int, [c_int, c_int, c_double, c_void_p, c_void_p]),
    "mdtile_weight_map_add_grid": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "mdtile_weight_map_add_rect": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_float, c_void_p]),
    "mdtile_reciprocal": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mdtile_rect_mul_canvas": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mdtile_gather": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "mdtile_gather_all": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, POINTER(c_void_p), c_int, c_void_p]),
    "mdtile_gather_all_shift": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, POINTER(c_void_p), c_int, c_int, c_int, c_void_p]),
    "mdtile_gather_range": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "mdtile_gather_rect": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "mdtile_stream_copy": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mdtile_blend": (c_int, [c_void_p, POINTER(_BlendArgs), POINTER(c_void_p), c_int, POINTER(_Region), c_int, c_void_p]),
    "mdtile_blend_shift": (c_int, [c_void_p, POINTER(_BlendArgs), POINTER(c_void_p), c_int, c_int, c_int, c_void_p]),
    "mdtile_blend_dispatch": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _IP]),
    "mdtile_blend_finalize": (c_int, [c_void_p, POINTER(_BlendArgs), c_void_p, POINTER(_Region), c_int, c_void_p]),
    "mdtile_gather_rect_wrap": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "mdtile_weight_map_add_rect_wrap": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_float, c_int, c_int, c_void_p]),
    "mdtile_region_noise_wrap": (c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(_Region), c_int, c_int, c_int, c_void_p]),
    "mdtile_blend_wrap_regions": (c_int, [c_void_p, POINTER(_BlendArgs), POINTER(c_void_p), c_int, POINTER(_WrapRegions), c_void_p]),
    "mdtile_tile_activity": (c_int, [c_void_p, c_void_p, c_int, c_void_p, c_void_p]),
    "mdtile_plan_create_subset": (c_void_p, [c_void_p, _IP, c_int]),
    "mdtile_plan_active": (c_int, [c_void_p, _IP]),
    "mdtile_blend_sparse": (c_int, [c_void_p, POINTER(_BlendArgs), POINTER(c_void_p), c_int, c_void_p, c_void_p]),
    "mdtile_lattice_make": (c_int, [c_int] * 8 + [POINTER(_Lattice)]),
    "mdtile_lattice_bboxes": (c_int, [POINTER(_Lattice), _IP]),
    "mdtile_lattice_weight_map": (c_int, [POINTER(_Lattice), c_void_p, c_void_p, c_void_p]),
    "mdtile_gather_all_lattice": (c_int, [POINTER(_Lattice), c_int, c_int, c_int, c_void_p, POINTER(c_void_p), c_int, c_void_p]),
    "mdtile_blend_lattice": (c_int, [POINTER(_Lattice), POINTER(_BlendArgs), POINTER(c_void_p), c_int, c_void_p]),
    "mdtile_blend_lattice_regions": (c_int, [POINTER(_Lattice), POINTER(_BlendArgs), POINTER(c_void_p), c_int, POINTER(_LatticeRegions), c_void_p]),
    "mdtile_lattice_activity": (c_int, [POINTER(_Lattice), c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "mdtile_lattice_subset_make": (c_int, [POINTER(_Lattice), _IP, c_int, c_void_p, POINTER(_LatticeSubset)]),
    "mdtile_lattice_subset_bboxes": (c_int, [POINTER(_LatticeSubset), _IP, _IP, _IP]),
    "mdtile_gather_all_lattice_sparse": (c_int, [POINTER(_LatticeSubset), c_int, c_int, c_int, c_void_p, POINTER(c_void_p), c_int, c_void_p]),
    "mdtile_blend_lattice_sparse": (c_int, [POINTER(_LatticeSubset), POINTER(_BlendArgs), POINTER(c_void_p), c_int, c_void_p, c_void_p]),
    "mdtile_mask_cover_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mdtile_mask_region": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_void_p, c_void_p, c_void_p]),
    "mdtile_blend_mask_regions": (c_int, [c_void_p, POINTER(_BlendArgs), POINTER(c_void_p), c_int, POINTER(_MaskRegion), c_int, c_void_p]),
    "mdtile_region_noise_masked": (c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(_MaskRegion), c_int, c_void_p]),
    "mdtile_region_noise": (c_int, [c_void_p, c_int, c_int, c_int, c_int, POINTER(_Region), c_int, c_void_p]),
    "mdtile_noise_inverse_blend": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, POINTER(_Region), c_int, c_void_p]),
    "mdtile_retouch_mask_ws_size": (c_size_t, [c_int, c_int, c_int]),
    "mdtile_retouch_mask": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mdtile_renoise_resize": (c_int, [c_void_p, c_int, c_int, c_float, c_void_p, c_int, c_int, c_void_p]),
    "mdtile_resample_ksize": (c_int, [c_int, c_int, c_int]),
    "mdtile_resample_table": (c_int, [c_int, c_int, c_int, c_void_p, c_void_p]),
    "mdtile_resample_u8_ws_size": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "mdtile_resample_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int,
                                   c_void_p, c_void_p]),
    "mdtile_colorfix_wavelet_ws_size": (c_size_t, [c_int, c_int, c_int]),
    "mdtile_colorfix_wavelet": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "mdtile_hist_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p]),
    "mdtile_lut_u8": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mdtile_gather_rects": (c_int, [c_int, c_int, c_int, c_int, c_int, c_void_p, _IP, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "mdtile_shard_init": (c_void_p, [c_int, _IP]),
    "mdtile_shard_unique_id": (c_int, [c_void_p]),
    "mdtile_shard_init_rank": (c_void_p, [c_int, c_int, c_void_p, c_int]),
    "mdtile_shard_probe_rank": (c_int, [c_int, c_int, c_void_p, c_int, c_double]),
    "mdtile_shard_destroy": (None, [c_void_p]),
    "mdtile_shard_info": (c_int, [c_void_p, _IP]),
    "mdtile_shard_stream": (c_void_p, [c_void_p, c_int]),
    "mdtile_halo_scratch_bytes": (c_size_t, [c_int, c_int, _IP, c_int, c_int, c_int]),
    "mdtile_halo_exchange": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_int, c_int, c_int, c_int, _IP, POINTER(c_void_p)]),
    "mdtile_allreduce_stats": (c_int, [c_void_p, POINTER(c_void_p), c_int, POINTER(c_void_p)]),
    "mdtile_shard_bcast": (c_int, [c_void_p, POINTER(c_void_p), c_size_t, c_int, POINTER(c_void_p)]),
    "mdtile_shard_p2p": (c_int, [c_void_p, POINTER(POINTER(_P2P)), _IP, POINTER(c_void_p)]),
    "mdtile_shard_allgather": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p), c_size_t, POINTER(c_void_p)]),
    "mdtile_shard_selfcheck_bytes": (c_size_t, [c_void_p]),
    "mdtile_shard_selfcheck": (c_int, [c_void_p, POINTER(c_void_p), POINTER(c_void_p)]),
    "mdtile_window_blend": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mdtile_dilated_gather": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, _IP, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mdtile_demofusion_combine": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_void_p]),
    "mdtile_depthwise_blur": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "mdtile_restandardize": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mdtile_vae_split_tiles": (c_int, [c_int, c_int, c_int, c_int, _IP, _IP, c_int]),
    "mdtile_vae_best_tile_size": (c_int, [c_int, c_int]),
    "mdtile_gn_stats_ws_size": (c_size_t, [c_int, c_int]),
    "mdtile_gn_stats": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mdtile_gn_pool": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "mdtile_gn_apply": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_float, c_int, c_void_p]),
    "mdtile_silu": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mdtile_tanh": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p]),
    "mdtile_add": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "mdtile_conv_packed_size": (c_size_t, [c_int, c_int, c_int]),
    "mdtile_conv_pack": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mdtile_conv_pack_f16_size": (c_size_t, [c_int, c_int, c_int]),
    "mdtile_conv_pack_f16": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "mdtile_conv2d": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int,
                              c_int, c_int, c_void_p]),
    "mdtile_conv2d_down2": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mdtile_gn_sums": (c_int, [c_void_p, c_int, c_int, c_size_t, c_size_t, c_size_t, c_int, c_void_p, c_void_p, c_void_p]),
    "mdtile_gn_from_sums": (c_int, [c_void_p, ctypes.c_double, c_int, c_void_p, c_void_p, c_void_p]),
    "mdtile_vae_attn_qk_ws_size": (c_size_t, [c_int, c_int, c_int, c_int]),
    "mdtile_vae_attn_qk": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "mdtile_gn_coeffs": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    "mdtile_conv2d_gn_supported": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "mdtile_conv2d_gn": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                 c_int, c_int, c_void_p]),
    "mdtile_conv_stats_ws_size": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),
    "mdtile_conv2d_gn_stats_supported": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "mdtile_conv2d_gn_stats": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                                       c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]),
    "mdtile_conv2d_rec_stats_supported": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "mdtile_conv2d_rec_stats": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                                        c_void_p, c_void_p, c_void_p, c_void_p]),
    "mdtile_rec_size": (c_size_t, [c_int, c_int, c_int, c_int]),
    "mdtile_rec_from_f32": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "mdtile_rec_to_f32": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "mdtile_rec_from_f32_fmt": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mdtile_rec_to_f32_fmt": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "mdtile_conv2d_rec_supported": (c_int, [c_int, c_int, c_int, c_int]),
    "mdtile_conv2d_rec": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                  c_int, c_int, c_void_p]),
    "mdtile_upconv2d_rec_window": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p] + [c_int] * 5 + [c_void_p, c_void_p, c_int, c_int,
                                                                                                                  c_int, c_void_p]),
    "mdtile_vae_attn_ws_size": (c_size_t, [c_int, c_int, c_int]),
    "mdtile_vae_attn_takes_channel_major": (c_int, [c_int, c_int]),
    "mdtile_vae_attn": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_float, c_int, c_void_p, c_void_p]),
    "mdtile_crop_store": (c_int, [c_void_p, c_int, c_int, c_int, c_int, _IP, _IP, c_int, c_void_p, c_int, c_int, c_void_p]),
    "mdtile_vae_assemble": (c_int, [POINTER(_VaeTile), c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "mdtile_vae_assemble_blend": (c_int, [POINTER(_VaeTile), c_int, c_int, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "mdtile_enable_peer_access": (c_int, [c_int, c_int]),
    "mdtile_mask_activity_u8": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p]),
    "mdtile_vae_assemble_sparse": (c_int, [POINTER(_VaeTile), c_int, _IP, c_int, c_void_p, c_int, c_int, c_void_p, c_int, c_int, c_void_p]),
    "mdtile_vae_fast_size": (c_int, [c_int, c_int, c_int, _IP, _IP]),
    "mdtile_vae_fast_ws_size": (c_size_t, [c_int]),
    "mdtile_vae_fast_input": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
}

_lib = None


def lib() -> ctypes.CDLL:
    """Load libmdtile.so (once).  Raises loudly when it is absent -- there is no fallback path."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MdtileError(f"{LIB_PATH} not found: build it with `python -m mdtile.build` (hipcc, gfx950). "
                          "This extension has no CPU/eager fallback.")
    L = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(L, name)  # AttributeError if the library does not export what the header declares
        fn.restype, fn.argtypes = res, args
    if L.mdtile_version() != 100:
        raise MdtileError(f"libmdtile.so version {L.mdtile_version()} != binding version 100")
    _lib = L
    return L


PRECISION_BF16X3, PRECISION_F32, PRECISION_BF16 = 0, 1, 2
PRECISION_F16 = 5


def set_precision(mode: int) -> None:
    """Arithmetic of the matrix-core kernels (convs, attention), process-wide:
    PRECISION_BF16X3 (default): split-bf16 operands, three bf16 MFMAs per product, fp32 accumulation (~1e-5 relative to fp32);
    PRECISION_F32: exact-fp32 MFMA kernels everywhere (~4x slower);
    PRECISION_BF16: one bf16 MFMA per product, bf16_rn(a) x bf16_rn(b) with fp32 accumulation -- the arithmetic of a half-precision
    (bfloat16) VAE; tensors in and out, the residual stream, GroupNorm statistics and softmax stay fp32;
    PRECISION_F16: one fp16 MFMA per product for the 3x3 convs behind a norm + SiLU (the arithmetic class of an fp16 VAE), three bf16 terms for
    every conv that reads the raw residual stream (it may pass fp16's range), the attention as in PRECISION_BF16 (include/mdtile.h).
    Raises MdtileError on any other value."""
    _check(lib().mdtile_set_precision(int(mode)), "mdtile_set_precision")


def get_precision() -> int:
    return int(lib().mdtile_get_precision())


@contextlib.contextmanager
def precision(mode: int):
    """`with mdtile.precision(mdtile.PRECISION_BF16): ...` -- sets the mode for the block and restores the previous one on the way out
    (also when the block raises).  The mode is process-wide: work queued on any stream inside the block runs in it.  A block that asks
    for the mode already in force changes nothing.  A load-time preset of only one strict bit (MDTILE_CONV_MODE=f32 without
    MDTILE_ATTN_MODE=f32, or the reverse) reads as PRECISION_BF16X3 and is restored as that."""
    prev = get_precision()
    if int(mode) == prev:
        yield
        return
    set_precision(mode)
    try:
        yield
    finally:
        set_precision(prev)


def exported_symbols() -> List[str]:
    return list(_SIGNATURES)


def _check(rc: int, what: str):
    if rc != OK:
        raise MdtileError(f"{what} failed (rc={rc}): {lib().mdtile_last_error().decode(errors='replace')}")


def require_device(dev) -> None:
    """The engine only runs on the GPU: callers check up front instead of failing inside the first kernel wrapper."""
    if torch.device(dev).type != "cuda":
        raise MdtileError(f"the mdtile engine needs its tensors on the GPU, got device {dev} (no CPU fallback exists; "
                          "for Tiled VAE enable 'Move VAE to GPU')")


def _dev_tensor(t: torch.Tensor, name: str, dtype=None) -> torch.Tensor:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if t.device.type != "cuda":
        raise MdtileError(f"{name} lives on {t.device}; the mdtile engine only runs on the GPU (no CPU fallback)")
    if dtype is not None and t.dtype != dtype:
        raise MdtileError(f"{name} has dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise MdtileError(f"{name} must be contiguous")
    return t


def _p(t: Optional[torch.Tensor]) -> c_void_p:
    return c_void_p(0) if t is None else c_void_p(t.data_ptr())


def _stream() -> c_void_p:
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def dtype_code(dt: torch.dtype) -> int:
    try:
        return _DTYPES[dt]
    except KeyError:
        raise MdtileError(f"unsupported dtype {dt}") from None


# ---------------------------------------------------------------------------------------------------------------------
class Plan:
    """Grid plan == split_bboxes + init_grid_bbox (tile_utils/utils.py:160-177, abstractdiffusion.py:173-186).
    wrap_x: the canvas is closed in x (panoramas, mdtile_plan_create_wrap): tile columns lie on a circle, a box's x + w may pass the canvas
    width (its columns are taken mod w), clamp is always on.  A tile as wide as the canvas raises MdtileError.
    wrap_y: the same for the rows; with wrap_x the canvas is a torus (seamless textures).  A box's y + h may pass the canvas height; a tile as
    tall as the canvas raises MdtileError.
    sparse: a plan of the tiles an inpaint mask touches (Plan.subset): the parent's geometry, `active_ids` = the parent tile indices it runs,
    bboxes / batches / num_tiles / num_batches / tile_bs of those tiles only; `parent_tiles` = the parent's tile count."""

    sparse = False
    active_ids: Tuple[int, ...] = ()

    def __init__(self, w: int, h: int, tile_w: int, tile_h: int, overlap: int, tile_bs: int, clamp: bool = True, wrap_x: bool = False,
                 wrap_y: bool = False):
        L = lib()
        self.wrap_x, self.wrap_y = bool(wrap_x), bool(wrap_y)
        if (self.wrap_x or self.wrap_y) and not clamp:
            axes = "wrap_x=True" if not self.wrap_y else "wrap_y=True"
            raise MdtileError(f"Plan({axes}) always clamps tile and overlap (clamp=False is not available)")
        if self.wrap_x or self.wrap_y:
            self._h = L.mdtile_plan_create_wrap(int(w), int(h), int(tile_w), int(tile_h), int(overlap), int(tile_bs), int(self.wrap_x), int(self.wrap_y))
        else:
            self._h = L.mdtile_plan_create(int(w), int(h), int(tile_w), int(tile_h), int(overlap), int(tile_bs), int(clamp))
        if not self._h:
            raise MdtileError("mdtile_plan_create: " + L.mdtile_last_error().decode(errors="replace"))
        info = (c_int * 8)()
        _check(L.mdtile_plan_info(self._h, info), "mdtile_plan_info")
        (self.cols, self.rows, self.num_tiles, self.num_batches, self.tile_bs, self.tile_w, self.tile_h,
         self.overlap) = list(info)
        self.w, self.h = int(w), int(h)
        self.parent_tiles = self.num_tiles
        self._read_boxes()

    def _read_boxes(self):
        L = lib()
        buf = (c_int * (4 * self.num_tiles))()
        _check(L.mdtile_plan_bboxes(self._h, buf), "mdtile_plan_bboxes")
        flat = list(buf)
        self.bboxes = [tuple(flat[4 * i:4 * i + 4]) for i in range(self.num_tiles)]  # (x, y, w, h), upstream order
        self.batches = [self.bboxes[i * self.tile_bs:(i + 1) * self.tile_bs] for i in range(self.num_batches)]

    def subset(self, active: Sequence[int], tile_bs: int) -> "Plan":
        """The sparse plan of the tiles with a non-zero flag in `active` (one flag per tile, as tile_activity returns them), batched by
        `tile_bs`: gather / gather_all fill its compact batches and blend_sparse blends them.  Raises MdtileError when no tile is active, on a
        wrap-around or sparse parent and beyond MAX_BATCHES batches.  The result does not depend on this plan staying alive."""
        L = lib()
        if len(active) != self.parent_tiles:
            raise MdtileError(f"Plan.subset: {len(active)} flags for {self.parent_tiles} tiles")
        flags = (c_int * max(1, len(active)))(*[1 if a else 0 for a in active])
        h = L.mdtile_plan_create_subset(self._h, flags, int(tile_bs))
        if not h:
            raise MdtileError("mdtile_plan_create_subset: " + L.mdtile_last_error().decode(errors="replace"))
        sub = Plan.__new__(Plan)
        sub._h = h
        sub.sparse, sub.wrap_x, sub.wrap_y = True, False, False
        sub.w, sub.h, sub.parent_tiles = self.w, self.h, self.parent_tiles
        info = (c_int * 8)()
        _check(L.mdtile_plan_info(h, info), "mdtile_plan_info")
        (sub.cols, sub.rows, sub.num_tiles, sub.num_batches, sub.tile_bs, sub.tile_w, sub.tile_h, sub.overlap) = list(info)
        ids = (c_int * sub.num_tiles)()
        n = L.mdtile_plan_active(h, ids)
        if n != sub.num_tiles:
            raise MdtileError(f"mdtile_plan_active: {n} active tiles, mdtile_plan_info reports {sub.num_tiles}")
        sub.active_ids = tuple(ids)
        sub._read_boxes()
        return sub

    @property
    def handle(self):
        return self._h

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.mdtile_plan_destroy(h)


class Lattice:
    """The jittered grid of one sampler step on a plain canvas (mdtile_lattice, include/mdtile.h): host integers only, no device table, nothing to
    destroy.  tile / overlap are the REQUESTED values (clamped as Plan(clamp=True) clamps them); sx in [1, stride_x], sy in [1, stride_y] on an
    axis that moves (tile < canvas), ignored on one that does not; (stride_x, stride_y) is the lattice at rest.  bboxes / batches are the
    PUSHED-IN boxes the model runs on, in tile order; num_tiles may differ by a column and a row between two shifts.  Raises MdtileError for a
    shift out of range."""

    def __init__(self, w: int, h: int, tile_w: int, tile_h: int, overlap: int, tile_bs: int, sx: int, sy: int):
        L = lib()
        self._c = _Lattice()
        _check(L.mdtile_lattice_make(int(w), int(h), int(tile_w), int(tile_h), int(overlap), int(tile_bs), int(sx), int(sy), ctypes.byref(self._c)),
               "mdtile_lattice_make")
        c = self._c
        self.w, self.h, self.tile_w, self.tile_h, self.overlap = c.w, c.h, c.tile_w, c.tile_h, c.overlap
        self.stride_x, self.stride_y, self.sx, self.sy = c.stride_x, c.stride_y, c.sx, c.sy
        self.cols, self.rows, self.num_tiles, self.num_batches, self.tile_bs = c.cols, c.rows, c.num_tiles, c.num_batches, c.tile_bs
        buf = (c_int * (4 * self.num_tiles))()
        _check(L.mdtile_lattice_bboxes(ctypes.byref(c), buf), "mdtile_lattice_bboxes")
        flat = list(buf)
        self.bboxes = [tuple(flat[4 * i:4 * i + 4]) for i in range(self.num_tiles)]
        self.batches = [self.bboxes[i * self.tile_bs:(i + 1) * self.tile_bs] for i in range(self.num_batches)]

    @property
    def ref(self):
        """The C struct by reference, for a call of the library."""
        return ctypes.byref(self._c)


class LatticeSubset:
    """The active tiles of one step's lattice (mdtile_lattice_subset, include/mdtile.h): flags = one per lattice tile (as lattice_activity returns
    them), slot = the device int32 table of their ranks (lattice_activity's second result, or the caller's own upload; kept alive here).  ids =
    the active tile indices in ascending order, bboxes / batches = their PUSHED-IN boxes in the compact batches, num_tiles = num_active = Ta.
    Raises MdtileError when no tile is active and beyond MAX_BATCHES batches.  Host integers only: nothing to destroy."""

    def __init__(self, lat: Lattice, flags: Sequence[int], tile_bs: int, slot: torch.Tensor):
        L = lib()
        if len(flags) != lat.num_tiles:
            raise MdtileError(f"LatticeSubset: {len(flags)} flags for {lat.num_tiles} tiles")
        _dev_tensor(slot, "slot", torch.int32)
        if slot.numel() != lat.num_tiles:
            raise MdtileError(f"LatticeSubset: slot table of {slot.numel()} entries for {lat.num_tiles} tiles")
        h_active = (c_int * max(1, len(flags)))(*[1 if a else 0 for a in flags])
        self._c = _LatticeSubset()
        _check(L.mdtile_lattice_subset_make(lat.ref, h_active, int(tile_bs), _p(slot), ctypes.byref(self._c)), "mdtile_lattice_subset_make")
        self.lat, self.slot = lat, slot
        self.num_active = self.num_tiles = self._c.num_active
        self.num_batches, self.tile_bs = self._c.num_batches, self._c.tile_bs
        self.w, self.h, self.tile_w, self.tile_h = lat.w, lat.h, lat.tile_w, lat.tile_h
        boxes, ids = (c_int * (4 * self.num_active))(), (c_int * self.num_active)()
        _check(L.mdtile_lattice_subset_bboxes(ctypes.byref(self._c), h_active, boxes, ids), "mdtile_lattice_subset_bboxes")
        flat = list(boxes)
        self.ids = tuple(ids)
        self.bboxes = [tuple(flat[4 * i:4 * i + 4]) for i in range(self.num_active)]
        self.batches = [self.bboxes[i * self.tile_bs:(i + 1) * self.tile_bs] for i in range(self.num_batches)]

    @property
    def ref(self):
        """The C struct by reference, for a call of the library."""
        return ctypes.byref(self._c)


def lattice_activity(lat: Lattice, mask: torch.Tensor) -> Tuple[List[int], torch.Tensor]:
    """Per tile of the step's lattice: 1 when some element of mask[:, contributing box] is not equal to zero (NaN counts, -0.0 does not), else 0
    -- the contributing box is the tile's LATTICE box clipped to the canvas, not the pushed-in box the model runs on.  -> (the flags on the host,
    the device int32 table of their ranks: slot[t] = number of active t' < t, or -1).  mask: fp32 [P, H, W] (or [H, W]) on the device.  Two
    launches and one device-to-host copy of num_tiles ints."""
    _dev_tensor(mask, "mask", torch.float32)
    if mask.dim() == 2:
        mask = mask.unsqueeze(0)
    if mask.dim() != 3 or tuple(mask.shape[-2:]) != (lat.h, lat.w):
        raise MdtileError(f"lattice_activity: mask {tuple(mask.shape)} is not [planes, {lat.h}, {lat.w}]")
    flags = torch.empty(lat.num_tiles, dtype=torch.int32, device=mask.device)
    slot = torch.empty(lat.num_tiles, dtype=torch.int32, device=mask.device)
    _check(lib().mdtile_lattice_activity(lat.ref, _p(mask), int(mask.shape[0]), _p(flags), _p(slot), _stream()), "mdtile_lattice_activity")
    return flags.cpu().tolist(), slot


def tile_activity(plan: Plan, mask: torch.Tensor) -> List[int]:
    """Per tile of the (plain) plan: 1 when some element of mask[:, y:y+h, x:x+w] is not equal to zero (NaN counts, -0.0 does not), else 0.
    mask: fp32 [P, H, W] (or [H, W]) on the device.  One launch and one device-to-host copy of num_tiles ints."""
    _dev_tensor(mask, "mask", torch.float32)
    if mask.dim() == 2:
        mask = mask.unsqueeze(0)
    if mask.dim() != 3 or tuple(mask.shape[-2:]) != (plan.h, plan.w):
        raise MdtileError(f"tile_activity: mask {tuple(mask.shape)} is not [planes, {plan.h}, {plan.w}]")
    flags = torch.empty(plan.parent_tiles, dtype=torch.int32, device=mask.device)
    _check(lib().mdtile_tile_activity(plan.handle, _p(mask), int(mask.shape[0]), _p(flags), _stream()), "mdtile_tile_activity")
    return flags.cpu().tolist()


# ---- maps ------------------------------------------------------------------------------------------------------------
def gaussian_weights(tile_w: int, tile_h: int, device) -> torch.Tensor:
    out = torch.empty((tile_h, tile_w), dtype=torch.float32, device=device)
    _dev_tensor(out, "out")
    _check(lib().mdtile_gaussian_weights(tile_w, tile_h, _p(out), _stream()), "mdtile_gaussian_weights")
    return out


def feather_mask(w: int, h: int, ratio: float, device) -> torch.Tensor:
    out = torch.empty((h, w), dtype=torch.float32, device=device)
    _dev_tensor(out, "out")
    _check(lib().mdtile_feather_mask(w, h, float(ratio), _p(out), _stream()), "mdtile_feather_mask")
    return out


def weight_map_add_grid(plan: Plan, tile_w: Optional[torch.Tensor], weights: torch.Tensor) -> None:
    _dev_tensor(weights, "weights", torch.float32)
    if tile_w is not None:
        _dev_tensor(tile_w, "tile_w", torch.float32)
        assert tuple(tile_w.shape[-2:]) == (plan.tile_h, plan.tile_w)
    assert weights.numel() == plan.w * plan.h
    _check(lib().mdtile_weight_map_add_grid(plan.handle, _p(tile_w), _p(weights), _stream()), "mdtile_weight_map_add_grid")


def lattice_weight_map(lat: Lattice, tile_w: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """The weight sum [h, w] of the step's grid, written (not added): the count of covering tiles (tile_w None), or the sum of the [tile_h, tile_w]
    map read in lattice coordinates.  The blend forms the same numbers itself; this call is for callers that want to look at them."""
    if tile_w is not None:
        _dev_tensor(tile_w, "tile_w", torch.float32)
        assert tuple(tile_w.shape) == (lat.tile_h, lat.tile_w), f"tile_w {tuple(tile_w.shape)}"
        device = tile_w.device
    if out is None:
        assert device is not None
        out = torch.empty((lat.h, lat.w), dtype=torch.float32, device=device)
    _dev_tensor(out, "out", torch.float32)
    assert out.numel() == lat.h * lat.w
    _check(lib().mdtile_lattice_weight_map(lat.ref, _p(tile_w), _p(out), _stream()), "mdtile_lattice_weight_map")
    return out


def weight_map_add_rect(weights: torch.Tensor, x: int, y: int, w: int, h: int, rect_w: Optional[torch.Tensor] = None,
                        scalar: float = 1.0) -> None:
    _dev_tensor(weights, "weights", torch.float32)
    H, W = weights.shape[-2:]
    if rect_w is not None:
        _dev_tensor(rect_w, "rect_w", torch.float32)
        assert rect_w.numel() == w * h
    _check(lib().mdtile_weight_map_add_rect(_p(weights), W, H, x, y, w, h, _p(rect_w), scalar, _stream()),
           "mdtile_weight_map_add_rect")


def weight_map_add_rect_wrap(weights: torch.Tensor, x: int, y: int, w: int, h: int, rect_w: Optional[torch.Tensor] = None,
                             scalar: float = 1.0, *, wrap_x: bool, wrap_y: bool) -> None:
    """weight_map_add_rect on a canvas closed on the axes whose flag is set: the rectangle's pixels are ((y + i) mod H, (x + j) mod W)."""
    _dev_tensor(weights, "weights", torch.float32)
    H, W = weights.shape[-2:]
    if rect_w is not None:
        _dev_tensor(rect_w, "rect_w", torch.float32)
        assert rect_w.numel() == w * h
    _check(lib().mdtile_weight_map_add_rect_wrap(_p(weights), W, H, int(x), int(y), int(w), int(h), _p(rect_w), scalar, int(bool(wrap_x)),
                                                 int(bool(wrap_y)), _stream()), "mdtile_weight_map_add_rect_wrap")


def _noise_regions_array(noise: torch.Tensor, regions):
    C = noise.shape[1]
    arr = (_Region * max(1, len(regions)))()
    keep = []
    for i, (x, y, w, h, mode, rand) in enumerate(regions):
        _dev_tensor(rand, f"regions[{i}].rand", torch.float32)
        assert tuple(rand.shape) == (1, C, h, w), f"region {i}: noise shape {tuple(rand.shape)} != (1, {C}, {h}, {w})"
        keep.append(rand)
        arr[i] = _Region(int(x), int(y), int(w), int(h), int(mode), 0, rand.data_ptr(), None)
    return arr, keep


def region_noise_wrap(noise: torch.Tensor, regions, *, wrap_x: bool, wrap_y: bool) -> torch.Tensor:
    """region_noise on a canvas closed on the axes whose flag is set: a region may pass the edge there and goes on at the other side."""
    _dev_tensor(noise, "noise", torch.float32)
    N, C, H, W = noise.shape
    arr, _keep = _noise_regions_array(noise, regions)
    _check(lib().mdtile_region_noise_wrap(_p(noise), N, C, H, W, arr, len(regions), int(bool(wrap_x)), int(bool(wrap_y)), _stream()),
           "mdtile_region_noise_wrap")
    return noise


def region_noise(noise: torch.Tensor, regions) -> torch.Tensor:
    """In-place per-region noise paste (tilediffusion.py:486-529).  noise: [N,C,H,W] fp32 on the GPU;
    regions: [(x, y, w, h, mode, rand)] with rand = that region's own noise [1,C,h,w] fp32 (same device), in list order."""
    _dev_tensor(noise, "noise", torch.float32)
    N, C, H, W = noise.shape
    arr, _keep = _noise_regions_array(noise, regions)
    _check(lib().mdtile_region_noise(_p(noise), N, C, H, W, arr, len(regions), _stream()), "mdtile_region_noise")
    return noise


def region_noise_masked(noise: torch.Tensor, regions) -> torch.Tensor:
    """region_noise where a region counts only at the pixels it covers.  regions: [(x, y, w, h, mode, rand, cover)], cover = uint8 [h, w] on the
    device or None (the whole rectangle)."""
    _dev_tensor(noise, "noise", torch.float32)
    N, C, H, W = noise.shape
    plain, keep = _noise_regions_array(noise, [r[:6] for r in regions])
    arr = (_MaskRegion * max(1, len(regions)))()
    for i, r in enumerate(regions):
        arr[i] = _MaskRegion(plain[i], _cover_ptr(r[6], r[2], r[3], f"regions[{i}].cover", keep))
    _check(lib().mdtile_region_noise_masked(_p(noise), N, C, H, W, arr, len(regions), _stream()), "mdtile_region_noise_masked")
    return noise


def _cover_ptr(cover, w: int, h: int, name: str, keep: list) -> int:
    """The address of a region's coverage map (uint8 [h, w], contiguous, on the device), or 0 for None."""
    if cover is None:
        return 0
    _dev_tensor(cover, name, torch.uint8)
    assert cover.numel() == w * h, f"{name} {tuple(cover.shape)} vs rect {h}x{w}"
    keep.append(cover)
    return cover.data_ptr()


def mask_cover_u8(mask: torch.Tensor, w: int, h: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """A painted mask [Hm, Wm] (uint8 on the device, Hm >= h, Wm >= w) -> (cover uint8 [h, w] of 0 / 1, box int32[5] = {xmin, ymin, xmax + 1,
    ymax + 1, count} of the covered cells, zeros when there is none), both on the device: a cell is covered when at least half of the mask pixels it
    owns, weighted by their value, are set (2 * sum >= 255 * count).  No synchronisation: read the box with .tolist() when it is needed."""
    _dev_tensor(mask, "mask", torch.uint8)
    assert mask.dim() == 2, f"mask {tuple(mask.shape)}"
    cover = torch.empty((int(h), int(w)), dtype=torch.uint8, device=mask.device)
    box = torch.empty(5, dtype=torch.int32, device=mask.device)
    _check(lib().mdtile_mask_cover_u8(_p(mask), mask.shape[1], mask.shape[0], int(w), int(h), _p(cover), _p(box), _stream()), "mdtile_mask_cover_u8")
    return cover, box


def mask_region(cover: torch.Tensor, x: int, y: int, w: int, h: int, feather_ratio: Optional[float] = None):
    """The dense tensors of the region (x, y, w, h) on a canvas coverage [H, W]: (rcover uint8 [h, w], feather fp32 [h, w] or None when
    feather_ratio is None).  The feather falls off with the chessboard distance to the nearest cell that is not covered (include/mdtile.h)."""
    _dev_tensor(cover, "cover", torch.uint8)
    assert cover.dim() == 2, f"cover {tuple(cover.shape)}"
    H, W = cover.shape
    ok = w > 0 and h > 0      # the library refuses the rest by name; a bad size must not reach torch.empty
    rcover = torch.empty((h, w) if ok else (1, 1), dtype=torch.uint8, device=cover.device)
    feather = None if feather_ratio is None else torch.empty((h, w) if ok else (1, 1), dtype=torch.float32, device=cover.device)
    _check(lib().mdtile_mask_region(_p(cover), W, H, int(x), int(y), int(w), int(h), float(feather_ratio or 0.0), _p(rcover), _p(feather), _stream()),
           "mdtile_mask_region")
    return rcover, feather


def noise_inverse_blend(noise: torch.Tensor, inverse_noise: torch.Tensor, renoise_mask: torch.Tensor, regions=()) -> torch.Tensor:
    """Renoise composite of Noise Inversion (abstractdiffusion.py:651-676).  noise / inverse_noise [N,C,H,W] fp32, renoise_mask
    [H,W] fp32; regions: [(x, y, w, h, mode, feather [h,w] fp32 or None)] -- pass them only when the grid is disabled (:658)."""
    _dev_tensor(noise, "noise", torch.float32)
    _dev_tensor(inverse_noise, "inverse_noise", torch.float32)
    _dev_tensor(renoise_mask, "renoise_mask", torch.float32)
    N, C, H, W = noise.shape
    assert inverse_noise.shape == noise.shape and tuple(renoise_mask.shape) == (H, W)
    arr = (_Region * max(1, len(regions)))()
    keep = []
    for i, (x, y, w, h, mode, feather) in enumerate(regions):
        fp = 0
        if feather is not None:
            _dev_tensor(feather, f"regions[{i}].feather", torch.float32)
            assert feather.numel() == w * h
            keep.append(feather)
            fp = feather.data_ptr()
        arr[i] = _Region(int(x), int(y), int(w), int(h), int(mode), 0, None, fp)
    out = torch.empty_like(noise)
    _check(lib().mdtile_noise_inverse_blend(_p(noise), _p(inverse_noise), _p(renoise_mask), _p(out), N, C, H, W, arr, len(regions), _stream()),
           "mdtile_noise_inverse_blend")
    return out


def retouch_mask(img_u8: torch.Tensor, kernel_size: int) -> torch.Tensor:
    """Renoise mask of Noise Inversion before the resize (get_retouch_mask, tile_utils/utils.py:216-247): img_u8 [H, W] grey or [H, W, 3] RGB
    bytes on the GPU -> [H, W] fp32 levels q / 255, defined exactly in include/mdtile.h.  1 <= kernel_size <= 512."""
    _dev_tensor(img_u8, "img_u8", torch.uint8)
    if not (img_u8.dim() == 2 or (img_u8.dim() == 3 and img_u8.shape[2] == 3)):
        raise MdtileError(f"img_u8 has shape {tuple(img_u8.shape)}, expected [H, W] or [H, W, 3]")
    H, W = int(img_u8.shape[0]), int(img_u8.shape[1])
    L = lib()
    ws = torch.empty(max(8, L.mdtile_retouch_mask_ws_size(H, W, int(kernel_size))), dtype=torch.uint8, device=img_u8.device)
    out = torch.empty((H, W), dtype=torch.float32, device=img_u8.device)
    _check(L.mdtile_retouch_mask(_p(img_u8), H, W, 1 if img_u8.dim() == 2 else 3, int(kernel_size), _p(out), _p(ws), _stream()),
           "mdtile_retouch_mask")
    return out


def renoise_resize(mask: torch.Tensor, size: Tuple[int, int], strength: float) -> torch.Tensor:
    """clamp((1 - bilinear(mask [H, W] -> size = (h, w))) * strength, 0, 1): the weight of fresh noise on the latent grid
    (abstractdiffusion.py:619-621), torch's align_corners=False rule in fp32."""
    _dev_tensor(mask, "mask", torch.float32)
    assert mask.dim() == 2, f"mask has shape {tuple(mask.shape)}, expected [H, W]"
    H, W = mask.shape
    h, w = int(size[0]), int(size[1])
    out = torch.empty((h, w), dtype=torch.float32, device=mask.device)
    _check(lib().mdtile_renoise_resize(_p(mask), H, W, float(strength), _p(out), h, w, _stream()), "mdtile_renoise_resize")
    return out

_RESAMPLE_TABLES: dict = {}      # (in, out, filter) -> (coef [out, ksize] int32, bounds [out, 2] int32), host arrays; a job asks for a handful


def resample_tables(in_size: int, out_size: int, filter: int):
    """The tap table of one axis of resize_u8 (mdtile_resample_table, defined in include/mdtile.h): (coef [out, ksize], bounds [out, 2]) as numpy
    int32 arrays, computed on the host and kept per (in, out, filter).  The arrays are shared: do not write to them."""
    import numpy as np
    key = (int(in_size), int(out_size), int(filter))
    hit = _RESAMPLE_TABLES.get(key)
    if hit is not None:
        return hit
    L = lib()
    ksize = L.mdtile_resample_ksize(*key)
    if ksize <= 0:
        raise MdtileError(f"resample_tables: bad arguments {key[0]} -> {key[1]}, filter {key[2]} (sizes >= 1, filter RESAMPLE_NEAREST / RESAMPLE_LANCZOS)")
    coef = np.empty((key[1], ksize), np.int32)
    bounds = np.empty((key[1], 2), np.int32)
    _check(L.mdtile_resample_table(key[0], key[1], key[2], c_void_p(coef.ctypes.data), c_void_p(bounds.ctypes.data)), "mdtile_resample_table")
    if len(_RESAMPLE_TABLES) >= 32:
        _RESAMPLE_TABLES.clear()
    _RESAMPLE_TABLES[key] = (coef, bounds)
    return coef, bounds


def resize_u8(img_u8: torch.Tensor, size: Tuple[int, int], filter: int) -> torch.Tensor:
    """Pillow's Image.resize for 8-bit images, bit for bit (include/mdtile.h): img_u8 [H, W] or [H, W, 3] bytes on the GPU -> size = (out_h, out_w),
    filter RESAMPLE_LANCZOS or RESAMPLE_NEAREST.  Runs on the input's device and its current stream; any strides and any alignment."""
    if not isinstance(img_u8, torch.Tensor):
        raise TypeError("img_u8 must be a tensor")
    if img_u8.device.type != "cuda":
        raise MdtileError(f"img_u8 lives on {img_u8.device}; the mdtile engine only runs on the GPU (no CPU fallback)")
    if img_u8.dtype != torch.uint8:
        raise MdtileError(f"img_u8 has dtype {img_u8.dtype}, expected {torch.uint8}")
    if not (img_u8.dim() == 2 or (img_u8.dim() == 3 and img_u8.shape[2] == 3)):
        raise MdtileError(f"img_u8 has shape {tuple(img_u8.shape)}, expected [H, W] or [H, W, 3]")
    if int(filter) not in (RESAMPLE_NEAREST, RESAMPLE_LANCZOS):
        raise MdtileError(f"resize_u8: unknown filter {filter}")
    img_u8 = img_u8.contiguous()
    H, W, C = int(img_u8.shape[0]), int(img_u8.shape[1]), 1 if img_u8.dim() == 2 else 3
    oh, ow = int(size[0]), int(size[1])
    L = lib()
    dev = img_u8.device
    with torch.cuda.device(dev):
        def axis(n_in, n_out):      # Lanczos skips an axis that keeps its size; Nearest always has both tables
            if int(filter) == RESAMPLE_LANCZOS and n_in == n_out:
                return None, None, 0
            coef, bounds = resample_tables(n_in, n_out, filter)
            return torch.from_numpy(coef).to(dev), torch.from_numpy(bounds).to(dev), coef.shape[1]
        if H < 1 or W < 1 or oh < 1 or ow < 1:
            raise MdtileError(f"resize_u8: bad sizes {H} x {W} -> {oh} x {ow}")
        cx, bx, kx = axis(W, ow)
        cy, by, ky = axis(H, oh)
        out = torch.empty((oh, ow) if C == 1 else (oh, ow, 3), dtype=torch.uint8, device=dev)
        ws = None
        if kx and ky:
            ws = torch.empty(max(1, L.mdtile_resample_u8_ws_size(H, W, C, oh, ow)), dtype=torch.uint8, device=dev)
        _check(L.mdtile_resample_u8(_p(img_u8), H, W, C, _p(out), oh, ow, _p(cx), _p(bx), kx, _p(cy), _p(by), ky, _p(ws), _stream()),
               "mdtile_resample_u8")
    return out


def _u8_image(t: torch.Tensor, name: str) -> Tuple[torch.Tensor, int, int, int]:
    """A uint8 image [H, W] / [H, W, 3] on the GPU, made contiguous -> (tensor, H, W, C)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if t.device.type != "cuda":
        raise MdtileError(f"{name} lives on {t.device}; the mdtile engine only runs on the GPU (no CPU fallback)")
    if t.dtype != torch.uint8:
        raise MdtileError(f"{name} has dtype {t.dtype}, expected {torch.uint8}")
    if not (t.dim() == 2 or (t.dim() == 3 and t.shape[2] in (1, 3))):
        raise MdtileError(f"{name} has shape {tuple(t.shape)}, expected [H, W], [H, W, 1] or [H, W, 3]")
    if t.numel() == 0:
        raise MdtileError(f"{name} has shape {tuple(t.shape)}: an empty image")
    return t.contiguous(), int(t.shape[0]), int(t.shape[1]), 1 if t.dim() == 2 else int(t.shape[2])


def colorfix_wavelet(content: torch.Tensor, style: torch.Tensor) -> torch.Tensor:
    """The wavelet colour fix on bytes, bit for bit the definition in include/mdtile.h: the content's detail over the style's low frequencies,
    out = clamp((content * 2^20 + low5(style - content) + 2^19) >> 20, 0, 255).  content, style: uint8 [H, W] or [H, W, 3] of the same shape on
    one GPU, any strides and any alignment -> a new tensor of that shape.  Runs on the content's device and its current stream."""
    content, H, W, C = _u8_image(content, "content")
    style, *_ = _u8_image(style, "style")
    if style.shape != content.shape or style.device != content.device:
        raise MdtileError(f"colorfix_wavelet: style {tuple(style.shape)} on {style.device} does not match content {tuple(content.shape)} on "
                          f"{content.device} (resize the style first: resize_u8)")
    L = lib()
    with torch.cuda.device(content.device):
        ws = torch.empty(max(4, L.mdtile_colorfix_wavelet_ws_size(H, W, C) // 4), dtype=torch.int32, device=content.device)
        out = torch.empty_like(content)
        _check(L.mdtile_colorfix_wavelet(_p(content), _p(style), _p(out), H, W, C, _p(ws), _stream()), "mdtile_colorfix_wavelet")
    return out


def hist_u8(img: torch.Tensor) -> torch.Tensor:
    """Exact counts of every byte value per channel: img uint8 [H, W] / [H, W, 3] on the GPU -> int64 [C, 256] on the same device (the
    engine's uint32 counts, widened).  Runs on the input's device and its current stream."""
    img, H, W, C = _u8_image(img, "img")
    with torch.cuda.device(img.device):
        counts = torch.empty((C, 256), dtype=torch.int32, device=img.device)      # uint32 bit patterns; below 2^31 by the size limit
        _check(lib().mdtile_hist_u8(_p(img), H, W, C, _p(counts), _stream()), "mdtile_hist_u8")
        return counts.to(torch.int64)


def adain_lut(hist_content, hist_style):
    """The AdaIN colour fix as per-channel 256-entry tables, on the HOST (include/mdtile.h): hist_* [C, 256] counts (tensor, array or lists) of
    the content and of the style image -> numpy uint8 [C, 256].  Sums are Python integers, mean and variance one correctly rounded division
    each, the table float64 in the order written in the header."""
    import numpy as np

    def stats(counts):
        counts = [int(v) for v in counts]
        n = sum(counts)
        s1 = sum(x * c for x, c in enumerate(counts))
        s2 = sum(x * x * c for x, c in enumerate(counts))
        if n < 1:
            raise MdtileError("adain_lut: an empty histogram")
        mean = s1 / n
        var = (n * s2 - s1 * s1) / (n * (n - 1)) if n > 1 else 0.0
        return mean, math.sqrt(var + 0.65025)

    hc = hist_content.cpu().tolist() if isinstance(hist_content, torch.Tensor) else np.asarray(hist_content).tolist()
    hs = hist_style.cpu().tolist() if isinstance(hist_style, torch.Tensor) else np.asarray(hist_style).tolist()
    if len(hc) != len(hs) or len(hc) not in (1, 3) or any(len(r) != 256 for r in hc + hs):
        raise MdtileError("adain_lut: both histograms are [C, 256] with the same C in {1, 3}")
    x = np.arange(256, dtype=np.float64)
    lut = np.empty((len(hc), 256), np.uint8)
    for c in range(len(hc)):
        mean_c, std_c = stats(hc[c])
        mean_s, std_s = stats(hs[c])
        lut[c] = np.clip(np.floor((x - mean_c) / std_c * std_s + mean_s + 0.5), 0, 255).astype(np.uint8)
    return lut


def lut_u8(img: torch.Tensor, lut) -> torch.Tensor:
    """out[y, x, c] = lut[c][img[y, x, c]]: img uint8 [H, W] / [H, W, 3] on the GPU, lut uint8 [C, 256] (tensor on any device, or array)."""
    img, H, W, C = _u8_image(img, "img")
    lut = torch.as_tensor(lut)
    if lut.dtype != torch.uint8 or tuple(lut.shape) != (C, 256):
        raise MdtileError(f"lut_u8: lut is {lut.dtype} {tuple(lut.shape)}, expected torch.uint8 ({C}, 256)")
    with torch.cuda.device(img.device):
        lut = lut.to(img.device).contiguous()
        out = torch.empty_like(img)
        _check(lib().mdtile_lut_u8(_p(img), H, W, C, _p(lut), _p(out), _stream()), "mdtile_lut_u8")
    return out


def colorfix_adain(content: torch.Tensor, style: torch.Tensor) -> torch.Tensor:
    """The AdaIN colour fix on bytes (include/mdtile.h): every channel of the content shifted and scaled to the style's mean and deviation.
    content, style: uint8 [H, W] / [H, W, 3] on the GPU with the same channel count; their sizes may differ."""
    return lut_u8(content, adain_lut(hist_u8(content), hist_u8(style)))


def gather_rects(x_in: torch.Tensor, rects_xy: Sequence[Tuple[int, int]], w: int, h: int, repeat: int = 1, tile_major: bool = True) -> torch.Tensor:
    """cat([x_in[:, :, y:y+h, x:x+w] for (x, y) in rects_xy]) repeated for the sampler's batch copies in one launch
    (ControlNet / StableSR tile slicing, abstractdiffusion.py:475-544, 548-588).  tile_major: every row's copies are consecutive
    (k-diffusion); else the whole batch is repeated (DDIM)."""
    _dev_tensor(x_in, "x_in")
    N, C, H, W = x_in.shape
    n = len(rects_xy)
    flat = (c_int * (2 * n))(*[int(v) for xy in rects_xy for v in xy])
    out = torch.empty((n * N * repeat, C, h, w), dtype=x_in.dtype, device=x_in.device)
    _check(lib().mdtile_gather_rects(dtype_code(x_in.dtype), N, C, W, H, _p(x_in), flat, n, int(w), int(h), int(repeat), int(tile_major),
                                     _p(out), _stream()), "mdtile_gather_rects")
    return out


def reciprocal(x: torch.Tensor) -> torch.Tensor:
    _dev_tensor(x, "x", torch.float32)
    out = torch.empty_like(x)
    _check(lib().mdtile_reciprocal(_p(x), _p(out), x.numel(), _stream()), "mdtile_reciprocal")
    return out


def rect_mul_canvas(rect_w: torch.Tensor, canvas: torch.Tensor, x: int, y: int, w: int, h: int) -> None:
    _dev_tensor(rect_w, "rect_w", torch.float32)
    _dev_tensor(canvas, "canvas", torch.float32)
    H, W = canvas.shape[-2:]
    assert rect_w.numel() == w * h
    _check(lib().mdtile_rect_mul_canvas(_p(rect_w), _p(canvas), W, H, x, y, w, h, _stream()), "mdtile_rect_mul_canvas")


# ---- gather ----------------------------------------------------------------------------------------------------------
def gather(plan: Plan, x_in: torch.Tensor, batch_id: int) -> torch.Tensor:
    """x_tile = cat([x_in[bbox.slicer] for bbox in batch]) -- tile-major (multidiffusion.py:155)."""
    _dev_tensor(x_in, "x_in")
    N, C, H, W = x_in.shape
    assert (H, W) == (plan.h, plan.w)
    nb = len(plan.batches[batch_id])
    out = torch.empty((nb * N, C, plan.tile_h, plan.tile_w), dtype=x_in.dtype, device=x_in.device)
    _check(lib().mdtile_gather(plan.handle, dtype_code(x_in.dtype), N, C, _p(x_in), batch_id, _p(out), _stream()), "mdtile_gather")
    return out


def gather_all(plan: Plan, x_in: torch.Tensor, out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """All tile batches in one launch."""
    _dev_tensor(x_in, "x_in")
    N, C, H, W = x_in.shape
    assert (H, W) == (plan.h, plan.w)
    if out is None and len(plan.batches) > MAX_BATCHES:
        # beyond the pointer table of the kernel arguments: one tile-major buffer, the batches are views into it
        packed = torch.empty((plan.num_tiles * N, C, plan.tile_h, plan.tile_w), dtype=x_in.dtype, device=x_in.device)
        gather_range(plan, x_in, packed, 0, plan.num_tiles)
        return list(packed.split([len(b) * N for b in plan.batches], dim=0))
    if out is None:
        out = [torch.empty((len(b) * N, C, plan.tile_h, plan.tile_w), dtype=x_in.dtype, device=x_in.device)
               for b in plan.batches]
    ptrs = (c_void_p * len(out))(*[t.data_ptr() for t in out])
    _check(lib().mdtile_gather_all(plan.handle, dtype_code(x_in.dtype), N, C, _p(x_in), ptrs, len(out), _stream()),
           "mdtile_gather_all")
    return list(out)


def gather_all_shift(plan: Plan, x_in: torch.Tensor, sx: int, sy: int, out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """gather_all with the wrapped grid displaced cyclically by (sx, sy): every tile batch of roll(x_in, (-sy, -sx)), one launch, nothing copied.
    Wrap-around plans only; a non-zero shift needs an axis that wraps."""
    _dev_tensor(x_in, "x_in")
    N, C, H, W = x_in.shape
    assert (H, W) == (plan.h, plan.w)
    if out is None:
        out = [torch.empty((len(b) * N, C, plan.tile_h, plan.tile_w), dtype=x_in.dtype, device=x_in.device)
               for b in plan.batches]
    for i, t in enumerate(out):
        _dev_tensor(t, f"out[{i}]", x_in.dtype)
    ptrs = (c_void_p * max(1, len(out)))(*[t.data_ptr() for t in out])
    _check(lib().mdtile_gather_all_shift(plan.handle, dtype_code(x_in.dtype), N, C, _p(x_in), ptrs, len(out), int(sx), int(sy), _stream()),
           "mdtile_gather_all_shift")
    return list(out)


def gather_all_lattice(lat: Lattice, x_in: torch.Tensor, out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """gather_all on the step's jittered grid: every tile batch cut at the lattice's pushed-in boxes, one launch, no plan."""
    _dev_tensor(x_in, "x_in")
    N, C, H, W = x_in.shape
    assert (H, W) == (lat.h, lat.w)
    if out is None:
        out = [torch.empty((len(b) * N, C, lat.tile_h, lat.tile_w), dtype=x_in.dtype, device=x_in.device) for b in lat.batches]
    for i, t in enumerate(out):
        _dev_tensor(t, f"out[{i}]", x_in.dtype)
        assert i >= len(lat.batches) or tuple(t.shape) == (len(lat.batches[i]) * N, C, lat.tile_h, lat.tile_w), f"out[{i}] {tuple(t.shape)}"
    ptrs = (c_void_p * max(1, len(out)))(*[t.data_ptr() for t in out])
    _check(lib().mdtile_gather_all_lattice(lat.ref, dtype_code(x_in.dtype), N, C, _p(x_in), ptrs, len(out), _stream()), "mdtile_gather_all_lattice")
    return list(out)


def gather_all_lattice_sparse(sub: LatticeSubset, x_in: torch.Tensor, out: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
    """gather_all_lattice of the active tiles only, into the subset's compact batches: one launch."""
    _dev_tensor(x_in, "x_in")
    N, C, H, W = x_in.shape
    assert (H, W) == (sub.h, sub.w)
    if out is None:
        out = [torch.empty((len(b) * N, C, sub.tile_h, sub.tile_w), dtype=x_in.dtype, device=x_in.device) for b in sub.batches]
    for i, t in enumerate(out):
        _dev_tensor(t, f"out[{i}]", x_in.dtype)
        assert i >= len(sub.batches) or tuple(t.shape) == (len(sub.batches[i]) * N, C, sub.tile_h, sub.tile_w), f"out[{i}] {tuple(t.shape)}"
    ptrs = (c_void_p * max(1, len(out)))(*[t.data_ptr() for t in out])
    _check(lib().mdtile_gather_all_lattice_sparse(sub.ref, dtype_code(x_in.dtype), N, C, _p(x_in), ptrs, len(out), _stream()),
           "mdtile_gather_all_lattice_sparse")
    return list(out)


def gather_range(plan: Plan, x_in: torch.Tensor, packed: torch.Tensor, tile_lo: int, tile_hi: int) -> torch.Tensor:
    """Tiles [tile_lo, tile_hi) into the packed [T*N, C, th, tw] buffer (rows of other tiles are left untouched)."""
    _dev_tensor(x_in, "x_in")
    _dev_tensor(packed, "packed", x_in.dtype)
    N, C, H, W = x_in.shape
    assert (H, W) == (plan.h, plan.w) and packed.numel() == plan.num_tiles * N * C * plan.tile_h * plan.tile_w
    _check(lib().mdtile_gather_range(plan.handle, dtype_code(x_in.dtype), N, C, _p(x_in), _p(packed), tile_lo, tile_hi, _stream()),
           "mdtile_gather_range")
    return packed


def gather_rect(x_in: torch.Tensor, x: int, y: int, w: int, h: int) -> torch.Tensor:
    _dev_tensor(x_in, "x_in")
    N, C, H, W = x_in.shape
    out = torch.empty((N, C, h, w), dtype=x_in.dtype, device=x_in.device)
    _check(lib().mdtile_gather_rect(dtype_code(x_in.dtype), N, C, W, H, _p(x_in), x, y, w, h, _p(out), _stream()),
           "mdtile_gather_rect")
    return out


def gather_rect_wrap(x_in: torch.Tensor, x: int, y: int, w: int, h: int, *, wrap_x: bool, wrap_y: bool, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """gather_rect on a canvas closed on the axes whose flag is set: out[n, c, i, j] = x_in[n, c, (y + i) mod H, (x + j) mod W]."""
    _dev_tensor(x_in, "x_in")
    N, C, H, W = x_in.shape
    if out is None:
        out = torch.empty((N, C, h, w), dtype=x_in.dtype, device=x_in.device)
    _dev_tensor(out, "out", x_in.dtype)
    assert out.numel() >= N * C * h * w, f"out {tuple(out.shape)}"
    _check(lib().mdtile_gather_rect_wrap(dtype_code(x_in.dtype), N, C, W, H, _p(x_in), int(x), int(y), int(w), int(h), int(bool(wrap_x)),
                                         int(bool(wrap_y)), _p(out), _stream()), "mdtile_gather_rect_wrap")
    return out


# ---- blend -----------------------------------------------------------------------------------------------------------
class RegionSpec:
    """One custom region for the blend: rect, mode, its model output and (optional) weight / feather map."""

    __slots__ = ("x", "y", "w", "h", "mode", "out", "weight", "cover")

    def __init__(self, x, y, w, h, mode, out, weight=None, cover=None):
        self.x, self.y, self.w, self.h, self.mode, self.out, self.weight = x, y, w, h, mode, out, weight
        self.cover = cover      # uint8 [h, w] on the device: where the region counts (blend_mask_regions); None = the whole rectangle


def _regions_array(regions: Sequence[RegionSpec], dtype, limit: bool = True):
    """limit False: the count is left to the library (blend_wrap_regions: it refuses by name)."""
    if limit and len(regions) > MAX_REGIONS:
        raise MdtileError(f"{len(regions)} regions > {MAX_REGIONS}")
    arr = (_Region * max(1, len(regions)))()
    keep = []
    for i, r in enumerate(regions):
        out = _dev_tensor(r.out, f"region[{i}].out", dtype)
        keep.append(out)
        wp = 0
        if r.weight is not None:
            wt = _dev_tensor(r.weight, f"region[{i}].weight", torch.float32)
            assert wt.numel() == r.w * r.h
            keep.append(wt)
            wp = wt.data_ptr()
        assert tuple(out.shape[-2:]) == (r.h, r.w), f"region[{i}] output {tuple(out.shape)} vs rect {r.h}x{r.w}"
        arr[i] = _Region(r.x, r.y, r.w, r.h, r.mode, 0, out.data_ptr(), wp)
    return arr, keep


def _as_one_buffer(parts: Sequence[torch.Tensor]) -> torch.Tensor:
    """The tensors of `parts` as one contiguous [sum rows, ...] tensor: zero-copy when they are back-to-back views of one storage."""
    first = parts[0]
    at, ok = first.data_ptr(), True
    for t in parts:
        ok = ok and t.is_contiguous() and t.data_ptr() == at and t.shape[1:] == first.shape[1:] and t.dtype == first.dtype
        at += t.numel() * t.element_size()
    rows = sum(t.shape[0] for t in parts)
    if ok and first.untyped_storage().nbytes() - first.storage_offset() * first.element_size() >= at - first.data_ptr():
        return first.as_strided((rows,) + tuple(first.shape[1:]), first.stride())
    return torch.cat(list(parts), dim=0)


def _blend_operands(plan: "Plan", method: int, batch_out, N: int, C: int, out_dtype, dtype, device, out, weights, tile_w, rescale, flags: int = 0,
                    tile_range=None, row_range=None):
    """What mdtile_blend and mdtile_blend_sparse share: the checked output (made here if None) and maps, the argument struct and the
    batch-pointer array -> (out, _BlendArgs, pointers)."""
    if out is None:
        out = torch.empty((N, C, plan.h, plan.w), dtype=out_dtype, device=device)
    _dev_tensor(out, "out", out_dtype)
    for nm, t in (("weights", weights), ("tile_w", tile_w), ("rescale", rescale)):
        if t is not None:
            _dev_tensor(t, nm, torch.float32)
    a = _BlendArgs(method, dtype_code(dtype), N, C, flags, *(tile_range or (0, 0)), *(row_range or (0, 0)),
                   _p(weights).value, _p(tile_w).value, _p(rescale).value, out.data_ptr())
    return out, a, (c_void_p * max(1, len(batch_out)))(*[t.data_ptr() for t in batch_out])


class BlendCall:
    """A fully marshalled mdtile_blend call: the argument struct, the batch-pointer array and the region array are built ONCE; calling
    the object only does the C call (a few microseconds of host time instead of rebuilding ~10 ctypes objects per evaluation -- the
    blend itself runs 20 us on an 8K canvas).  Valid while the tensors it was built from stay alive at the same addresses (sampler
    loops that write the model outputs into fixed buffers; bench.py)."""

    __slots__ = ("plan", "out", "_a", "_ptrs", "_n", "_rarr", "_nreg", "_keep", "_fn", "_aligned")

    def __init__(self, plan: Plan, method: int, batch_out: Sequence[torch.Tensor], N: int, C: int, *, weights=None, tile_w=None, rescale=None,
                 regions: Sequence[RegionSpec] = (), out: Optional[torch.Tensor] = None, dtype=None, device=None, partial: bool = False,
                 tile_range=None, row_range=None, packed: bool = False):
        if len(batch_out):
            dtype, device = batch_out[0].dtype, batch_out[0].device
        elif len(regions):
            dtype, device = regions[0].out.dtype, regions[0].out.device
        assert dtype is not None and device is not None
        for i, t in enumerate(batch_out):
            _dev_tensor(t, f"batch_out[{i}]", dtype)
        if not packed and len(batch_out) > MAX_BATCHES:
            # more tile batches than pointers ride in the kernel arguments (e.g. a 1024^2 latent at tile 96 / overlap 48 / batch 1 =
            # 441): hand the kernel ONE tile-major buffer instead.  Batches are consecutive runs of the tile list, so the views
            # gather_all returns in this situation are already one buffer; anything else costs one concatenation.
            batch_out, packed = [_as_one_buffer(batch_out)], True
        flags = (BLEND_PARTIAL if partial else 0) | (BLEND_PACKED if packed else 0) | (BLEND_TILE_RANGE if tile_range is not None else 0)
        self.plan = plan
        self.out, self._a, self._ptrs = _blend_operands(plan, method, batch_out, N, C, torch.float32 if partial else dtype, dtype, device, out, weights,
                                                        tile_w, rescale, flags, tile_range, row_range)
        self._n = len(batch_out)
        self._aligned = all(t.data_ptr() % 16 == 0 for t in batch_out)
        self._rarr, keep = _regions_array(regions, dtype)
        self._nreg = len(regions)
        self._keep = (list(batch_out), weights, tile_w, rescale, keep)
        self._fn = lib().mdtile_blend

    def __call__(self) -> torch.Tensor:
        rc = self._fn(self.plan.handle, ctypes.byref(self._a), self._ptrs, self._n, self._rarr, self._nreg, _stream())
        if rc != OK:
            _check(rc, "mdtile_blend")
        return self.out

    def dispatch(self) -> "BlendDispatch":
        """The kernel and launch shape this call gets (mdtile_blend_dispatch on exactly these arguments and pointers)."""
        a = self._a
        return _blend_dispatch(self.plan, a.dtype, a.N, a.C, a.flags, self._n, self._aligned, (a.row_lo, a.row_hi))


class BlendDispatch(NamedTuple):
    """Answer of mdtile_blend_dispatch: kernel = BLEND_KERNEL_PLAIN (k_blend: planes = planes per thread, shape = candidates per chunk;
    vec / elem / walk_quads = quads on its 16-byte loads, per-element loads, generic walk) or BLEND_KERNEL_LDS (k_blend_lds: planes = planes
    per block, shape = quads per strip, lds_bytes / ncs = the stage)."""
    kernel: int
    planes: int
    shape: int
    lds_bytes: int
    ncs: int
    vec_quads: int
    elem_quads: int
    walk_quads: int

    @property
    def lds(self) -> bool:
        return self.kernel == BLEND_KERNEL_LDS


def _blend_dispatch(plan: Plan, dtype_c: int, N: int, C: int, flags: int, num_batches: int, aligned: bool, rows) -> BlendDispatch:
    info = (c_int * 8)()
    _check(lib().mdtile_blend_dispatch(plan.handle, dtype_c, int(N), int(C), int(flags), int(num_batches), int(bool(aligned)),
                                       int(rows[0]), int(rows[1]), info), "mdtile_blend_dispatch")
    return BlendDispatch(*list(info))


def blend_dispatch(plan: Plan, dtype, N: int, C: int, *, partial: bool = False, tile_range=None, row_range=None, packed: bool = False,
                   num_batches: Optional[int] = None, aligned: bool = True) -> BlendDispatch:
    """Which kernel blend() launches for these arguments (no tensors, no device: the library answers from the plan's host tables with the
    function its launcher calls).  num_batches: tile-batch tensors handed over (default: the plan's; more than MAX_BATCHES are packed into
    one buffer, as BlendCall does); aligned: every batch tensor starts on a 16-byte boundary."""
    n = plan.num_batches if num_batches is None else int(num_batches)
    if not packed and n > MAX_BATCHES:
        n, packed = 1, True
    if packed and n > 0:
        n = 1
    flags = (BLEND_PARTIAL if partial else 0) | (BLEND_PACKED if packed else 0) | (BLEND_TILE_RANGE if tile_range is not None else 0)
    return _blend_dispatch(plan, dtype_code(dtype), N, C, flags, n, aligned, row_range or (0, 0))


def blend(plan: Plan, method: int, batch_out: Sequence[torch.Tensor], N: int, C: int, *, weights=None, tile_w=None,
          rescale=None, regions: Sequence[RegionSpec] = (), out: Optional[torch.Tensor] = None, dtype=None, device=None,
          partial: bool = False, tile_range=None, row_range=None, packed: bool = False) -> torch.Tensor:
    """One fused launch replacing the scatter/normalise/feather op sequence of sample_one_step / apply_model_hijack."""
    return BlendCall(plan, method, batch_out, N, C, weights=weights, tile_w=tile_w, rescale=rescale, regions=regions, out=out, dtype=dtype,
                     device=device, partial=partial, tile_range=tile_range, row_range=row_range, packed=packed)()


def _batch_operands(grid, batch_out, N: int, C: int, dtype, device, strict: bool, regions=()):
    """What the one-launch blends ask of batch_out first: dtype and device (the first batch's, else the first region output's, else as given), and
    every tensor on the device, in that dtype, shaped as the batch of `grid` (a Plan or a Lattice) at its index.  strict False: a tensor past the
    grid's batches goes unchecked -- the library refuses the count by name.  -> (dtype, device)"""
    if len(batch_out):
        dtype, device = batch_out[0].dtype, batch_out[0].device
    elif len(regions):
        dtype, device = regions[0].out.dtype, regions[0].out.device
    assert dtype is not None and device is not None
    for i, t in enumerate(batch_out):
        _dev_tensor(t, f"batch_out[{i}]", dtype)
        assert (not strict and i >= len(grid.batches)) or tuple(t.shape) == (len(grid.batches[i]) * N, C, grid.tile_h, grid.tile_w), \
            f"batch_out[{i}] {tuple(t.shape)}"
    return dtype, device


def _region_operands(regions: Sequence[RegionSpec], N: int, C: int, dtype):
    """The region array of the blends that take raw region weights: every output [N, C, h, w]; the count is left to the library."""
    for i, r in enumerate(regions):
        assert tuple(r.out.shape) == (N, C, r.h, r.w), f"region[{i}] output {tuple(r.out.shape)} vs [{N}, {C}, {r.h}, {r.w}]"
    return _regions_array(regions, dtype, limit=False)


def blend_shift(plan: Plan, method: int, batch_out: Sequence[torch.Tensor], N: int, C: int, *, sx: int, sy: int, weights=None, tile_w=None,
                rescale=None, out: Optional[torch.Tensor] = None, dtype=None, device=None) -> torch.Tensor:
    """blend on a wrap-around plan with the grid displaced cyclically by (sx, sy): roll(blend(...), (+sy, +sx)) bit for bit, in one launch.
    weights / tile_w / rescale are the plan's unshifted maps."""
    dtype, device = _batch_operands(plan, batch_out, N, C, dtype, device, strict=True)
    out, a, ptrs = _blend_operands(plan, method, batch_out, N, C, dtype, dtype, device, out, weights, tile_w, rescale)
    _check(lib().mdtile_blend_shift(plan.handle, ctypes.byref(a), ptrs, len(batch_out), int(sx), int(sy), _stream()), "mdtile_blend_shift")
    return out


def blend_wrap_regions(plan: Plan, method: int, batch_out: Sequence[torch.Tensor], N: int, C: int, *, regions: Sequence[RegionSpec] = (),
                       grid_w: Optional[torch.Tensor], region_w: torch.Tensor, sx: int = 0, sy: int = 0, tile_w=None, weights=None, rescale=None,
                       out: Optional[torch.Tensor] = None, dtype=None, device=None) -> torch.Tensor:
    """The blend of a wrap-around plan WITH custom regions, one launch: the grid (batch_out; empty = no grid is drawn) displaced by (sx, sy), then
    the regions where they lie on the canvas -- a region may cross a seam on an axis that wraps.  grid_w: the grid's weight sum [H, W] in plan
    coordinates (None iff batch_out is empty); region_w: the background regions' weight sum [H, W] on the canvas (zeros when there is none).
    A background region's weight is its RAW Gaussian (Mixture of Diffusers): the kernel forms grid_w + region_w and its reciprocal per pixel.
    weights / rescale exist only to be refused: the library takes no total map here."""
    dtype, device = _batch_operands(plan, batch_out, N, C, dtype, device, strict=False, regions=regions)
    for nm, t in (("grid_w", grid_w), ("region_w", region_w)):
        if t is not None:
            _dev_tensor(t, nm, torch.float32)
            assert t.numel() == plan.h * plan.w, f"{nm} {tuple(t.shape)}"
    out, a, ptrs = _blend_operands(plan, method, batch_out, N, C, dtype, dtype, device, out, weights, tile_w, rescale)
    rarr, _keep = _region_operands(regions, N, C, dtype)
    wr = _WrapRegions(rarr, len(regions), _p(grid_w).value, _p(region_w).value, int(sx), int(sy))
    _check(lib().mdtile_blend_wrap_regions(plan.handle, ctypes.byref(a), ptrs, len(batch_out), ctypes.byref(wr), _stream()), "mdtile_blend_wrap_regions")
    return out


def blend_mask_regions(plan: Plan, method: int, batch_out: Sequence[torch.Tensor], N: int, C: int, *, regions: Sequence[RegionSpec] = (), weights=None,
                       tile_w=None, rescale=None, out: Optional[torch.Tensor] = None, dtype=None, device=None, flags: int = 0, row_range=None) -> torch.Tensor:
    """blend on a plain plan where region r enters a pixel only if it covers it (r.cover, uint8 [h, w]; None = the whole rectangle), one launch.  A
    region's output and weight are not read elsewhere.  weights / rescale are the host's maps, made WITH the covers; a BG region's weight under Mixture
    of Diffusers is premultiplied as blend takes it.  flags / row_range exist only to be refused: the library takes neither here."""
    dtype, device = _batch_operands(plan, batch_out, N, C, dtype, device, strict=False, regions=regions)
    out, a, ptrs = _blend_operands(plan, method, batch_out, N, C, dtype, dtype, device, out, weights, tile_w, rescale, flags, None, row_range)
    rarr, keep = _region_operands(regions, N, C, dtype)
    marr = (_MaskRegion * max(1, len(regions)))()
    for i, r in enumerate(regions):
        marr[i] = _MaskRegion(rarr[i], _cover_ptr(r.cover, r.w, r.h, f"region[{i}].cover", keep))
    _check(lib().mdtile_blend_mask_regions(plan.handle, ctypes.byref(a), ptrs, len(batch_out), marr, len(regions), _stream()), "mdtile_blend_mask_regions")
    return out


def _blend_lattice(lat: Lattice, method: int, batch_out, N: int, C: int, tile_w, weights, rescale, out, dtype, device, regions=None, region_w=None):
    """blend_lattice (regions None) and blend_lattice_regions (a sequence, which may be empty)."""
    dtype, device = _batch_operands(lat, batch_out, N, C, dtype, device, strict=False)
    if region_w is not None:
        _dev_tensor(region_w, "region_w", torch.float32)
        assert region_w.numel() == lat.h * lat.w, f"region_w {tuple(region_w.shape)}"
    out, a, ptrs = _blend_operands(lat, method, batch_out, N, C, dtype, dtype, device, out, weights, tile_w, rescale)
    if regions is None:
        _check(lib().mdtile_blend_lattice(lat.ref, ctypes.byref(a), ptrs, len(batch_out), _stream()), "mdtile_blend_lattice")
        return out
    rarr, _keep = _region_operands(regions, N, C, dtype)
    lr = _LatticeRegions(rarr, len(regions), _p(region_w).value)
    _check(lib().mdtile_blend_lattice_regions(lat.ref, ctypes.byref(a), ptrs, len(batch_out), ctypes.byref(lr), _stream()),
           "mdtile_blend_lattice_regions")
    return out


def blend_lattice(lat: Lattice, method: int, batch_out: Sequence[torch.Tensor], N: int, C: int, *, tile_w=None, weights=None, rescale=None,
                  out: Optional[torch.Tensor] = None, dtype=None, device=None) -> torch.Tensor:
    """The blend of the step's jittered grid, one launch: every tile contributes where its LATTICE box lies, read at its pushed-in box; the weight
    sum of the step (MultiDiffusion's count, Mixture of Diffusers' Gaussian sum and its reciprocal) is formed inside the kernel.  tile_w: the
    [tile_h, tile_w] map, required for METHOD_MOD.  weights / rescale exist only to be refused: the library takes no maps here."""
    return _blend_lattice(lat, method, batch_out, N, C, tile_w, weights, rescale, out, dtype, device)


def blend_lattice_regions(lat: Lattice, method: int, batch_out: Sequence[torch.Tensor], N: int, C: int, *, regions: Sequence[RegionSpec] = (),
                          region_w: Optional[torch.Tensor] = None, tile_w=None, weights=None, rescale=None, out: Optional[torch.Tensor] = None,
                          dtype=None, device=None) -> torch.Tensor:
    """blend_lattice WITH custom regions, one launch: the step's jittered grid, then the regions where they lie on the canvas -- only the grid
    moves.  region_w: the background regions' weight sum [H, W] on the canvas (weight_map_add_rect on zeros in list order: 1.0 each for
    MultiDiffusion, the raw Gaussians for Mixture of Diffusers), made once per job; None iff there is no background region.  A background
    region's weight is its RAW Gaussian (Mixture of Diffusers): the kernel forms the step's weight sum + region_w and its reciprocal per pixel.
    weights / rescale exist only to be refused: the library takes no total map here."""
    return _blend_lattice(lat, method, batch_out, N, C, tile_w, weights, rescale, out, dtype, device, regions=list(regions), region_w=region_w)


def blend_lattice_sparse(sub: LatticeSubset, method: int, batch_out: Sequence[torch.Tensor], N: int, C: int, *, fill: torch.Tensor, tile_w=None,
                         weights=None, rescale=None, out: Optional[torch.Tensor] = None, dtype=None, device=None) -> torch.Tensor:
    """The blend of the active tiles of the step's lattice, one launch: batch_out = the model outputs of the subset's compact batches.  Where every
    covering lattice tile is active the result is blend_lattice()'s on the full lattice, bit for bit; everywhere else it is `fill` ([N, C, H, W],
    the outputs' dtype), bit for bit.  weights / rescale exist only to be refused: the library takes no maps here."""
    dtype, device = _batch_operands(sub, batch_out, N, C, dtype, device, strict=False)
    _dev_tensor(fill, "fill", dtype)
    assert tuple(fill.shape) == (N, C, sub.h, sub.w), f"fill {tuple(fill.shape)}"
    out, a, ptrs = _blend_operands(sub, method, batch_out, N, C, dtype, dtype, device, out, weights, tile_w, rescale)
    _check(lib().mdtile_blend_lattice_sparse(sub.ref, ctypes.byref(a), ptrs, len(batch_out), _p(fill), _stream()), "mdtile_blend_lattice_sparse")
    return out


def blend_sparse(plan: Plan, method: int, batch_out: Sequence[torch.Tensor], N: int, C: int, *, fill: torch.Tensor, weights=None, tile_w=None,
                 rescale=None, out: Optional[torch.Tensor] = None, dtype=None, device=None) -> torch.Tensor:
    """The blend of a sparse plan (Plan.subset): batch_out = the model outputs of its compact batches.  Where every covering tile of the parent
    is active the result is blend()'s on the parent, bit for bit; everywhere else it is `fill` ([N, C, H, W], the outputs' dtype), bit for bit.
    weights / rescale are the parent's full maps."""
    if not plan.sparse:
        raise MdtileError("blend_sparse needs a sparse plan (Plan.subset); the blend of a full plan is blend()")
    dtype, device = _batch_operands(plan, batch_out, N, C, dtype, device, strict=True)
    _dev_tensor(fill, "fill", dtype)
    assert tuple(fill.shape) == (N, C, plan.h, plan.w), f"fill {tuple(fill.shape)}"
    out, a, ptrs = _blend_operands(plan, method, batch_out, N, C, dtype, dtype, device, out, weights, tile_w, rescale)
    _check(lib().mdtile_blend_sparse(plan.handle, ctypes.byref(a), ptrs, len(batch_out), _p(fill), _stream()), "mdtile_blend_sparse")
    return out


class StreamCopyCall:
    """Marshalled mdtile_stream_copy (src -> dst, same size, contiguous, 16-byte aligned): the measurement floor bench.py times beside the
    blend kernel, launched the same way (see BlendCall)."""

    __slots__ = ("_args", "_fn", "_keep")

    def __init__(self, src: torch.Tensor, dst: torch.Tensor):
        _dev_tensor(src, "src")
        _dev_tensor(dst, "dst")
        nbytes = src.numel() * src.element_size()
        assert nbytes == dst.numel() * dst.element_size() and nbytes % 16 == 0
        self._args = (c_void_p(src.data_ptr()), c_void_p(dst.data_ptr()), c_size_t(nbytes))
        self._keep = (src, dst)
        self._fn = lib().mdtile_stream_copy

    def __call__(self) -> None:
        rc = self._fn(*self._args, _stream())
        if rc != OK:
            _check(rc, "mdtile_stream_copy")


def stream_copy(src: torch.Tensor, dst: torch.Tensor) -> torch.Tensor:
    StreamCopyCall(src, dst)()
    return dst


class GatherRangeCall:
    """Marshalled mdtile_gather_range (tiles [tile_lo, tile_hi) into a packed buffer), see BlendCall."""

    __slots__ = ("_args", "_fn", "_keep", "packed")

    def __init__(self, plan: Plan, x_in: torch.Tensor, packed: torch.Tensor, tile_lo: int, tile_hi: int):
        _dev_tensor(x_in, "x_in")
        _dev_tensor(packed, "packed", x_in.dtype)
        N, C, H, W = x_in.shape
        assert (H, W) == (plan.h, plan.w) and packed.numel() == plan.num_tiles * N * C * plan.tile_h * plan.tile_w
        self._args = (plan.handle, dtype_code(x_in.dtype), N, C, _p(x_in), _p(packed), int(tile_lo), int(tile_hi))
        self._fn = lib().mdtile_gather_range
        self._keep, self.packed = (plan, x_in), packed

    def __call__(self) -> torch.Tensor:
        rc = self._fn(*self._args, _stream())
        if rc != OK:
            _check(rc, "mdtile_gather_range")
        return self.packed


def blend_finalize(plan: Plan, method: int, partial: torch.Tensor, *, weights=None, regions: Sequence[RegionSpec] = (),
                   out: Optional[torch.Tensor] = None, dtype=torch.float32, row_range=None) -> torch.Tensor:
    _dev_tensor(partial, "partial", torch.float32)
    N, C = partial.shape[:2]
    if out is None:
        out = torch.empty((N, C, plan.h, plan.w), dtype=dtype, device=partial.device)
    _dev_tensor(out, "out", dtype)
    a = _BlendArgs(method, dtype_code(dtype), N, C, 0, 0, 0, *(row_range or (0, 0)), _p(weights).value, 0, 0, out.data_ptr())
    rarr, _keep = _regions_array(regions, dtype)
    _check(lib().mdtile_blend_finalize(plan.handle, ctypes.byref(a), _p(partial), rarr, len(regions), _stream()),
           "mdtile_blend_finalize")
    return out


# ---- tiled VAE -------------------------------------------------------------------------------------------------------
def vae_split_tiles(h: int, w: int, tile_size: int, is_decoder: bool = True):
    """split_tiles (scripts/tilevae.py:405-462): ([x1,x2,y1,y2] input bboxes, output bboxes).  Host ints only."""
    L = lib()
    n = L.mdtile_vae_split_tiles(h, w, tile_size, int(is_decoder), None, None, 0)
    if n < 0:
        _check(n, "mdtile_vae_split_tiles")
    ins, outs = (c_int * (4 * n))(), (c_int * (4 * n))()
    rc = L.mdtile_vae_split_tiles(h, w, tile_size, int(is_decoder), ins, outs, n)
    if rc < 0:
        _check(rc, "mdtile_vae_split_tiles")
    fi, fo = list(ins), list(outs)
    return [fi[4 * i:4 * i + 4] for i in range(n)], [fo[4 * i:4 * i + 4] for i in range(n)]


def vae_best_tile_size(lowerbound: int, upperbound: int) -> int:
    """get_best_tile_size (scripts/tilevae.py:390-403).  Host ints only."""
    return int(lib().mdtile_vae_best_tile_size(int(lowerbound), int(upperbound)))


def gn_stats(x: torch.Tensor, groups: int = 32):
    """get_var_mean (tilevae.py:207-215) -> (var, mean), each [B*groups]."""
    _dev_tensor(x, "x", torch.float32)
    B, C = x.shape[:2]
    HW = x.numel() // (B * C)
    mean = torch.empty(B * groups, dtype=torch.float32, device=x.device)
    var = torch.empty_like(mean)
    ws = torch.empty(lib().mdtile_gn_stats_ws_size(B, groups) // 8, dtype=torch.float64, device=x.device)
    _check(lib().mdtile_gn_stats(_p(x), B, C, HW, groups, _p(mean), _p(var), _p(ws), _stream()), "mdtile_gn_stats")
    return var, mean


def gn_pool(means: torch.Tensor, vars_: torch.Tensor, pixels: Sequence[int]):
    """GroupNormParam.summary (tilevae.py:320-335) -> (var, mean)."""
    _dev_tensor(means, "means", torch.float32)
    _dev_tensor(vars_, "vars", torch.float32)
    T, BG = means.shape
    assert len(pixels) == T
    mean = torch.empty(BG, dtype=torch.float32, device=means.device)
    var = torch.empty_like(mean)
    # p_i exactly as upstream forms them (fp32, tilevae.py:328-331); T host floats -- control data, not tensor math
    px = torch.tensor([int(p) for p in pixels], dtype=torch.float32) / max(pixels)
    frac = (px / torch.sum(px)).to(means.device)
    _check(lib().mdtile_gn_pool(_p(means), _p(vars_), _p(frac), T, BG, _p(mean), _p(var), _stream()), "mdtile_gn_pool")
    return var, mean


def gn_apply(x: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, gamma=None, beta=None, groups: int = 32,
             eps: float = 1e-6, silu: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """custom_group_norm (+ fused SiLU) (tilevae.py:218-245, 102-104)."""
    _dev_tensor(x, "x", torch.float32)
    B, C = x.shape[:2]
    HW = x.numel() // (B * C)
    if out is None:
        out = torch.empty_like(x)
    for nm, t in (("mean", mean), ("var", var)):
        _dev_tensor(t, nm, torch.float32)
        assert t.numel() == B * groups
    for nm, t in (("gamma", gamma), ("beta", beta)):
        if t is not None:
            _dev_tensor(t, nm, torch.float32)
            assert t.numel() == C
    _check(lib().mdtile_gn_apply(_p(x), _p(out), B, C, HW, groups, _p(mean), _p(var), _p(gamma), _p(beta), eps, int(silu),
                                 _stream()), "mdtile_gn_apply")
    return out


def gn_sums(x: torch.Tensor, row_lo: int, row_hi: int, groups: int = 32) -> torch.Tensor:
    """fp64 [B*groups, 2] (sum, sum of squares) over rows [row_lo, row_hi) of every plane of x [B, C, H, W] (the rows a rank
    owns; halo rows excluded).  Piece of get_var_mean (tilevae.py:207-215) for a row-split activation."""
    _dev_tensor(x, "x", torch.float32)
    B, C, H, W = x.shape
    assert 0 <= row_lo < row_hi <= H
    sums = torch.empty((B * groups, 2), dtype=torch.float64, device=x.device)
    ws = torch.empty(lib().mdtile_gn_stats_ws_size(B, groups) // 8, dtype=torch.float64, device=x.device)
    _check(lib().mdtile_gn_sums(_p(x), B, C, H * W, row_lo * W, (row_hi - row_lo) * W, groups, _p(sums), _p(ws), _stream()), "mdtile_gn_sums")
    return sums


def gn_from_sums(sums: torch.Tensor, count: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(var, mean) from all-reduced fp64 sums; count = elements per (sample, group) over every rank."""
    _dev_tensor(sums, "sums", torch.float64)
    BG = sums.shape[0]
    mean = torch.empty(BG, dtype=torch.float32, device=sums.device)
    var = torch.empty_like(mean)
    _check(lib().mdtile_gn_from_sums(_p(sums), float(count), BG, _p(mean), _p(var), _stream()), "mdtile_gn_from_sums")
    return var, mean


def gn_coeffs(mean: torch.Tensor, var: torch.Tensor, gamma, beta, C: int, groups: int = 32, eps: float = 1e-6) -> torch.Tensor:
    """[B, 2, C] per-channel (a, s) of a fixed-statistics GroupNorm: a = gamma / sqrt(var + eps), s = beta - mean * a --
    the operand of the fused pre-activation conv (`PackedConv.__call__(..., pre_gn=coef)`)."""
    _dev_tensor(mean, "mean", torch.float32)
    _dev_tensor(var, "var", torch.float32)
    B = mean.numel() // groups
    assert mean.numel() == B * groups and var.numel() == B * groups
    for nm, t in (("gamma", gamma), ("beta", beta)):
        if t is not None:
            _dev_tensor(t, nm, torch.float32)
            assert t.numel() == C
    coef = torch.empty((B, 2, C), dtype=torch.float32, device=mean.device)
    _check(lib().mdtile_gn_coeffs(_p(mean), _p(var), _p(gamma), _p(beta), B, C, groups, eps, _p(coef), _stream()), "mdtile_gn_coeffs")
    return coef


class RecImage:
    """Split-bf16 record image of an activation [B, C, H, W] (include/mdtile.h "Record-image conv path"): the form the record
    conv kernels read by DMA.  `data` is an opaque int32 buffer of mdtile_rec_size bytes."""

    __slots__ = ("data", "shape", "fmt")

    def __init__(self, shape, device, fmt: int = REC_BF16X2):
        B, C, H, W = (int(v) for v in shape)
        n = lib().mdtile_rec_size(B, C, H, W)
        if n == 0:
            raise MdtileError(f"no record image for shape {tuple(shape)} (C % 32 == 0 required)")
        self.shape = (B, C, H, W)
        self.fmt = int(fmt)      # REC_BF16X2 | REC_F16: the form the producer wrote; the wrappers hand it to every call that reads the image
        self.data = torch.empty(n // 4, dtype=torch.int32, device=device)

    REC_COL0 = 7          # csrc/conv_rec_common.h: column of the left border record; pixel x sits at column x + 8

    @staticmethod
    def pitch(W: int) -> int:
        """records per row of a plane: W + 2 logical columns behind 7 columns of padding, rounded up to whole 128-byte lines"""
        return (int(W) + 2 + RecImage.REC_COL0 + 7) & ~7

    def records(self) -> torch.Tensor:
        """[B, 2 (hi | lo), C / 8, H + 2, W + 2, 4] int32 view of the LOGICAL image: border records included, the row padding (never
        written, never read) left out -- what two record images are compared on."""
        B, C, H, W = self.shape
        full = self.data.view(B, 2, C // 8, H + 2, RecImage.pitch(W), 4)
        return full[:, :, :, :, RecImage.REC_COL0:RecImage.REC_COL0 + W + 2, :]

    def to_f32(self) -> torch.Tensor:
        B, C, H, W = self.shape
        out = torch.empty(self.shape, dtype=torch.float32, device=self.data.device)
        _check(lib().mdtile_rec_to_f32_fmt(_p(self.data), _p(out), B, C, H, W, self.fmt, _stream()), "mdtile_rec_to_f32_fmt")
        return out


def rec_from_f32(x: torch.Tensor, coef: Optional[torch.Tensor] = None) -> RecImage:
    """split(silu(a x + s)) with coef = gn_coeffs(...) [B, 2, C], or split(x) when coef is None.  In PRECISION_F16 an activated record is
    written in its fp16 form (RecImage.fmt == REC_F16)."""
    _dev_tensor(x, "x", torch.float32)
    B, C, H, W = x.shape
    rec = RecImage(x.shape, x.device, _act_rec_fmt(coef))
    if coef is not None:
        _dev_tensor(coef, "coef", torch.float32)
        assert tuple(coef.shape) == (B, 2, C)
    _check(lib().mdtile_rec_from_f32_fmt(_p(x), _p(coef), _p(rec.data), B, C, H, W, rec.fmt, _stream()), "mdtile_rec_from_f32_fmt")
    return rec


def _act_rec_fmt(coef) -> int:
    """The form a producer writes now: an activated record (coef given) is fp16 in PRECISION_F16, everything else a bf16 split."""
    return REC_F16 if coef is not None and get_precision() == PRECISION_F16 else REC_BF16X2


def silu(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _dev_tensor(x, "x", torch.float32)
    out = torch.empty_like(x) if out is None else out
    _check(lib().mdtile_silu(_p(x), _p(out), x.numel(), _stream()), "mdtile_silu")
    return out


def tanh(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decoder.tanh_out (the queue's last task, scripts/tilevae.py:192-193)."""
    _dev_tensor(x, "x", torch.float32)
    out = torch.empty_like(x) if out is None else out
    _check(lib().mdtile_tanh(_p(x), _p(out), x.numel(), _stream()), "mdtile_tanh")
    return out


def add(a: torch.Tensor, b: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _dev_tensor(a, "a", torch.float32)
    _dev_tensor(b, "b", torch.float32)
    assert a.shape == b.shape
    out = torch.empty_like(a) if out is None else out
    _check(lib().mdtile_add(_p(a), _p(b), _p(out), a.numel(), _stream()), "mdtile_add")
    return out


class PackedConv:
    """Weights of one nn.Conv2d (1x1 or 3x3, stride 1, 'same' padding) re-laid out once for the MFMA conv kernel."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], attn_proj: bool = False):
        """attn_proj: the conv is q / k / v / proj_out of the attention (a 1x1 conv): in PRECISION_F16 it follows the attention's one-term bf16
        arithmetic (CONV_ATTN_PROJ); every other 1x1 conv reads the raw stream and keeps three terms.  No effect in the other modes."""
        _dev_tensor(weight, "weight", torch.float32)
        self.attn_proj = bool(attn_proj)
        self._packed_f16 = None      # fp16 weight plane of PRECISION_F16, built by packed_f16() the first time a call needs it
        self.cout, self.cin, kh, kw = weight.shape
        assert kh == kw and kh in (1, 3)
        self.ksize = kh
        n = lib().mdtile_conv_packed_size(self.cout, self.cin, self.ksize)
        self.packed = torch.empty(n, dtype=torch.float32, device=weight.device)
        _check(lib().mdtile_conv_pack(_p(weight), _p(self.packed), self.cout, self.cin, self.ksize, _stream()), "mdtile_conv_pack")
        self.bias = None if bias is None else _dev_tensor(bias.detach().contiguous(), "bias", torch.float32)
        # the record kernels fetch the bias of a whole 32-cout tile: pad narrow convs (conv_out) with zeros
        self.bias_rec = self.bias
        if self.bias is not None and self.cout % 32:
            self.bias_rec = torch.zeros((self.cout + 31) // 32 * 32, dtype=torch.float32, device=weight.device)
            self.bias_rec[:self.cout] = self.bias

    def packed_f16(self) -> torch.Tensor:
        """fp16 weight plane of PRECISION_F16 (mdtile_conv_pack_f16), built from the packed buffer the first time a call needs it."""
        w = self._packed_f16
        if w is None:
            n = lib().mdtile_conv_pack_f16_size(self.cout, self.cin, self.ksize)
            if n == 0:
                raise MdtileError(f"no fp16 kernel takes a {self.ksize}x{self.ksize} conv {self.cin} -> {self.cout}")
            w = torch.empty(n, dtype=torch.float32, device=self.packed.device)
            _check(lib().mdtile_conv_pack_f16(_p(self.packed), _p(w), self.cout, self.cin, self.ksize, _stream()), "mdtile_conv_pack_f16")
            self._packed_f16 = w
        return w

    def _rec_operands(self, x: "RecImage", yrec: Optional["RecImage"]):
        """(weights, flag bits) of a record conv call reading x and writing yrec: the forms travel with the images."""
        x16 = getattr(x, "fmt", REC_BF16X2) == REC_F16
        flags = (CONV_REC_X_F16 if x16 else 0) | (CONV_REC_Y_F16 if yrec is not None and yrec.fmt == REC_F16 else 0)
        return (self.packed_f16() if x16 else self.packed), flags

    def down2(self, x: torch.Tensor) -> torch.Tensor:
        """ldm Downsample: conv3x3 stride 2 over pad(x, right 1, bottom 1) (encoder 'downsample' task)."""
        _dev_tensor(x, "x", torch.float32)
        B, cin, H, W = x.shape
        assert cin == self.cin and self.ksize == 3 and H >= 2 and W >= 2
        y = torch.empty((B, self.cout, (H - 2) // 2 + 1, (W - 2) // 2 + 1), dtype=torch.float32, device=x.device)
        _check(lib().mdtile_conv2d_down2(_p(x), _p(self.packed), _p(self.bias), _p(y), B, self.cin, self.cout, H, W, _stream()),
               "mdtile_conv2d_down2")
        return y

    def fuses_pre_gn(self, upsample2x: bool = False, token_major: bool = False, exact: bool = False) -> bool:
        """True when this conv has a kernel that applies GroupNorm + SiLU to its input on load (mdtile_conv2d_gn)."""
        flags = (CONV_UPSAMPLE2X if upsample2x else 0) | (CONV_EXACT_F32 if exact else 0)
        return bool(lib().mdtile_conv2d_gn_supported(self.cout, self.cin, self.ksize, flags, int(token_major)))

    def takes_rec(self, upsample2x: bool = False) -> bool:
        """True when the record-image kernels (mdtile_conv2d_rec) take this conv."""
        return bool(lib().mdtile_conv2d_rec_supported(self.cout, self.cin, self.ksize, CONV_UPSAMPLE2X if upsample2x else 0))

    def call_rec(self, x: RecImage, residual: Optional[torch.Tensor] = None, upsample2x: bool = False, want_f32: bool = True,
                 want_rec: bool = False, rec_coef: Optional[torch.Tensor] = None, window: Optional[Tuple[int, int, int, int]] = None,
                 family: int = 0):
        """y = conv(x_rec) + bias (+ residual) -> (fp32 NCHW or None, RecImage or None), always that pair (the statistics-leaving form is
        call_rec_stats).  The record output is
        split(silu(a y + s)) with rec_coef = gn_coeffs(...) of the NEXT norm, or split(y) when rec_coef is None.
        window = (y0, x0, h, w) in INPUT pixels (upsample2x only; y0, x0: ints, or one int per image): the conv of that window of x,
        outputs [B, cout, 2h, 2w] (mdtile_upconv2d_rec_window: live-window narrowing of a decoder tile)."""
        B, cin, H, W = x.shape
        assert cin == self.cin and (want_f32 or want_rec)
        if window is not None:
            assert upsample2x and residual is None, "a window is taken by the upsample conv only"
            y0, x0, h, w = window
            y0 = [int(y0)] * B if isinstance(y0, int) else [int(v) for v in y0]       # one origin for every image, or one per image
            x0 = [int(x0)] * B if isinstance(x0, int) else [int(v) for v in x0]
            assert len(y0) == len(x0) == B, f"{B} images but {len(y0)} / {len(x0)} window origins"
            h, w = int(h), int(w)
            y = torch.empty((B, self.cout, 2 * h, 2 * w), dtype=torch.float32, device=x.data.device) if want_f32 else None
            yr = RecImage((B, self.cout, 2 * h, 2 * w), x.data.device, _act_rec_fmt(rec_coef)) if want_rec else None
            if rec_coef is not None:
                _dev_tensor(rec_coef, "rec_coef", torch.float32)
                assert want_rec and tuple(rec_coef.shape) == (B, 2, self.cout)
            wts, fmt_flags = self._rec_operands(x, yr)
            _check(lib().mdtile_upconv2d_rec_window(_p(x.data), _p(wts), _p(self.bias_rec), _p(y), None if yr is None else _p(yr.data),
                                                    _p(rec_coef), B, self.cin, self.cout, H, W, (c_int * B)(*y0), (c_int * B)(*x0), h, w, int(family) | fmt_flags, _stream()),
                   "mdtile_upconv2d_rec_window")
            return y, yr
        if upsample2x:
            H, W = 2 * H, 2 * W
        y = torch.empty((B, self.cout, H, W), dtype=torch.float32, device=x.data.device) if want_f32 else None
        yr = RecImage((B, self.cout, H, W), x.data.device, _act_rec_fmt(rec_coef)) if want_rec else None
        if residual is not None:
            _dev_tensor(residual, "residual", torch.float32)
            assert tuple(residual.shape) == (B, self.cout, H, W)
        if rec_coef is not None:
            _dev_tensor(rec_coef, "rec_coef", torch.float32)
            assert want_rec and tuple(rec_coef.shape) == (B, 2, self.cout)
        wts, fmt_flags = self._rec_operands(x, yr)
        _check(lib().mdtile_conv2d_rec(_p(x.data), _p(wts), _p(self.bias_rec), _p(residual), _p(y), None if yr is None else _p(yr.data),
                                       _p(rec_coef), B, self.cin, self.cout, H, W, (CONV_UPSAMPLE2X if upsample2x else 0) | int(family) | fmt_flags, _stream()),
               "mdtile_conv2d_rec")
        return y, yr

    def call_rec_stats(self, x: RecImage, residual: Optional[torch.Tensor] = None, upsample2x: bool = False, family: int = 0, groups: int = 32):
        """y = conv(x_rec) + bias (+ residual) as fp32 NCHW AND get_var_mean(y, groups) from the conv's own epilogue
        (mdtile_conv2d_rec_stats; leaves_stats(groups, upsample2x, rec=True) says where) -> (y, (var, mean)), always that pair."""
        B, cin, H, W = x.shape
        assert cin == self.cin
        if upsample2x:
            H, W = 2 * H, 2 * W
        y = torch.empty((B, self.cout, H, W), dtype=torch.float32, device=x.data.device)
        if residual is not None:
            _dev_tensor(residual, "residual", torch.float32)
            assert tuple(residual.shape) == (B, self.cout, H, W)
        mean, var, ws = self._stats_buffers(B, H, W, int(groups), x.data.device)
        wts, fmt_flags = self._rec_operands(x, None)
        _check(lib().mdtile_conv2d_rec_stats(_p(x.data), _p(wts), _p(self.bias_rec), _p(residual), _p(y), B, self.cin, self.cout, H, W,
                                             (CONV_UPSAMPLE2X if upsample2x else 0) | int(family) | fmt_flags, int(groups), _p(mean), _p(var), _p(ws),
                                             _stream()), "mdtile_conv2d_rec_stats")
        return y, (var, mean)

    def call_stats(self, x: torch.Tensor, pre_gn: torch.Tensor, residual: Optional[torch.Tensor] = None, groups: int = 32):
        """y = conv(silu(a * x + s)) (+ residual) on the fp32 hand-over kernel AND get_var_mean(y, groups) from its epilogue
        (mdtile_conv2d_gn_stats; leaves_stats(groups) says where) -> (y, (var, mean)), always that pair."""
        _dev_tensor(x, "x", torch.float32)
        _dev_tensor(pre_gn, "pre_gn", torch.float32)
        B, cin, H, W = x.shape
        assert cin == self.cin and tuple(pre_gn.shape) == (B, 2, self.cin)
        y = torch.empty((B, self.cout, H, W), dtype=torch.float32, device=x.device)
        if residual is not None:
            _dev_tensor(residual, "residual", torch.float32)
            assert residual.shape == y.shape
        mean, var, ws = self._stats_buffers(B, H, W, int(groups), x.device)
        w16 = get_precision() == PRECISION_F16      # the operand is silu(a x + s) by construction: the fp16 one-term kernel
        _check(lib().mdtile_conv2d_gn_stats(_p(x), _p(pre_gn), _p(self.packed_f16() if w16 else self.packed), _p(self.bias), _p(residual), _p(y), B, self.cin, self.cout,
                                            H, W, self.ksize, CONV_W_F16 if w16 else 0, int(groups), _p(mean), _p(var), _p(ws), _stream()), "mdtile_conv2d_gn_stats")
        return y, (var, mean)

    def leaves_stats(self, groups: int = 32, upsample2x: bool = False, rec: bool = False) -> bool:
        """True when this conv has a kernel whose epilogue also leaves the GroupNorm statistics of its output (slow mode: the producer of
        a pooled norm's input): call_stats(x, pre_gn, ...), or call_rec_stats(...) with rec=True."""
        if rec:
            return bool(lib().mdtile_conv2d_rec_stats_supported(self.cout, self.cin, self.ksize, CONV_UPSAMPLE2X if upsample2x else 0, int(groups)))
        return bool(not upsample2x and lib().mdtile_conv2d_gn_stats_supported(self.cout, self.cin, self.ksize, 0, int(groups)))

    def _stats_buffers(self, B: int, H: int, W: int, groups: int, device):
        """(mean, var) rows of one call -- fresh: the caller keeps them (GroupNormParam pools the rows of several tiles) -- and the partials
        workspace, which only lives inside the call (launches of one stream run in order): ONE buffer per (shape, device), up to ~10 MB."""
        mean = torch.empty(B * groups, dtype=torch.float32, device=device)
        key = (B, H, W, groups, str(device))
        cache = self.__dict__.setdefault("_stats_ws", {})
        if key not in cache:
            if len(cache) >= 8:
                cache.clear()
            cache[key] = torch.empty((lib().mdtile_conv_stats_ws_size(B, self.cout, H, W, groups) + 7) // 8, dtype=torch.float64, device=device)
        return mean, torch.empty_like(mean), cache[key]

    def __call__(self, x: torch.Tensor, residual: Optional[torch.Tensor] = None, upsample2x: bool = False,
                 token_major: bool = False, exact: bool = False, pre_gn: Optional[torch.Tensor] = None):
        """exact=True forces the exact-fp32 MFMA kernel; by default 3x3 convs with cin % 16 == 0 run on the split-bf16
        ("bf16x3") matrix-core kernel: fp32 accumulate, ~1e-5 relative to fp32.
        pre_gn = gn_coeffs(...) [B, 2, cin]: y = conv(silu(a * x + s)) -- GroupNorm + SiLU fused into the input staging
        (only where fuses_pre_gn() says so)."""
        _dev_tensor(x, "x", torch.float32)
        B, cin, H, W = x.shape
        assert cin == self.cin, f"conv expects {self.cin} input channels, got {cin}"
        if upsample2x:
            H, W = 2 * H, 2 * W
        shape = (B, H * W, self.cout) if token_major else (B, self.cout, H, W)
        y = torch.empty(shape, dtype=torch.float32, device=x.device)
        if residual is not None:
            _dev_tensor(residual, "residual", torch.float32)
            assert residual.shape == y.shape
        if pre_gn is not None:
            _dev_tensor(pre_gn, "pre_gn", torch.float32)
            assert tuple(pre_gn.shape) == (B, 2, self.cin) and not token_major and not upsample2x
            w16 = not exact and get_precision() == PRECISION_F16      # the operand is silu(a x + s) by construction: the fp16 one-term kernel
            _check(lib().mdtile_conv2d_gn(_p(x), _p(pre_gn), _p(self.packed_f16() if w16 else self.packed), _p(self.bias), _p(residual), _p(y), B, self.cin,
                                          self.cout, H, W, self.ksize, (CONV_EXACT_F32 if exact else 0) | (CONV_W_F16 if w16 else 0), _stream()), "mdtile_conv2d_gn")
            return y
        _check(lib().mdtile_conv2d(_p(x), _p(self.packed), _p(self.bias), _p(residual), _p(y), B, self.cin, self.cout, H, W,
                                   self.ksize, (CONV_UPSAMPLE2X if upsample2x else 0) | (CONV_EXACT_F32 if exact else 0) |
                                   (CONV_ATTN_PROJ if self.attn_proj else 0), int(token_major), _stream()), "mdtile_conv2d")
        return y


def vae_attn(q: torch.Tensor, k: torch.Tensor, v_tok: torch.Tensor, scale: float, exact: bool = False, v_channel_major: bool = False) -> torch.Tensor:
    """Single-head attention core (tile_utils/attn.py:55-70).  q,k: [B,C,T]; v_tok: [B,T,C] (or [B,C,T] with v_channel_major); returns
    [B,C,T].  Default: split-bf16 matrix-core flash kernel (fp32 accumulate / softmax, ~1e-5 relative); exact=True: fp32 MFMA."""
    _dev_tensor(q, "q", torch.float32)
    _dev_tensor(k, "k", torch.float32)
    _dev_tensor(v_tok, "v", torch.float32)
    B, C, T = q.shape
    assert k.shape == q.shape and tuple(v_tok.shape) == ((B, C, T) if v_channel_major else (B, T, C))
    out = torch.empty_like(q)
    ws_bytes = 0 if exact else lib().mdtile_vae_attn_ws_size(B, C, T)
    ws = torch.empty(max(1, (ws_bytes + 3) // 4), dtype=torch.float32, device=q.device)
    flags = (ATTN_EXACT_F32 if exact else 0) | (ATTN_V_CHANNEL_MAJOR if v_channel_major else 0)
    _check(lib().mdtile_vae_attn(_p(q), _p(k), _p(v_tok), _p(out), B, C, T, scale, flags, _p(ws), _stream()), "mdtile_vae_attn")
    return out


def v_channel_major_ok(C: int = 512, exact: bool = False) -> bool:
    """True when vae_attn(C channels) takes a channel-major v (the split-bf16 kernel; the exact-fp32 kernel wants it token-major).
    Asked of the library: the answer uses the very predicate mdtile_vae_attn dispatches on (precision mode, MDTILE_ATTN_MODE, C)."""
    return bool(lib().mdtile_vae_attn_takes_channel_major(int(C), ATTN_EXACT_F32 if exact else 0))


def vae_attn_qk(q: torch.Tensor, k: torch.Tensor, v_tok: torch.Tensor, scale: float) -> torch.Tensor:
    """Attention of a band of queries q [B,C,Tq] against keys k [B,C,Tk] / values v_tok [B,Tk,C]; returns [B,C,Tq]."""
    _dev_tensor(q, "q", torch.float32)
    _dev_tensor(k, "k", torch.float32)
    _dev_tensor(v_tok, "v", torch.float32)
    B, C, Tq = q.shape
    Tk = k.shape[2]
    assert k.shape[:2] == (B, C) and tuple(v_tok.shape) == (B, Tk, C)
    out = torch.empty_like(q)
    ws = torch.empty(max(1, (lib().mdtile_vae_attn_qk_ws_size(B, C, Tq, Tk) + 3) // 4), dtype=torch.float32, device=q.device)
    _check(lib().mdtile_vae_attn_qk(_p(q), _p(k), _p(v_tok), _p(out), B, C, Tq, Tk, scale, _p(ws), _stream()), "mdtile_vae_attn_qk")
    return out


def crop_store(tile: torch.Tensor, in_bbox, out_bbox, result: torch.Tensor, is_decoder: bool = True) -> None:
    """result[..., out_bbox] = crop_valid_region(tile) (tilevae.py:248-259, 630-632)."""
    _dev_tensor(tile, "tile", torch.float32)
    _dev_tensor(result, "result", torch.float32)
    N, C, th, tw = tile.shape
    assert result.shape[:2] == (N, C)
    ib, ob = (c_int * 4)(*in_bbox), (c_int * 4)(*out_bbox)
    _check(lib().mdtile_crop_store(_p(tile), N, C, th, tw, ib, ob, int(is_decoder), _p(result), result.shape[2], result.shape[3],
                                   _stream()), "mdtile_crop_store")


def vae_assemble(tiles: Sequence[Tuple[torch.Tensor, Sequence[int], Sequence[int]]], result: torch.Tensor, is_decoder: bool = True) -> None:
    """crop_store of every (tile, in_bbox, out_bbox) into `result`, one launch per VAE_ASSEMBLE_CHUNK tiles, on the current stream of the
    current device, which must own `result`.  A tile may live on another device: it is read through the peer mapping (enabled by the call;
    MdtileError when this device cannot read that one)."""
    _dev_tensor(result, "result", torch.float32)
    N, C, RH, RW = result.shape
    table = (_VaeTile * max(1, len(tiles)))()
    for k, (t, ib, ob) in enumerate(tiles):
        _dev_tensor(t, f"tiles[{k}]", torch.float32)
        if tuple(t.shape[:2]) != (N, C):
            raise MdtileError(f"tiles[{k}] has shape {tuple(t.shape)}, the result {tuple(result.shape)}")
        table[k] = _VaeTile(t.data_ptr(), t.shape[2], t.shape[3], (c_int * 4)(*ib), (c_int * 4)(*ob))
    _check(lib().mdtile_vae_assemble(table, len(tiles), N, C, int(is_decoder), _p(result), RH, RW, _stream()), "mdtile_vae_assemble")


def vae_assemble_blend(tiles: Sequence[Tuple[torch.Tensor, Sequence[int], Sequence[int]]], rows: int, cols: int, result: torch.Tensor, band: int,
                       is_decoder: bool = True) -> None:
    """vae_assemble with the tile borders cross-faded over `band` output px per side (include/mdtile.h: mdtile_vae_assemble_blend): the
    rows x cols tiles of one call in row-major order, each read in its padded extent.  Every pixel of `result` is written once (it need not
    be zeroed).  MdtileError, and nothing written, when the grid does not admit the band."""
    _dev_tensor(result, "result", torch.float32)
    N, C, RH, RW = result.shape
    if rows < 1 or cols < 1 or len(tiles) != rows * cols:
        raise MdtileError(f"vae_assemble_blend: {len(tiles)} tiles are no {rows} x {cols} grid")
    table = (_VaeTile * len(tiles))()
    for k, (t, ib, ob) in enumerate(tiles):
        _dev_tensor(t, f"tiles[{k}]", torch.float32)
        if tuple(t.shape[:2]) != (N, C):
            raise MdtileError(f"tiles[{k}] has shape {tuple(t.shape)}, the result {tuple(result.shape)}")
        table[k] = _VaeTile(t.data_ptr(), t.shape[2], t.shape[3], (c_int * 4)(*ib), (c_int * 4)(*ob))
    _check(lib().mdtile_vae_assemble_blend(table, int(rows), int(cols), N, C, int(is_decoder), int(band), _p(result), RH, RW, _stream()),
           "mdtile_vae_assemble_blend")


def mask_activity_u8(mask: torch.Tensor, boxes: Sequence[Sequence[int]]) -> List[int]:
    """Per box (x1, x2, y1, y2) in image px, as vae_split_tiles returns them: 1 when some byte of mask[y1:y2, x1:x2] is not zero, else 0.
    mask: uint8 [RH, RW] on the device.  One launch and one device-to-host copy of the flags; MdtileError for a box outside the mask, no box
    or more than MASK_ACTIVITY_MAX_BOXES."""
    _dev_tensor(mask, "mask", torch.uint8)
    if mask.dim() != 2:
        raise MdtileError(f"mask_activity_u8: mask {tuple(mask.shape)} is not [RH, RW]")
    flat = [int(v) for b in boxes for v in b]
    if len(flat) != 4 * len(boxes):
        raise MdtileError("mask_activity_u8: every box is (x1, x2, y1, y2)")
    d_boxes = torch.tensor(flat, dtype=torch.int32).view(-1, 4).to(mask.device)
    flags = torch.empty(max(1, len(boxes)), dtype=torch.int32, device=mask.device)
    with torch.cuda.device(mask.device):
        _check(lib().mdtile_mask_activity_u8(_p(mask), int(mask.shape[0]), int(mask.shape[1]), _p(d_boxes), len(boxes), _p(flags), _stream()),
               "mdtile_mask_activity_u8")
    return flags[:len(boxes)].cpu().tolist()


def vae_assemble_sparse(tiles: Sequence[Tuple[torch.Tensor, Sequence[int], Sequence[int]]], fill_boxes: Sequence[Sequence[int]],
                        fill: Optional[torch.Tensor], result: torch.Tensor) -> None:
    """vae_assemble (decoder) of the tiles that were decoded, and every box of fill_boxes (x1, x2, y1, y2) written from `fill` -- one uint8
    [RH, RW, C] image on the result's device, as (float)byte / 127.5 - 1 -- or with 0.0 when fill is None.  The tiles' out boxes and the
    fill boxes must partition the result: every pixel is written once (it need not be zeroed); MdtileError, and nothing written, otherwise."""
    _dev_tensor(result, "result", torch.float32)
    N, C, RH, RW = result.shape
    if fill is not None:
        _dev_tensor(fill, "fill", torch.uint8)
        if tuple(fill.shape) != (RH, RW, C) or fill.device != result.device:
            raise MdtileError(f"vae_assemble_sparse: fill {tuple(fill.shape)} on {fill.device} is not [{RH}, {RW}, {C}] on {result.device}")
    table = (_VaeTile * max(1, len(tiles)))()
    for k, (t, ib, ob) in enumerate(tiles):
        _dev_tensor(t, f"tiles[{k}]", torch.float32)
        if tuple(t.shape[:2]) != (N, C):
            raise MdtileError(f"tiles[{k}] has shape {tuple(t.shape)}, the result {tuple(result.shape)}")
        table[k] = _VaeTile(t.data_ptr(), t.shape[2], t.shape[3], (c_int * 4)(*ib), (c_int * 4)(*ob))
    flat = [int(v) for b in fill_boxes for v in b]
    if len(flat) != 4 * len(fill_boxes):
        raise MdtileError("vae_assemble_sparse: every fill box is (x1, x2, y1, y2)")
    boxes = (c_int * max(1, len(flat)))(*flat)
    _check(lib().mdtile_vae_assemble_sparse(table, len(tiles), boxes, len(fill_boxes), _p(fill), N, C, _p(result), RH, RW, _stream()),
           "mdtile_vae_assemble_sparse")


def enable_peer_access(device: int, peer: int) -> None:
    """Kernels running on `device` may read memory of `peer` afterwards (idempotent); MdtileError when the hardware cannot."""
    _check(lib().mdtile_enable_peer_access(int(device), int(peer)), "mdtile_enable_peer_access")


def vae_fast_input(z: torch.Tensor, tile_size: int) -> torch.Tensor:
    """Fast-mode estimator input (tilevae.py:545-559): downsample to <= tile_size, re-standardise, clamp."""
    _dev_tensor(z, "z", torch.float32)
    N, C, H, W = z.shape
    oh, ow = c_int(), c_int()
    _check(lib().mdtile_vae_fast_size(H, W, int(tile_size), ctypes.byref(oh), ctypes.byref(ow)), "mdtile_vae_fast_size")
    out = torch.empty((N, C, oh.value, ow.value), dtype=torch.float32, device=z.device)
    ws = torch.empty((lib().mdtile_vae_fast_ws_size(C) + 7) // 8, dtype=torch.float64, device=z.device)
    _check(lib().mdtile_vae_fast_input(_p(z), N, C, H, W, int(tile_size), _p(out), _p(ws), _stream()), "mdtile_vae_fast_input")
    return out


# ---- DemoFusion (tile_methods/demofusion.py:219-324) -----------------------------------------------------------------------
class WindowSet:
    """The jittered local windows of one DemoFusion phase on the device: origins (row-major over rows x cols), their nominal
    (un-jittered) grid and the jitter range J (every origin lies in [nominal, nominal + 2 J])."""

    def __init__(self, origins: Sequence[Tuple[int, int]], nomx: Sequence[int], nomy: Sequence[int], jitter: int, window: int, device):
        assert len(origins) == len(nomx) * len(nomy)
        self.rows, self.cols, self.jitter, self.window = len(nomy), len(nomx), int(jitter), int(window)
        self.origins = [(int(x), int(y)) for x, y in origins]
        self.xy = torch.tensor([v for o in self.origins for v in o], dtype=torch.int32, device=device)
        self.nomx = torch.tensor([int(v) for v in nomx], dtype=torch.int32, device=device)
        self.nomy = torch.tensor([int(v) for v in nomy], dtype=torch.int32, device=device)


def window_blend(tiles: torch.Tensor, ws: WindowSet, N: int, C: int, Hp: int, Wp: int) -> torch.Tensor:
    """Count-averaged sum of the window outputs (demofusion.py:244-257).  tiles [T*N, C, window, window], tile-major."""
    _dev_tensor(tiles, "tiles")
    assert tuple(tiles.shape) == (ws.rows * ws.cols * N, C, ws.window, ws.window)
    out = torch.empty((N, C, Hp, Wp), dtype=tiles.dtype, device=tiles.device)
    _check(lib().mdtile_window_blend(dtype_code(tiles.dtype), _p(tiles), _p(out), _p(ws.xy), _p(ws.nomx), _p(ws.nomy), ws.rows, ws.cols, ws.jitter,
                                     ws.window, N, C, Hp, Wp, _stream()), "mdtile_window_blend")
    return out


def dilated_gather(x: torch.Tensor, x_filtered: Optional[torch.Tensor], num_from_x: int, cells: Sequence[Tuple[int, int]], S: int, jitter: int,
                   h0: int, w0: int) -> torch.Tensor:
    """cat([src[:, :, by+J:Wp-J:S, bx+J:Wp-J:S] for (bx, by) in cells]) with src = x for the first num_from_x cells, x_filtered after."""
    _dev_tensor(x, "x")
    N, C, Hp, Wp = x.shape
    if x_filtered is not None:
        _dev_tensor(x_filtered, "x_filtered", x.dtype)
        assert x_filtered.shape == x.shape
    flat = (c_int * (2 * len(cells)))(*[int(v) for c in cells for v in c])
    out = torch.empty((len(cells) * N, C, h0, w0), dtype=x.dtype, device=x.device)
    _check(lib().mdtile_dilated_gather(dtype_code(x.dtype), _p(x), _p(x_filtered), int(num_from_x), _p(out), flat, len(cells), N, C, Hp, Wp, int(S),
                                       int(jitter), int(h0), int(w0), _stream()), "mdtile_dilated_gather")
    return out


def demofusion_combine(x_local: torch.Tensor, global_out: torch.Tensor, S: int, jitter: int, mixture: bool, c2: float) -> torch.Tensor:
    """x_local * (1 - c2) + scatter(global_out) * c2 (demofusion.py:284-322).  global_out [cells*N, C, h0, w0] in cell-list order."""
    _dev_tensor(x_local, "x_local")
    _dev_tensor(global_out, "global_out", x_local.dtype)
    N, C, Hp, Wp = x_local.shape
    h0, w0 = global_out.shape[2:]
    assert global_out.shape[0] == S * S * N * (2 if mixture else 1)
    out = torch.empty_like(x_local)
    _check(lib().mdtile_demofusion_combine(dtype_code(x_local.dtype), _p(x_local), _p(global_out), _p(out), N, C, Hp, Wp, int(S), int(jitter), h0, w0,
                                           int(bool(mixture)), float(c2), _stream()), "mdtile_demofusion_combine")
    return out


def depthwise_blur(x: torch.Tensor, kernel2d: torch.Tensor) -> torch.Tensor:
    """F.conv2d(x, kernel2d[None, None].repeat(C, 1, 1, 1), padding=K // 2, groups=C)  (demofusion.py:173-178)."""
    _dev_tensor(x, "x")
    _dev_tensor(kernel2d, "kernel2d", torch.float32)
    N, C, H, W = x.shape
    K = kernel2d.shape[-1]
    assert tuple(kernel2d.shape) == (K, K) and K % 2 == 1
    out = torch.empty_like(x)
    _check(lib().mdtile_depthwise_blur(dtype_code(x.dtype), _p(x), _p(kernel2d), _p(out), N * C, H, W, K, _stream()), "mdtile_depthwise_blur")
    return out


def moments(x: torch.Tensor) -> torch.Tensor:
    """fp64 [2] = (mean, unbiased std) of the whole tensor, on the device, without a host sync (two-stage fp64 sums of mdtile_gn_sums)."""
    xf = x if x.dtype == torch.float32 else x.float()
    n = xf.numel()
    sums = gn_sums(xf.contiguous().view(1, 1, 1, n), 0, 1, groups=1)[0]          # (sum, sum of squares)
    mean = sums[0] / n
    var = (sums[1] - sums[0] * sums[0] / n) / (n - 1)
    return torch.stack([mean, torch.sqrt(torch.clamp(var, min=0.0))])


def restandardize(x: torch.Tensor, stats4: torch.Tensor) -> torch.Tensor:
    """(x - stats4[0]) / stats4[1] * stats4[3] + stats4[2]; stats4 fp32 [4] on the device."""
    _dev_tensor(x, "x")
    _dev_tensor(stats4, "stats4", torch.float32)
    out = torch.empty_like(x)
    _check(lib().mdtile_restandardize(dtype_code(x.dtype), _p(x), _p(stats4), _p(out), x.numel(), _stream()), "mdtile_restandardize")
    return out


# ---- multi-GPU -------------------------------------------------------------------------------------------------------
class Shard:
    """Shard context of the C ABI (include/mdtile.h "Multi-GPU"): one RCCL communicator + one stream per local rank.
    Shard(dev_ids=[0, 1, ...])            single process, one rank per device (the form usable inside a webui process)
    Shard(nranks=N, rank=r, uid=bytes)    one rank of a process-per-GPU job; uid = Shard.unique_id() of rank 0, distributed by the host"""

    def __init__(self, dev_ids: Optional[Sequence[int]] = None, nranks: int = 0, rank: int = 0, uid: Optional[bytes] = None,
                 device: Optional[int] = None):
        L = lib()
        if dev_ids is not None:
            arr = (c_int * len(dev_ids))(*[int(d) for d in dev_ids])
            self._h = L.mdtile_shard_init(len(dev_ids), arr)
            self.devices = [int(d) for d in dev_ids]
        else:
            assert uid is not None and len(uid) == 128
            dev = torch.cuda.current_device() if device is None else int(device)
            self._uid = ctypes.create_string_buffer(bytes(uid), 128)
            self._h = L.mdtile_shard_init_rank(int(nranks), int(rank), self._uid, dev)
            self.devices = [dev]
        if not self._h:
            raise MdtileError("mdtile_shard_init: " + L.mdtile_last_error().decode(errors="replace"))
        info = (c_int * 4)()
        _check(L.mdtile_shard_info(self._h, info), "mdtile_shard_info")
        self.nranks, self.nlocal, self.first, self.rccl = info[0], info[1], info[2], bool(info[3])

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(128)
        _check(lib().mdtile_shard_unique_id(buf), "mdtile_shard_unique_id")
        return buf.raw

    @staticmethod
    def probe(nranks: int, rank: int, uid: bytes, device: int, timeout_s: float = 60.0) -> None:
        """Interruptible bring-up probe (mdtile_shard_probe_rank): the rendezvous of a process-per-GPU communicator on a non-blocking
        communicator that is aborted on the deadline and thrown away on success.  Raises MdtileError (timeout included); never leaves
        the calling thread inside RCCL.  `uid` must be an id of its own (not the one the real communicator is built from)."""
        buf = ctypes.create_string_buffer(bytes(uid), 128)
        _check(lib().mdtile_shard_probe_rank(int(nranks), int(rank), buf, int(device), float(timeout_s)), "mdtile_shard_probe_rank")

    def _streams(self, streams):
        if streams is None:
            return None
        return (c_void_p * self.nlocal)(*[int(s) for s in streams])

    def stream(self, local_rank: int) -> int:
        return int(lib().mdtile_shard_stream(self._h, int(local_rank)) or 0)

    def halo_scratch(self, band_rows: Sequence[int], N: int, C: int, W: int) -> List[torch.Tensor]:
        """One scratch buffer per local rank for halo_exchange (send + receive copies of the shared slabs)."""
        arr = (c_int * len(band_rows))(*[int(v) for v in band_rows])
        out = []
        for i, dev in enumerate(self.devices):
            n = lib().mdtile_halo_scratch_bytes(self.nranks, self.first + i, arr, N, C, W)
            out.append(torch.empty(max(1, n // 4), dtype=torch.float32, device=torch.device("cuda", dev)))
        return out

    def halo_exchange(self, partials: Sequence[torch.Tensor], scratch: Sequence[torch.Tensor], band_rows: Sequence[int], streams=None) -> None:
        """In place: every partial canvas ([N,C,H,W] fp32, one per local rank) becomes complete on the rows its band touches."""
        assert len(partials) == self.nlocal == len(scratch)
        N, C, H, W = partials[0].shape
        for t in partials:
            _dev_tensor(t, "partial", torch.float32)
        pp = (c_void_p * self.nlocal)(*[t.data_ptr() for t in partials])
        ss = (c_void_p * self.nlocal)(*[t.data_ptr() for t in scratch])
        arr = (c_int * len(band_rows))(*[int(v) for v in band_rows])
        _check(lib().mdtile_halo_exchange(self._h, pp, ss, N, C, H, W, arr, self._streams(streams)), "mdtile_halo_exchange")

    def allreduce_stats(self, bufs: Sequence[torch.Tensor], streams=None) -> None:
        for t in bufs:
            _dev_tensor(t, "buf", torch.float64)
        pp = (c_void_p * self.nlocal)(*[t.data_ptr() for t in bufs])
        _check(lib().mdtile_allreduce_stats(self._h, pp, bufs[0].numel(), self._streams(streams)), "mdtile_allreduce_stats")

    def bcast(self, bufs: Sequence[torch.Tensor], root: int, streams=None) -> None:
        pp = (c_void_p * self.nlocal)(*[t.data_ptr() for t in bufs])
        _check(lib().mdtile_shard_bcast(self._h, pp, bufs[0].numel() * bufs[0].element_size(), int(root), self._streams(streams)), "mdtile_shard_bcast")

    def p2p(self, ops: Sequence[Sequence[Tuple[int, Optional[torch.Tensor], Optional[torch.Tensor]]]], streams=None) -> None:
        """Grouped point-to-point: ops[i] = [(peer rank, tensor to send or None, tensor to receive into or None), ...] of local
        rank i; every tensor contiguous on that rank's device.  One ncclGroup for the whole call."""
        assert len(ops) == self.nlocal
        arrs, keep = [], []
        for lst in ops:
            a = (_P2P * max(1, len(lst)))()
            for k, (peer, snd, rcv) in enumerate(lst):
                for nm, t in (("send", snd), ("recv", rcv)):
                    if t is not None:
                        _dev_tensor(t, nm)
                keep.append((snd, rcv))
                a[k] = _P2P(int(peer), None if snd is None else snd.data_ptr(), 0 if snd is None else snd.numel() * snd.element_size(),
                            None if rcv is None else rcv.data_ptr(), 0 if rcv is None else rcv.numel() * rcv.element_size())
            arrs.append(a)
        pp = (POINTER(_P2P) * self.nlocal)(*[ctypes.cast(a, POINTER(_P2P)) for a in arrs])
        cnt = (c_int * self.nlocal)(*[len(lst) for lst in ops])
        _check(lib().mdtile_shard_p2p(self._h, pp, cnt, self._streams(streams)), "mdtile_shard_p2p")

    def allgather(self, sends: Sequence[torch.Tensor], streams=None) -> List[torch.Tensor]:
        """Every rank contributes a tensor of one common shape; returns per local rank the [nranks, *shape] stack in rank order."""
        outs = []
        for t in sends:
            _dev_tensor(t, "send")
            outs.append(torch.empty((self.nranks,) + tuple(t.shape), dtype=t.dtype, device=t.device))
        ss = (c_void_p * self.nlocal)(*[t.data_ptr() for t in sends])
        rr = (c_void_p * self.nlocal)(*[t.data_ptr() for t in outs])
        _check(lib().mdtile_shard_allgather(self._h, ss, rr, sends[0].numel() * sends[0].element_size(), self._streams(streams)), "mdtile_shard_allgather")
        return outs

    def selfcheck(self, streams=None) -> None:
        """Bring-up check (all-reduce, broadcast, grouped ring send / receive, all-gather; verified on the host).  Raises on failure."""
        n = int(lib().mdtile_shard_selfcheck_bytes(self._h))
        bufs = [torch.empty(n, dtype=torch.uint8, device=torch.device("cuda", d)) for d in self.devices]
        pp = (c_void_p * self.nlocal)(*[t.data_ptr() for t in bufs])
        _check(lib().mdtile_shard_selfcheck(self._h, pp, self._streams(streams)), "mdtile_shard_selfcheck")

    def destroy(self) -> None:
        h, self._h = getattr(self, "_h", None), None
        if h and _lib is not None:
            _lib.mdtile_shard_destroy(h)

    def __del__(self):
        self.destroy()
