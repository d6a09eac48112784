/*
 * mdtile.h -- C ABI of the MI355X-native tiled-diffusion / tiled-VAE engine (libmdtile.so).
 *
 * This is the drop-in boundary below the A1111 plugin surface (SURVEY.md section 8b "inner boundary").
 * The upstream extension is pure Python and has no FFI of its own; each entry point below replaces the torch
 * op sequence at the cited upstream call site (paths relative to the upstream repo root).  The Python host
 * (multidiffusion-upscaler-for-automatic1111_amd/mdtile/) binds these with ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - plain C types only; every device buffer is owned by the caller (PyTorch), the library allocates nothing on
 *     the device except the small index tables inside an opaque plan
 *   - every launch is asynchronous on the hipStream_t passed as `stream` (void* here; NULL = default stream)
 *   - return value: 0 = ok, negative = error (see MDTILE_E_*); mdtile_last_error() gives text; nothing throws/aborts
 *   - tensors are dense NCHW; "f32"/"f16"/"bf16" I/O selected by MDTILE_DT_*; all accumulation is fp32
 *   - not re-entrant on one plan; one plan per host thread
 */
#ifndef MDTILE_H
#define MDTILE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDTILE_VERSION 100

#define MDTILE_OK 0
#define MDTILE_E_ARG (-1)      /* bad argument / unsupported shape */
#define MDTILE_E_HIP (-2)      /* HIP runtime error               */
#define MDTILE_E_LIMIT (-3)    /* compile-time capacity exceeded  */

#define MDTILE_DT_F32 0
#define MDTILE_DT_F16 1
#define MDTILE_DT_BF16 2

#define MDTILE_METHOD_MD 0     /* MultiDiffusion            (tile_methods/multidiffusion.py)      */
#define MDTILE_METHOD_MOD 1    /* Mixture of Diffusers      (tile_methods/mixtureofdiffusers.py)  */

#define MDTILE_REGION_BG 0     /* BlendMode.BACKGROUND (tile_utils/utils.py:36-39) */
#define MDTILE_REGION_FG 1     /* BlendMode.FOREGROUND */

#define MDTILE_MAX_BATCHES 320 /* tile-batch pointers carried in kernel arguments */
#define MDTILE_MAX_REGIONS 16  /* = upstream md_max_regions cap (scripts/tilediffusion.py:81) */

typedef void* mdtile_stream_t; /* hipStream_t */
typedef struct mdtile_plan mdtile_plan;

int mdtile_version(void);
const char* mdtile_last_error(void);

/* Arithmetic of the matrix-core kernels (convs, attention).  Default MDTILE_PRECISION_BF16X3: every fp32 factor is split into two
 * bf16 halves (16 significand bits), three bf16 MFMAs per product, fp32 accumulation (~1e-5 relative to fp32 end to end; the stated
 * tolerance of the path is 1e-3).  MDTILE_PRECISION_F32: exact-fp32 MFMA kernels everywhere (bit-comparable to an fp32 fmaf chain),
 * ~4x slower.  MDTILE_PRECISION_BF16: one bf16 MFMA per product, bf16_rn(a) x bf16_rn(b) (the hi halves the splitters and weight packers
 * already produce), fp32 accumulation; everything outside the matrix-core products stays fp32 (residual stream, GroupNorm statistics,
 * softmax, conv_in).  Error class of bf16 operands: ~2^-9 relative per product, ~1e-3 of the output range end to end -- the arithmetic of a
 * half-precision VAE (dtype_vae = bfloat16), at up to a third of the MFMAs.  Process-wide; env MDTILE_CONV_MODE=f32 / MDTILE_ATTN_MODE=f32
 * preset it (and win over MDTILE_PRECISION_BF16 / MDTILE_PRECISION_F16 for the kernels they cover).
 *
 * MDTILE_PRECISION_F16 (= 5; 3 and 4 stay unknown): the fast mode for an fp16 VAE (11 significand bits, the webui's default half VAE).
 *   - A 3x3 conv whose operand the library itself produces as silu(a x + s) runs as ONE fp16 MFMA per product, fp16_rn(act) x fp16_rn(w),
 *     fp32 accumulation (v_mfma_f32_32x32x16_f16).  Three cases: the input is an ACTIVATED record image in its fp16 form (below,
 *     MDTILE_CONV_REC_X_F16); the fp32 hand-over conv mdtile_conv2d_gn(_stats) is called with MDTILE_CONV_W_F16; conv_out behind norm_out
 *     (the narrow record kernel, the same flag as the first case).
 *   - Conversion: v_cvt_pk_f16_f32, round to nearest even, of the value clamped to +-65504 first: no Inf is ever written or multiplied.
 *     fp16 subnormals are operands like any other: v_mfma_f32_32x32x16_f16 multiplies subnormal A / B values as they are, it does not flush
 *     them (measured on an MI355X: a conv whose weights all lie below 2^-14 gives max |y| 8.3e-4 where flushing would give 0, 4.9e-7 of the
 *     range from the fp64 reference on the unflushed fp16 weights; tests/test_gpu_precision_f16.py), so nothing is scaled.
 *   - A conv whose operand is the raw residual stream, or one the library cannot prove normalised, runs the existing THREE-TERM bf16 kernels:
 *     the upsample convs, nin_shortcut and every other 1x1 conv outside the attention, Downsample, mdtile_conv2d, mdtile_conv2d_gn without
 *     MDTILE_CONV_W_F16, and a record conv given a bf16-split record.  (The GroupNorm behind the stream is scale-free, the stream is not:
 *     it may pass 65504.)
 *   - The attention and its q / k / v / proj_out 1x1 convs (mdtile_conv2d with MDTILE_CONV_ATTN_PROJ): exactly as in MDTILE_PRECISION_BF16.
 *   - Everything outside the matrix products stays fp32: residual stream, statistics, softmax, conv_in.
 *   The route predicates (mdtile_conv2d_rec_supported, mdtile_conv2d_gn_supported, mdtile_vae_attn_takes_channel_major) answer as in the default mode. */
#define MDTILE_PRECISION_BF16X3 0
#define MDTILE_PRECISION_F32 1
#define MDTILE_PRECISION_BF16 2
#define MDTILE_PRECISION_F16 5
int mdtile_set_precision(int mode);
int mdtile_get_precision(void);

/* ----------------------------------------------------------------------------------------------------------
 * Grid planning (host integers only).
 * Replaces split_bboxes (tile_utils/utils.py:160-177) + init_grid_bbox (tile_methods/abstractdiffusion.py:173-186):
 *   tile := min(tile, canvas); overlap := max(0, min(overlap, min(tile_w_req, tile_h_req) - 4));
 *   cols = ceil((w-ov)/(tw-ov)); dx = (w-tw)/(cols-1) (double); x_c = min(int(c*dx), w-tw); rows likewise;
 *   num_batches = ceil(T/tile_bs); tile_bs := ceil(T/num_batches).
 * w,h,tile_*,overlap are in latent pixels.  The plan owns small device tables (origins, per-column / per-row
 * covering ranges) used by the gather-formulated kernels below.
 * -------------------------------------------------------------------------------------------------------- */
mdtile_plan* mdtile_plan_create(int w, int h, int tile_w, int tile_h, int overlap, int tile_bs, int clamp);
/* clamp = 1: init_grid_bbox semantics (tile and overlap clamped as above); clamp = 0: raw split_bboxes(w,h,tw,th,overlap) */
void mdtile_plan_destroy(mdtile_plan* plan);
/* info[8] = { cols, rows, num_tiles, num_batches, tile_bs, tile_w, tile_h, overlap_effective } */
int mdtile_plan_info(const mdtile_plan* plan, int* info8);
/* xywh[4*num_tiles], row-major tile order (y outer) == upstream bbox list order */
int mdtile_plan_bboxes(const mdtile_plan* plan, int* xywh);
/* The canvas closed in x (360-degree panoramas): the same plan with its tile columns laid on a circle, so that tiles span x = w-1 -> 0.
 *   tile and overlap clamp, rows, batching and tile order (row-major, y outer): as mdtile_plan_create(clamp = 1)
 *   cols = ceil(w / (tw - ov));  x_c = (int)(c * (double)w / cols);  tile c covers the columns (x_c + i) mod w, i in [0, tw)
 *   the origin stride w / cols is at most tw - ov: cyclic neighbours overlap by at least ov everywhere, the seam included
 *   effective tw >= w: NULL + mdtile_last_error (a tile would meet itself)
 * It is mdtile_plan_create_wrap(..., wrap_x = 1, wrap_y = 0) under its first name.
 * mdtile_plan_info / mdtile_plan_bboxes work on such a plan; a box reports x_c, so x_c + tw may exceed w.  mdtile_plan_wrap_x: 1 for such a plan, else 0.
 * mdtile_weight_map_add_grid, mdtile_gather, mdtile_gather_all and mdtile_blend take a wrap-x plan (the per-axis kernels of csrc/wrap.hip): column
 * indices mod w, the covering tiles summed in ascending tile index -- at a seam pixel tile column 0 before column cols-1 -- so results equal the
 * sequential `+=` loop over the tile list bit for bit.  REFUSED on a wrap-x plan (MDTILE_E_ARG, the text names the reason): num_regions > 0, any
 * MDTILE_BLEND_* flag, a row band, mdtile_gather_range, mdtile_blend_finalize, the packed destination of mdtile_gather_all, mdtile_blend_dispatch. */
mdtile_plan* mdtile_plan_create_wrap_x(int w, int h, int tile_w, int tile_h, int overlap, int tile_bs);
int mdtile_plan_wrap_x(const mdtile_plan* plan);
/* The canvas closed in y as well (seamless textures: a torus), or in y alone (a vertical strip that tiles): per-axis wrap.
 *   tile and overlap clamp, batching and tile order (row-major, y outer): as mdtile_plan_create(clamp = 1)
 *   a wrapped axis uses the circle rule of the wrap-x columns: rows = ceil(h / (th - ov));  y_r = (int)(r * (double)h / rows);  tile row r covers
 *   the rows (y_r + i) mod h, i in [0, th); a box reports y_r, so y_r + th may exceed h.  An unwrapped axis keeps the plain origins.
 *   (wrap_x, wrap_y) = (1, 0): the plan of mdtile_plan_create_wrap_x, as specified above.   (0, 0): NULL + mdtile_last_error (use mdtile_plan_create).
 *   effective tw >= w on a wrapped x, th >= h on a wrapped y: NULL + mdtile_last_error, the text names the axis.
 * mdtile_plan_wrap_x / mdtile_plan_wrap_y: 1 when that axis of the plan wraps, else 0.
 * Everything said above of a wrap-x plan holds for a plan with wrap_y: the same calls take it (both indices mod the canvas, the covering tiles
 * summed in ascending tile index -- rows outer, columns inner -- so results equal the sequential `+=` loop over the tile list bit for bit), and
 * the same calls are refused. */
mdtile_plan* mdtile_plan_create_wrap(int w, int h, int tile_w, int tile_h, int overlap, int tile_bs, int wrap_x, int wrap_y);
int mdtile_plan_wrap_y(const mdtile_plan* plan);
/* The wrapped grid displaced cyclically by (sx, sy) (a new offset every sampler step averages the tile borders out over time).
 * Displacing every tile origin of a wrap plan on the circle does not change which tile indices cover a pixel, or in which order; it moves the pixel:
 *   mdtile_gather_all_shift: tile t with plan origin (x_t, y_t) gets x_tile[ty, tx] = x_in[(y_t + sy + ty) mod h, (x_t + sx + tx) mod w]
 *                            = mdtile_gather_all on roll(x_in, (-sy, -sx))
 *   mdtile_blend_shift:      the value mdtile_blend computes for plan coordinate (y, x) -- same covering tiles in ascending tile index, d_weights /
 *                            d_rescale / d_tile_w read in PLAN coordinates, same per-term operations and epilogue, fp32 accumulation from +0.0 -- is
 *                            stored at out[(y + sy) mod h, (x + sx) mod w] = roll(mdtile_blend(...), (+sy, +sx)), bit for bit
 * No table, weight map or reciprocal map is rebuilt for a shift.  0 <= sx < w, 0 <= sy < h; (0, 0) equals the unshifted calls bitwise.
 * REFUSED (MDTILE_E_ARG, the text names the reason, nothing is written): a plain plan, a sparse plan, a shift out of range, a non-zero shift on
 * an axis that does not wrap, and everything mdtile_gather_all / mdtile_blend refuse on a wrap plan (no regions exist in this call). */
int mdtile_gather_all_shift(const mdtile_plan* plan, int dtype, int N, int C, const void* d_x_in, void* const* batch_ptrs,
                            int num_batches, int sx, int sy, mdtile_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * Weight maps (init time, device).
 * -------------------------------------------------------------------------------------------------------- */
/* gaussian_weights (tile_utils/utils.py:180-194): d_out[tile_h*tile_w] fp32; profile evaluated in fp64, var=0.01,
 * both axes normalised by tile_w^2, x midpoint (tile_w-1)/2, y midpoint tile_h/2. */
int mdtile_gaussian_weights(int tile_w, int tile_h, float* d_out, mdtile_stream_t stream);
/* feather_mask (tile_utils/utils.py:196-214): d_out[h*w] fp32. */
int mdtile_feather_mask(int w, int h, double ratio, float* d_out, mdtile_stream_t stream);
/* Grid weight map: the `weight[bbox.slicer] += init_weight` loop of split_bboxes (utils.py:164-175) followed by
 * `self.weights += weights` (abstractdiffusion.py:181-182).  d_tile_w == NULL -> uniform 1.0 (MultiDiffusion),
 * else the [tile_h, tile_w] Gaussian (Mixture of Diffusers).  d_weights[h*w] is updated in place. */
int mdtile_weight_map_add_grid(const mdtile_plan* plan, const float* d_tile_w, float* d_weights, mdtile_stream_t stream);
/* Region contribution: `self.weights[bbox.slicer] += 1.0` (multidiffusion.py:44-46, d_rect_w == NULL, scalar used) or
 * `+= gaussian_weights(bbox.w, bbox.h)` (mixtureofdiffusers.py:50-53).  Canvas is [H, W]. */
int mdtile_weight_map_add_rect(float* d_weights, int W, int H, int x, int y, int w, int h, const float* d_rect_w,
                               float scalar, mdtile_stream_t stream);
/* rescale_factor = 1 / weights (mixtureofdiffusers.py:32); inf where weights == 0, as upstream. */
int mdtile_reciprocal(const float* d_in, float* d_out, size_t n, mdtile_stream_t stream);
/* custom_weights[i] *= rescale_factor[bbox.slicer] (mixtureofdiffusers.py:34-36); d_rect_w[h*w] in place. */
int mdtile_rect_mul_canvas(float* d_rect_w, const float* d_canvas, int W, int H, int x, int y, int w, int h,
                           mdtile_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * Tile gather (K2): x_tile[i*N + n, c, :, :] = x_in[n, c, y_i:y_i+th, x_i:x_i+tw]  (tile-major batch layout)
 * Replaces `torch.cat([x_in[bbox.slicer] for bbox in bboxes], dim=0)` (multidiffusion.py:155,
 * mixtureofdiffusers.py:88,104).  mdtile_gather_all fills every batch in ONE launch (batch_ptrs[num_batches]).
 * -------------------------------------------------------------------------------------------------------- */
int mdtile_gather(const mdtile_plan* plan, int dtype, int N, int C, const void* d_x_in, int batch_id, void* d_x_tile,
                  mdtile_stream_t stream);
int mdtile_gather_all(const mdtile_plan* plan, int dtype, int N, int C, const void* d_x_in, void* const* batch_ptrs,
                      int num_batches, mdtile_stream_t stream);
/* Tiles [tile_lo, tile_hi) only, into ONE packed buffer laid out as [T*N, C, th, tw] (tile t at row t*N): the multi-GPU
 * path gathers just the rank's band of tile rows. */
int mdtile_gather_range(const mdtile_plan* plan, int dtype, int N, int C, const void* d_x_in, void* d_packed, int tile_lo,
                        int tile_hi, mdtile_stream_t stream);
/* Arbitrary-rect gather for custom regions: `x_in[bbox.slicer]` (multidiffusion.py:184, mixtureofdiffusers.py:140). */
int mdtile_gather_rect(int dtype, int N, int C, int W, int H, const void* d_x_in, int x, int y, int w, int h,
                       void* d_out, mdtile_stream_t stream);
/* Plain streaming copy of `bytes` bytes (16-byte accesses, one KiB per wave-instruction; both pointers 16-byte aligned, bytes % 16 == 0),
 * launched like the blend (one grid over the buffer, same stream).  Nothing upstream corresponds to it: it is the measurement
 * floor bench.py prints beside the blend kernel (`roofline_blend.copy_floor_us`: the same number of HBM bytes moved with no
 * table hop, no tile walk and no arithmetic), and a device-to-device copy for callers that have no torch at hand. */
int mdtile_stream_copy(const void* d_src, void* d_dst, size_t bytes, mdtile_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * Overlap blend (K3..K7), gather-formulated: one thread owns output pixels, sums the covering tile values in
 * upstream's tile order (so fp32 results are bit-identical to the sequential `+=` loop), then applies the
 * method's epilogue.  ONE launch per model evaluation.
 *
 *   MD  (multidiffusion.py:147-216):  buf = sum_tiles out_t (+ sum_bg out_r);  x = weights > 1 ? buf / weights : buf
 *   MoD (mixtureofdiffusers.py:74-175): buf = sum_tiles out_t * (tile_w * rescale[slicer]) (+ sum_bg out_r * cw_r)
 *   both: foreground regions: fbuf += out_r, fmask += feather_r, fcnt += 1; averaged where fcnt > 1;
 *         x = fcnt > 0 ? x * (1 - fmask) + fbuf * fmask : x
 *
 * batch_out[b] : device pointer to the model output of tile batch b, [nb_b*N, C, tile_h, tile_w] (tile-major)
 *                num_batches == 0  <=>  draw_background == False (abstractdiffusion.py:199-201)
 * regions      : in upstream list order
 * flags        : MDTILE_BLEND_PARTIAL = write raw partial sums (buf only, no epilogue) -- the multi-GPU path sums
 *                partials across ranks and then calls mdtile_blend_finalize.
 * -------------------------------------------------------------------------------------------------------- */
typedef struct mdtile_region {
    int x, y, w, h;
    int mode;            /* MDTILE_REGION_BG | MDTILE_REGION_FG */
    int _pad;
    const void* out;     /* model output for the region, [N, C, h, w], dtype as the call */
    const float* weight; /* BG+MoD: pre-multiplied custom weight [h,w]; FG: feather mask [h,w]; BG+MD: NULL */
} mdtile_region;

#define MDTILE_BLEND_PARTIAL 1
#define MDTILE_BLEND_TILE_RANGE 2 /* only tiles with tile_lo <= index < tile_hi contribute (row-band sharding) */
#define MDTILE_BLEND_PACKED 4     /* batch_out[0] is ONE packed buffer [T*N, C, th, tw] holding every tile (any T) */

typedef struct mdtile_blend_args {
    int method;                  /* MDTILE_METHOD_* */
    int dtype;                   /* MDTILE_DT_* of batch_out / region out / x_out */
    int N, C;
    int flags;
    int tile_lo, tile_hi;        /* with MDTILE_BLEND_TILE_RANGE */
    int row_lo, row_hi;          /* canvas rows to produce [row_lo,row_hi); 0,0 = all */
    const float* d_weights;      /* MD : [H,W] weight-sum map                                        */
    const float* d_tile_w;       /* MoD: [tile_h, tile_w] Gaussian                                    */
    const float* d_rescale;      /* MoD: [H,W] 1/weights                                              */
    void* d_x_out;               /* [N,C,H,W]; with PARTIAL: fp32 [N,C,H,W] raw sums                  */
} mdtile_blend_args;

int mdtile_blend(const mdtile_plan* plan, const mdtile_blend_args* args, const void* const* batch_out, int num_batches,
                 const mdtile_region* regions, int num_regions, mdtile_stream_t stream);
/* mdtile_blend on a wrap plan with the grid displaced by (sx, sy): specified with mdtile_gather_all_shift above. */
int mdtile_blend_shift(const mdtile_plan* plan, const mdtile_blend_args* args, const void* const* batch_out, int num_batches,
                       int sx, int sy, mdtile_stream_t stream);
/* Which kernel mdtile_blend launches for these arguments, and in what shape -- answered by the SAME host function the launcher calls, from
 * the plan's host tables alone (no device is touched, no GPU is needed): tests pin a geometry to the code path it was written for.
 *   flags = the MDTILE_BLEND_* of the call; num_batches as for mdtile_blend (0 = no grid); ptrs_aligned16 = every batch pointer (the packed
 *   buffer's with MDTILE_BLEND_PACKED) is 16-byte aligned; row_lo, row_hi as in mdtile_blend_args.
 *   info8 = { kernel, planes per thread (k_blend) / per block (k_blend_lds), candidates per chunk G (k_blend) / quads per strip SQ
 *             (k_blend_lds), LDS bytes per block, most tile columns staged per strip,
 *             k_blend only: quads (4 px of a row) on the 16-byte vector loads, on the per-element loads, on the generic walk } */
#define MDTILE_BLEND_KERNEL_PLAIN 0 /* k_blend: tile values global -> registers */
#define MDTILE_BLEND_KERNEL_LDS 1   /* k_blend_lds: tile row segments staged in LDS by DMA */
int mdtile_blend_dispatch(const mdtile_plan* plan, int dtype, int N, int C, int flags, int num_batches, int ptrs_aligned16, int row_lo,
                          int row_hi, int* info8);
/* Epilogue on summed partials (multi-GPU): MD divide + FG composite, identical math to mdtile_blend's tail.
 * d_partial fp32 [N,C,H,W]; FG regions are re-read from `regions`. */
int mdtile_blend_finalize(const mdtile_plan* plan, const mdtile_blend_args* args, const float* d_partial,
                          const mdtile_region* regions, int num_regions, mdtile_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * Custom regions on a wrap-around canvas (csrc/wrap_regions.hip, the blend kernel in csrc/wrap.hip).  Nothing upstream corresponds to it.  A rectangle (x, y, w, h)
 * on a canvas W x H with flags (wrap_x, wrap_y) covers the canvas pixels ((y + i) mod H, (x + j) mod W), i in [0, h), j in [0, w); it has ONE
 * origin and one dense [h, w] (or [N, C, h, w]) tensor whether or not it crosses a seam.  Valid iff 0 <= x < W, 0 <= y < H, 0 < w <= W,
 * 0 < h <= H, and x + w <= W unless wrap_x, y + h <= H unless wrap_y.  Canvas pixel (yc, xc) is covered iff ry = (yc - y) mod H < h and
 * rx = (xc - x) mod W < w, and then reads the rectangle's tensor at off = ry * w + rx.  Since w <= W and h <= H no pixel is covered twice by one
 * rectangle.  mdtile_blend, mdtile_blend_shift, mdtile_blend_finalize and the plain rect calls are unchanged and keep their refusals: regions on a
 * wrap plan go through the calls below only.
 *
 * mdtile_gather_rect_wrap:         out[n, c, i, j] = x_in[n, c, (y + i) mod H, (x + j) mod W], copied as bits (dtype = MDTILE_DT_*).  A rectangle inside
 *                                  the canvas: mdtile_gather_rect.
 * mdtile_weight_map_add_rect_wrap: weights[(y + i) mod H, (x + j) mod W] += d_rect_w ? d_rect_w[i, j] : scalar -- mdtile_weight_map_add_rect with the
 *                                  destination taken mod the canvas; every covered pixel receives exactly one add.
 * mdtile_region_noise_wrap:        mdtile_region_noise's definition (per layer: sum + hit count over the regions in list order, averaged where the
 *                                  count > 1; background pasted where its count > 0, foreground on top) with coverage and offsets on the circle.
 * mdtile_blend_wrap_regions:       plan = a wrap plan (mdtile_plan_create_wrap); batch_out / num_batches as mdtile_blend (0 = no grid is drawn); wr:
 *     regions      canvas coordinates, list order; .out [N, C, h, w] in args->dtype; .weight [h, w] fp32: FG = the feather mask; BG + Mixture of
 *                  Diffusers = the region's RAW Gaussian -- NOT premultiplied by a reciprocal map as mdtile_blend takes it: the kernel multiplies it
 *                  by this pixel's reciprocal; BG + MultiDiffusion: unused, may be NULL
 *     d_grid_w     [H, W] fp32 in PLAN coordinates: the grid's weight sum (mdtile_weight_map_add_grid on zeros; d_tile_w NULL for MultiDiffusion, the
 *                  Gaussian for Mixture of Diffusers); NULL iff num_batches == 0
 *     d_region_w   [H, W] fp32 in CANVAS coordinates: the BG regions' weight sum (mdtile_weight_map_add_rect_wrap on zeros in list order, scalar 1.0 for
 *                  MultiDiffusion, the raw Gaussians for Mixture of Diffusers); required, all zeros when there is no BG region
 *     sx, sy       the grid's shift as in mdtile_blend_shift; (0, 0) = the grid at rest
 *   Two maps because the grid's map travels with the shift while the regions stay on the canvas: their sum is another one every step.
 *   args->d_weights and args->d_rescale must be NULL (the kernel forms the total and its reciprocal); d_tile_w is required for Mixture of Diffusers
 *   when num_batches > 0; flags = 0, row_lo = row_hi = 0.
 *   For canvas pixel (yc, xc), plan pixel (yp, xp) = ((yc - sy) mod H, (xc - sx) mod W) and plane (n, c), in fp32 without contraction (half I/O: fp32
 *   arithmetic on the dtype-rounded inputs, rounded once at the store):
 *     wsum = (d_grid_w ? d_grid_w[yp, xp] : 0.0f) + d_region_w[yc, xc];     MoD: resc = 1.0f / wsum (IEEE division; inf at 0, never multiplied there)
 *     buf  = +0.0;  the grid tiles covering (yp, xp) in ascending tile index, as mdtile_blend on the plan:  MD buf += v;  MoD buf += v * (tile_w[ty, tx] * resc)
 *            then the BG regions covering (yc, xc) in list order:                                           MD buf += v_r;  MoD buf += v_r * (R.weight[off] * resc)
 *     MD:    x = wsum > 1 ? buf / wsum : buf;        MoD: x = buf
 *     FG:    fbuf += v_r, fmask += R.weight[off], fcnt += 1 over the covering FG regions in list order; fbuf and fmask divided by fcnt where fcnt > 1;
 *            x = x * (1 - fmask) + fbuf * fmask where fcnt > 0
 *   Every canvas pixel is written exactly once.  With num_regions = 0 and d_region_w all zeros the result equals mdtile_blend_shift with the plan's own
 *   maps bit for bit (at shift 0: mdtile_blend).  MultiDiffusion's weight sums are small integers, so gw + (c1 + c2) equals the running `+=` of the
 *   plain path exactly; for Mixture of Diffusers the grouping gw + (c1 + c2) can differ from (gw + c1) + c2 in the last bit where two or more BG
 *   regions overlap -- this grouping is the definition here, so that the grid at rest and the shifted grid are one definition.
 * REFUSED (MDTILE_E_ARG, the text names the reason, nothing is written): a rectangle that is not valid as above (w > W, h > H, x or y off the
 *   canvas, past an edge on an axis whose flag is 0); for the blend also: a sparse plan, a plain plan, a shift out of range or non-zero on an axis
 *   that does not wrap, more than MDTILE_MAX_REGIONS regions (the noise call too), any MDTILE_BLEND_* flag (MDTILE_BLEND_PACKED included), a row band,
 *   non-NULL d_weights / d_rescale, NULL d_region_w, d_grid_w that is not NULL iff num_batches == 0, num_batches neither 0 nor the plan's, a missing
 *   d_tile_w / region output / region weight, a bad mode, N, C, method or dtype; null pointers where one is required in every call.
 * -------------------------------------------------------------------------------------------------------- */
typedef struct mdtile_wrap_regions {
    const mdtile_region* regions; int num_regions;   /* canvas coordinates, list order; may cross a seam on a wrapping axis */
    const float* d_grid_w;    /* [H,W], PLAN coordinates: the grid's weight sum (mdtile_weight_map_add_grid on zeros); NULL iff num_batches == 0 */
    const float* d_region_w;  /* [H,W], CANVAS coordinates: the BG regions' weight sum (add_rect_wrap on zeros, list order); required */
    int sx, sy;               /* the grid's shift as in mdtile_blend_shift; 0, 0 = the grid at rest */
} mdtile_wrap_regions;
int mdtile_gather_rect_wrap(int dtype, int N, int C, int W, int H, const void* d_x_in, int x, int y, int w, int h, int wrap_x, int wrap_y,
                            void* d_out, mdtile_stream_t stream);
int mdtile_weight_map_add_rect_wrap(float* d_weights, int W, int H, int x, int y, int w, int h, const float* d_rect_w, float scalar, int wrap_x,
                                    int wrap_y, mdtile_stream_t stream);
int mdtile_region_noise_wrap(float* d_noise, int N, int C, int H, int W, const mdtile_region* regions, int num_regions, int wrap_x, int wrap_y,
                             mdtile_stream_t stream);
int mdtile_blend_wrap_regions(const mdtile_plan* plan, const mdtile_blend_args* args, const void* const* batch_out, int num_batches,
                              const mdtile_wrap_regions* wr, mdtile_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * Tile skipping (img2img inpainting): run only the grid tiles a mask touches.  Nothing upstream corresponds to it.
 *
 * mdtile_tile_activity: d_mask fp32 [planes, H, W], d_active int32[T] on the device.  active[t] = 1 iff some element of
 *   mask[:, y_t:y_t+th, x_t:x_t+tw] is not equal to zero, tested as !(v == 0.0f): NaN, denormals, negatives and fractions count, +0.0 and -0.0
 *   do not; else 0.  One launch writes every entry (no pre-clearing).  Plain plans only (a wrap or sparse plan: MDTILE_E_ARG).
 * mdtile_plan_create_subset: h_active = T host ints (non-zero = active).  The result is a SPARSE plan: the parent's geometry (w, h, tile, overlap,
 *   cols, rows, origins, covering tables -- copied: the parent may be destroyed first) plus two device tables, slot[t] = rank of tile t among the
 *   active tiles in ascending tile index or -1, and the list of active tile indices.  Batching is the usual rule on the active count Ta:
 *   num_batches = ceil(Ta / tile_bs), tile_bs := ceil(Ta / num_batches).  NULL + mdtile_last_error for Ta == 0, a wrap plan or a sparse plan as
 *   parent, num_batches > MDTILE_MAX_BATCHES.  Ta == T is allowed.  Destroyed with mdtile_plan_destroy.
 * mdtile_plan_active: returns Ta and fills ids[Ta] (ascending parent tile indices; ids may be NULL); 0 on a plan that is not sparse.
 * On a sparse plan mdtile_plan_info reports num_tiles = Ta with the new num_batches / tile_bs (cols, rows: the parent's) and mdtile_plan_bboxes
 *   lists the Ta active boxes in ascending parent index.  mdtile_gather / mdtile_gather_all fill the COMPACT batches: active tile number s (its
 *   slot) occupies rows (s mod tile_bs) * N ... of batch s / tile_bs; each tile's values are as on the parent.
 * mdtile_blend_sparse: batch_out[b] = model output of compact batch b; d_fill [N,C,H,W] of args->dtype, required.  A pixel is LIVE iff every grid
 *   tile of the parent that covers it is active.  At a live pixel the output equals, bit for bit, what mdtile_blend writes there on the parent
 *   plan given the same outputs for the active tiles (covering tiles in ascending tile index, fp32 accumulation from +0.0, MoD term
 *   out * (tile_w * rescale[y,x]), MD epilogue weights > 1 ? buf / weights : buf, rounded once; d_weights / d_rescale are the PARENT's full maps).
 *   At any other pixel the output is the bit pattern of d_fill[n,c,y,x] and no tile output is read for it.  args->flags must be 0,
 *   row_lo = row_hi = 0; there are no regions.
 * REFUSED on a sparse plan (MDTILE_E_ARG, the text names the reason): mdtile_blend, mdtile_blend_finalize, mdtile_blend_dispatch,
 *   mdtile_gather_range, mdtile_weight_map_add_grid (the weight maps belong to the parent).
 * -------------------------------------------------------------------------------------------------------- */
int mdtile_tile_activity(const mdtile_plan* plan, const float* d_mask, int planes, int* d_active, mdtile_stream_t stream);
mdtile_plan* mdtile_plan_create_subset(const mdtile_plan* parent, const int* h_active, int tile_bs);
int mdtile_plan_active(const mdtile_plan* plan, int* ids);
int mdtile_blend_sparse(const mdtile_plan* plan, const mdtile_blend_args* args, const void* const* batch_out, int num_batches,
                        const void* d_fill, mdtile_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * The jittered grid on a plain (bounded) canvas: a new tile grid every sampler step without a plan, a table or a map.  Nothing
 * upstream corresponds to it.  The grid of a step is a pure function of the integers in mdtile_lattice; the kernels take them by value.
 *
 * Per axis (x shown; y likewise with tile_h, h, sy).  Tile and overlap are clamped as mdtile_plan_create(clamp = 1) does; stride st = tw - ov.
 *   tw >= w: ONE tile at 0, the axis does not move, its shift is ignored (stored as 0).  Otherwise, for a shift s in [1, st]:
 *     u_k  = s - st + k st,  k = 0 .. K        the lattice origins, u_0 <= 0;   K = max(0, ceil((w - tw - (s - st)) / st)): the first k with u_k + tw >= w
 *     x'_k = min(max(u_k, 0), w - tw)          the box the model is run on: pushed inside the canvas, full size; strictly increasing in k
 *   s = st is the lattice at rest (u_0 = 0).  Tile k COVERS x iff u_k <= x < u_k + tw: a tile is evaluated at its pushed-in box but contributes
 *   only where its lattice box lies, so every tile border is at some u_k or u_k + tw and moves with s.  Every pixel is covered, by the contiguous
 *   range max(0, floor((x - tw - (s - st)) / st) + 1) .. min(K, floor((x - (s - st)) / st)), and 0 <= x - x'_k < tw for each covering tile.
 * Tiles are numbered row-major, y outer: t = r cols + c;  num_batches = ceil(T / tile_bs), tile_bs := ceil(T / num_batches).  T may differ by one
 * column and one row between two shifts.
 *
 * mdtile_lattice: host integers only; it owns nothing and is not destroyed.  Fill it with mdtile_lattice_make (works without a GPU); the calls
 *   below check it again (MDTILE_E_ARG for a struct that mdtile_lattice_make did not write).
 * mdtile_lattice_bboxes:     xywh[4 * num_tiles] = the pushed-in boxes (x'_c, y'_r, tile_w, tile_h) in tile order.
 * mdtile_lattice_weight_map: d_weights[h * w] fp32 := wsum (WRITTEN, not added);  wsum[y, x] = sum of w_t over the covering tiles in ascending t, fp32
 *   from +0.0;  d_tile_w == NULL: w_t = 1.0f (MultiDiffusion), else w_t = d_tile_w[y - v_r, x - u_c] read in LATTICE coordinates (v_r = lattice row
 *   origin), so that the Gaussian tapers at the moving borders (Mixture of Diffusers).
 * mdtile_gather_all_lattice: x_tile[ty, tx] = x_in[y'_r + ty, x'_c + tx], tile-major compact batches as mdtile_gather_all; one launch.
 * mdtile_blend_lattice:      covering tiles in ascending t, fp32 from +0.0, no contraction, the tile's value read at the PUSHED-IN coordinates
 *   (y - y'_r, x - x'_c):   MD  buf += v;  out = wsum > 1 ? buf / wsum : buf      MoD  buf += v * (tile_w[y - v_r, x - u_c] * (1.0f / wsum))  (IEEE
 *   division, as mdtile_reciprocal).  Half I/O: fp32 arithmetic on the dtype-rounded inputs, rounded once.  args->d_weights and args->d_rescale must be
 *   NULL (the kernel forms the weight sum itself), d_tile_w is required for MoD, flags and the row band must be 0; there are no regions.
 *   At rest on a canvas with (w - tw) % st == 0 and (h - th) % st == 0 the lattice is the plain plan, and all three calls equal
 *   mdtile_weight_map_add_grid (on zeros) / mdtile_gather_all / mdtile_blend (with the plan's own maps) on it bit for bit.
 * REFUSED (MDTILE_E_ARG, the text names the reason, nothing is written): a shift outside [1, stride] on a moving axis; num_batches != the
 *   lattice's or > MDTILE_MAX_BATCHES; non-NULL d_weights / d_rescale; flags or a row band; bad shapes (canvas, tile, N, C, dtype, null pointers,
 *   overlap == clamped tile, more than 65535 tiles in one gather).
 * -------------------------------------------------------------------------------------------------------- */
typedef struct mdtile_lattice {
    int w, h;                    /* canvas (latent px) */
    int tile_w, tile_h, overlap; /* clamped */
    int stride_x, stride_y;      /* tile - overlap (meaningful on a moving axis) */
    int sx, sy;                  /* the shift, in [1, stride] on a moving axis; 0 on an axis that does not move */
    int cols, rows, num_tiles;
    int num_batches, tile_bs;
} mdtile_lattice;
int mdtile_lattice_make(int w, int h, int tile_w, int tile_h, int overlap, int tile_bs, int sx, int sy, mdtile_lattice* lat);
int mdtile_lattice_bboxes(const mdtile_lattice* lat, int* xywh);
int mdtile_lattice_weight_map(const mdtile_lattice* lat, const float* d_tile_w, float* d_weights, mdtile_stream_t stream);
int mdtile_gather_all_lattice(const mdtile_lattice* lat, int dtype, int N, int C, const void* d_x_in, void* const* batch_ptrs, int num_batches,
                              mdtile_stream_t stream);
int mdtile_blend_lattice(const mdtile_lattice* lat, const mdtile_blend_args* args, const void* const* batch_out, int num_batches,
                         mdtile_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * Custom regions under the jittered grid (csrc/lattice.hip).  Nothing upstream corresponds to it.  The grid is the step's
 * lattice; the regions are ordinary rectangles on the canvas that stay where they are -- only the grid moves.  Region R covers pixel (y, x) iff
 * R.y <= y < R.y + R.h and R.x <= x < R.x + R.w, and then reads its tensors at off = (y - R.y) * R.w + (x - R.x).  mdtile_gather_rect,
 * mdtile_weight_map_add_rect and mdtile_region_noise serve such regions as they are.
 *
 * mdtile_blend_lattice_regions: lat, args, batch_out, num_batches as mdtile_blend_lattice (d_weights, d_rescale NULL; d_tile_w required for Mixture
 *   of Diffusers; flags and the row band 0); r:
 *     regions      list order; .out [N, C, h, w] in args->dtype; .weight [h, w] fp32: FG = the feather mask; BG + Mixture of Diffusers = the region's
 *                  RAW Gaussian -- NOT premultiplied by a reciprocal map as mdtile_blend takes it: the reciprocal changes every step, the kernel
 *                  multiplies by this pixel's; BG + MultiDiffusion: unused, may be NULL
 *     d_region_w   [H, W] fp32: the BG regions' weight sum on the canvas, made once per job -- zeros, then per BG region in list order
 *                  mdtile_weight_map_add_rect with scalar 1.0 (MultiDiffusion) or the region's Gaussian (Mixture of Diffusers); NULL iff the list
 *                  holds no BG region (a map of zeros is accepted there too)
 *   For canvas pixel (y, x) and plane (n, c), in fp32 without contraction (half I/O: fp32 arithmetic on the dtype-rounded inputs, rounded once at
 *   the store):
 *     gw   = sum of w_t over the grid tiles whose LATTICE box covers (y, x), ascending t, from +0.0: exactly mdtile_lattice_weight_map
 *     wsum = d_region_w ? gw + d_region_w[y, x] : gw;                 MoD: resc = 1.0f / wsum (IEEE division; the lattice covers every pixel: wsum > 0)
 *     buf  = +0.0;  the grid tiles in ascending t, the value read at the PUSHED-IN coordinates as mdtile_blend_lattice:
 *                                                                     MD buf += v;    MoD buf += v * (tile_w[y - v_r, x - u_c] * resc)
 *            then the BG regions covering (y, x) in list order:       MD buf += v_R;  MoD buf += v_R * (R.weight[off] * resc)
 *     MD:    out = wsum > 1 ? buf / wsum : buf;                       MoD: out = buf
 *     FG:    fbuf += v_R, fmask += R.weight[off], fcnt += 1 over the covering FG regions in list order; fbuf and fmask divided by fcnt where fcnt > 1;
 *            out = out * (1 - fmask) + fbuf * fmask where fcnt > 0
 *   Every canvas pixel is written exactly once; the part of a pushed-in tile outside its lattice box is never read.  With num_regions = 0 and
 *   d_region_w NULL or all zeros the result is mdtile_blend_lattice's bit for bit.  At rest on a canvas with (w - tw) % st == 0 and
 *   (h - th) % st == 0 the result equals mdtile_blend on the plain plan with the same regions (its maps made as the plain path makes them: add_grid
 *   on zeros, add_rect per BG region, reciprocal, rect_mul_canvas on each BG Gaussian) bit for bit -- for MultiDiffusion always (the weight sums
 *   are small integers), for Mixture of Diffusers wherever no pixel lies under two or more BG regions: there the definition gives gw + (c1 + c2)
 *   and the plain path's running sum (gw + c1) + c2, which can differ in the last bit (the grouping of mdtile_blend_wrap_regions, for its reason).
 * REFUSED (MDTILE_E_ARG, the text names the reason, nothing is written): everything mdtile_blend_lattice refuses; a NULL r; more than
 *   MDTILE_MAX_REGIONS regions; a rectangle with w < 1, h < 1, x < 0, y < 0, x + w > W or y + h > H; a mode other than BG / FG; a NULL .out; a NULL
 *   .weight on an FG region, or on a BG region with Mixture of Diffusers; a BG region together with a NULL d_region_w.
 * -------------------------------------------------------------------------------------------------------- */
typedef struct mdtile_lattice_regions {
    const mdtile_region* regions;  /* list order; BG+MD: weight NULL; BG+MoD: RAW Gaussian [h,w]; FG: feather mask [h,w] */
    int num_regions;               /* 0 .. MDTILE_MAX_REGIONS */
    const float* d_region_w;       /* [H,W] fp32: the BG regions' weight sum on the canvas; NULL iff the list holds no BG region */
} mdtile_lattice_regions;
int mdtile_blend_lattice_regions(const mdtile_lattice* lat, const mdtile_blend_args* args, const void* const* batch_out, int num_batches,
                                 const mdtile_lattice_regions* r, mdtile_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * Inpaint tile skipping under the jittered grid (csrc/lattice.hip).  Nothing upstream corresponds to it.  For a lattice `lat`
 * (fields as mdtile_lattice_make writes them) tile t = r cols + c has lattice origin (v_r, u_c) and pushed-in box (y'_r, x'_c).
 *
 * Its CONTRIBUTING box is its lattice box clipped to the canvas, [max(v_r, 0), min(v_r + th, H)) x [max(u_c, 0), min(u_c + tw, W)): the only
 *   place where the tile's output enters the blend.
 * ACTIVITY  active[t] = 1 iff some element of mask[:, contributing box of t] satisfies !(v == 0.0f), the test of mdtile_tile_activity: NaN,
 *   denormals, negatives and fractions count, +0.0 and -0.0 do not.  The test runs on the contributing box, NOT the pushed-in box: a tile pushed in
 *   from the edge is evaluated over pixels it never writes, and those do not make it active.  Every pixel with a non-zero mask lies in the
 *   contributing box of each tile that covers it, so every such pixel is live (below).
 * COMPACT NUMBERING  slot[t] = number of active t' < t if t is active, else -1;  Ta = number of active tiles;  num_batches = ceil(Ta / tile_bs
 *   requested), tile_bs := ceil(Ta / num_batches): the rule of mdtile_plan_create_subset.  Active tile number s occupies rows (s mod tile_bs) * N ...
 *   of batch s / tile_bs.
 * GATHER  the compact batches hold, for each active tile, exactly what mdtile_gather_all_lattice puts into that tile's rows: the pushed-in box,
 *   copied as bits.
 * BLEND   a pixel is LIVE iff every lattice tile that covers it is active.  At a live pixel the output is, bit for bit, what mdtile_blend_lattice
 *   writes there given the same outputs for the active tiles: covering tiles in ascending t, fp32 from +0.0, no contraction, the weight sum over all
 *   covering tiles, MD wsum > 1 ? buf / wsum : buf, MoD v * (tile_w[lattice coords] * (1.0f / wsum)), half I/O rounded once.  At any other pixel the
 *   output is the bit pattern of d_fill[n, c, y, x], and no tile output is read for it.  Every canvas pixel is written exactly once.
 *
 * mdtile_lattice_activity: d_mask fp32 [planes, H, W]; d_active, d_slot device int32[lat->num_tiles].  Two launches (the per-tile reduction, then
 *   the ranks) write every entry of both, no pre-clearing; at most 65535 tiles.
 * mdtile_lattice_subset_make: host integers only.  h_active = lat->num_tiles host ints (non-zero = active); fills *sub with the lattice, Ta and the
 *   compact batching for `tile_bs`, and keeps d_slot (caller-owned device memory, not read here).
 * mdtile_lattice_subset_bboxes: xywh[4 * Ta] = the pushed-in boxes of the active tiles, ids[Ta] = their tile indices, both in ascending t (ids may
 *   be NULL); h_active must hold exactly sub->num_active non-zero flags.
 * d_slot must hold the ranks of the same flags mdtile_lattice_subset_make was given -- from mdtile_lattice_activity, or the caller's own upload.
 *   The library cannot check that without a synchronisation, so the kernels treat any slot[t] < 0 or slot[t] >= num_active as "not active": a wrong
 *   table can give pixels that are not live (or, where two tiles claim one slot, the wrong tile's values) but never an access outside a batch.
 * mdtile_gather_all_lattice_sparse / mdtile_blend_lattice_sparse: batch_ptrs / batch_out = the sub->num_batches COMPACT batches; args as
 *   mdtile_blend_lattice; d_fill [N, C, H, W] of args->dtype, required.  One launch each.  Ta == num_tiles is allowed.
 * REFUSED (MDTILE_E_ARG, the text names the function and the reason, before any device is touched, nothing is written): everything
 *   mdtile_blend_lattice / mdtile_gather_all_lattice refuse (flags, a row band, non-NULL d_weights / d_rescale, MoD without d_tile_w, bad N / C / dtype /
 *   method, null pointers); a sub->lat that mdtile_lattice_make did not write; num_active outside 1 .. num_tiles (no active tile: nothing to run);
 *   num_batches, tile_bs that are not the rule's for num_active; num_batches different from the call's argument, or above MDTILE_MAX_BATCHES; NULL
 *   d_slot or d_fill; planes < 1 (or above 65535); more than 65535 tiles in the activity or the gather.
 * -------------------------------------------------------------------------------------------------------- */
typedef struct mdtile_lattice_subset {
    mdtile_lattice lat;          /* the step's full lattice */
    int num_active;              /* Ta, 1 .. lat.num_tiles */
    int num_batches, tile_bs;    /* of the compact batches */
    const int* d_slot;           /* device int32[lat.num_tiles], caller-owned */
} mdtile_lattice_subset;
int mdtile_lattice_activity(const mdtile_lattice* lat, const float* d_mask, int planes, int* d_active, int* d_slot, mdtile_stream_t stream);
int mdtile_lattice_subset_make(const mdtile_lattice* lat, const int* h_active, int tile_bs, const int* d_slot, mdtile_lattice_subset* sub);
int mdtile_lattice_subset_bboxes(const mdtile_lattice_subset* sub, const int* h_active, int* xywh, int* ids);
int mdtile_gather_all_lattice_sparse(const mdtile_lattice_subset* sub, int dtype, int N, int C, const void* d_x_in, void* const* batch_ptrs,
                                     int num_batches, mdtile_stream_t stream);
int mdtile_blend_lattice_sparse(const mdtile_lattice_subset* sub, const mdtile_blend_args* args, const void* const* batch_out, int num_batches,
                                const void* d_fill, mdtile_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * Free-form mask regions beside the rectangles (csrc/mask_regions.hip, the blend kernel in csrc/blend.hip).  Nothing upstream
 * corresponds to it.  A region keeps its rectangle (its bounding box: what is gathered, conditioned and evaluated) and gains a COVERAGE map,
 * [h, w] bytes: region R covers canvas pixel (yc, xc) iff the pixel lies in R's rectangle and (cover == NULL or cover[off] != 0), off = ry * w + rx.
 * Coverage is not a zero weight: upstream counts every pixel of a rectangle in fcnt and in the weight sums whatever its feather is, so two regions
 * whose boxes overlap and whose shapes do not would leak into each other at half weight.  A region that does not cover a pixel takes no part in it.
 *
 * mdtile_mask_cover_u8: a painted mask d_mask [Hm, Wm] (device bytes; Hm >= H, Wm >= W, e.g. 8192 x 8192 for H = W = 1024) -> d_cover [H, W] bytes
 *   (0 / 1) and d_box (device int32[5]).  Cell (y, x) owns mask rows [y*Hm/H, (y+1)*Hm/H) and columns [x*Wm/W, (x+1)*Wm/W) (integer division; never
 *   empty); with s the byte sum and n the pixel count of that box, cover = (2*s >= 255*n) ? 1 : 0.  d_box = {xmin, ymin, xmax+1, ymax+1, count} of the
 *   covered cells, {0,0,0,0,0} when there is none.  Two launches write every output; nothing is cleared beforehand; integers only, the same bits every
 *   run.  Limits: H * W < 2^31 and at most 2^22 mask pixels per cell.
 * mdtile_mask_region: the dense tensors of the region with rectangle (x, y, w, h) on the [H, W] coverage d_cover: d_rcover[i, j] = d_cover[y+i, x+j] != 0
 *   (bytes 0 / 1) and, unless d_feather is NULL, its feather [h, w] fp32: R = int(min(w/2, h/2) * feather_ratio) as mdtile_feather_mask forms it (integer
 *   halves, double product, truncation); for a covered cell k = the chessboard distance max(|di|, |dj|) to the nearest cell that is not covered, cells
 *   outside the rectangle counting as not covered (k >= 1); d = k - 1; feather = d >= R ? 1.0f : (float)((double)d / (double)R)^2 -- the double
 *   expression of mdtile_feather_mask; 0.0f in a cell that is not covered.  The search goes no further than R.  Chessboard and not Euclidean distance: it
 *   is integer arithmetic and so has a bitwise definition, and for a fully covered rectangle with even w and h it is upstream's feather_mask bit for bit.
 *   For odd w or h upstream leaves the middle row / column at 1.0 (a quirk of its quadrant loop); the distance form does NOT reproduce that.
 * mdtile_blend_mask_regions: mdtile_blend on a plain plan where a region enters a pixel only if it covers it: the grid tiles in ascending tile index,
 *   then the covering BG regions in list order (MD buf += v, MoD buf += v * weight[off], weight premultiplied as mdtile_blend takes it), MD's
 *   weights > 1 ? buf / weights : buf, then the composite over the covering FG regions in list order (fbuf += v, fmask += weight[off], fcnt += 1,
 *   averaged where fcnt > 1, x = x * (1 - fmask) + fbuf * fmask where fcnt > 0); fp32 without contraction, half I/O rounded once at the store.
 *   num_batches == 0: regions only.  A region's output and weight are NOT READ at a pixel it does not cover.  d_weights / d_rescale are the host's maps,
 *   made with the covers (MD: the cover as 0.0 / 1.0 through mdtile_weight_map_add_rect; MoD: gaussian * cover).  With every cover NULL or all ones the
 *   result is mdtile_blend's bit for bit.  Always the register form of the kernel (no LDS form).
 * mdtile_region_noise_masked: mdtile_region_noise with the same coverage rule; with every cover NULL it is mdtile_region_noise bit for bit.
 * REFUSED (MDTILE_E_ARG, the text names the reason, nothing is written): null required pointers; bad sizes, dtypes, methods or modes; a rectangle that
 *   leaves the canvas; more than MDTILE_MAX_REGIONS regions; and by mdtile_blend_mask_regions a wrap-around plan, a sparse plan, any MDTILE_BLEND_* flag
 *   and a row band; by mdtile_mask_cover_u8 a mask smaller than the latent canvas on either axis (Wm < W or Hm < H: a cell would own no mask pixel).
 * What mask regions are NOT combined with, each refused or set aside by name:
 *   wrap-around canvases (--mdtile-wrap-x / --mdtile-wrap-y), with or without --mdtile-wrap-regions   the plugin raises RuntimeError; this call refuses the plan
 *   Noise Inversion                                               the plugin raises RuntimeError (mdtile_noise_inverse_blend knows rectangles only)
 *   --mdtile-grid-jitter with --mdtile-jitter-regions             the fixed grid runs, one line through the jitter note (mdtile_blend_lattice_regions takes no cover)
 *   --mdtile-inpaint-skip                                         stands down as with every region job (this call refuses a sparse plan)
 *   ShardedBlend (mdtile/sharding.py, the multi-GPU blend)        refuses a region with a cover (this call refuses partial sums, tile ranges and row bands)
 *   a mask smaller than the latent canvas on either axis          the plugin raises RuntimeError before the call; the call refuses it too
 * -------------------------------------------------------------------------------------------------------- */
/* The struct has a tag and no typedef: the function mdtile_mask_region owns the plain name, so the type is written `struct mdtile_mask_region` (C and
 * C++ both keep tags apart from functions). */
struct mdtile_mask_region {
    mdtile_region r;
    const unsigned char* cover;   /* [h, w], NULL = the whole rectangle */
};
int mdtile_mask_cover_u8(const unsigned char* d_mask, int Wm, int Hm, int W, int H, unsigned char* d_cover, int* d_box, mdtile_stream_t stream);
int mdtile_mask_region(const unsigned char* d_cover, int W, int H, int x, int y, int w, int h, double feather_ratio, unsigned char* d_rcover,
                       float* d_feather /* may be NULL */, mdtile_stream_t stream);
int mdtile_blend_mask_regions(const mdtile_plan* plan, const mdtile_blend_args* args, const void* const* batch_out, int num_batches,
                              const struct mdtile_mask_region* regions, int num_regions, mdtile_stream_t stream);
int mdtile_region_noise_masked(float* d_noise, int N, int C, int H, int W, const struct mdtile_mask_region* regions, int num_regions,
                               mdtile_stream_t stream);

/* Per-region initial noise (scripts/tilediffusion.py:486-529, create_random_tensors_hijack): d_noise [N,C,H,W] fp32 is the job's
 * noise, updated in place.  regions[i].out = the region's own noise [1,C,h,w] fp32 (drawn by the host with the region's CPU
 * seed, shared by all N samples), .mode = MDTILE_REGION_BG / _FG, .weight unused.  Per layer: sum + hit count over the regions
 * in list order, averaged where count > 1; background layer pasted where its count > 0, foreground layer on top.  <= 16 regions. */
int mdtile_region_noise(float* d_noise, int N, int C, int H, int W, const mdtile_region* regions, int num_regions,
                        mdtile_stream_t stream);

/* Noise Inversion renoise composite (tile_methods/abstractdiffusion.py:651-676, inside sample_img2img):
 *   d_noise, d_inverse_noise, d_out [N,C,H,W] fp32, d_renoise_mask [H,W] fp32 (already scaled by the renoise strength and clamped).
 *   num_regions > 0 (the caller passes the custom regions only when the grid is disabled, :658): the job's noise is first re-weighted
 *   noise' = bg * (1 - fw) + fg * fw with bg = noise where a background region covers the pixel, fg / fw = hit-count averages of
 *   the noise / of the foreground regions' feather masks (.weight [h,w] fp32; .out unused), in list order.
 *   out = ((1 - m) * inverse + m * noise') / sqrt(m^2 + (1 - m)^2).   The same fp32 ops in the same order as the eager code, each
 *   correctly rounded (torch's CPU sqrt is 1 ulp off on ~1 % of inputs: that is the only possible last-bit difference).  <= 16 regions. */
int mdtile_noise_inverse_blend(const float* d_noise, const float* d_inverse_noise, const float* d_renoise_mask, float* d_out, int N, int C,
                               int H, int W, const mdtile_region* regions, int num_regions, mdtile_stream_t stream);

/* Noise Inversion renoise mask (tile_utils/utils.py:216-247, get_retouch_mask; tile_methods/abstractdiffusion.py:607-621): where the init image
 * carries detail -- the residue of a self-guided box filter (guide = input, eps 0.01), quantised to uint8 levels.  Upstream computes it with
 * OpenCV on the CPU; here the result is DEFINED, so that it can be checked bit for bit (DESIGN.md 3.9 lists the two differences from OpenCV).
 *   d_img     [H, W] grey bytes (channels = 1) or [H, W, 3] interleaved RGB bytes (channels = 3): L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16,
 *             PIL's convert("L")
 *   window    of pixel (y, x): rows y - k/2 .. y - k/2 + k - 1 and the same in x (k/2 = floor, OpenCV's default anchor); indices outside the
 *             image are mapped by BORDER_REFLECT_101, i.e. the triangle wave of period 2 (n - 1), applied as often as needed (k/2 >= n is
 *             legal; n == 1 -> 0)
 *   sums      S1 = sum of L, S2 = sum of L^2 over the window as exact integers (S2 in 64 bits): no dependence on order or block shape
 *   then, every operation ONE correctly rounded fp32 operation (no FMA), n = k^2:
 *             img  = float(L) / 255.0f
 *             mean = (float)((double)S1 / (255.0 * n))          msq = (float)((double)S2 / (65025.0 * n))
 *             var  = msq - mean * mean                          a = var / (var + 0.01f)            b = mean - a * mean
 *             gf   = ((a * img + b) - img) * 255.0f
 *             q    = ((int32)trunc(gf)) & 255                   upstream's astype(uint8): toward zero, negatives wrap
 *             mask = float(q) / 255.0f                          d_mask [H, W] fp32
 *   1 <= kernel_size <= 512, channels 1 or 3, H * W < 2^31 (anything else: MDTILE_E_ARG).  Work per pixel does not grow with the window area:
 *   horizontal window sums per row (block scan), then vertical sliding sums with a k-row start-up per chunk of rows.
 *   d_ws: mdtile_retouch_mask_ws_size(H, W, kernel_size) bytes (8 per pixel: the row sums; 0 for arguments the call would refuse), 8-byte aligned.
 * mdtile_renoise_resize: the tail of upstream :619-621, d_out [h, w] = clamp((1 - bilinear(d_mask [H, W] -> h x w)) * strength, 0, 1) with torch's
 *   align_corners = False rule in fp32, per axis:  scale = float(H) / h;  src = max(scale * (dst + 0.5) - 0.5, 0);  i0 = (int)src;
 *   i1 = min(i0 + 1, H - 1);  l1 = src - i0;  l0 = 1 - l1;    value = l0y * (l0x * p00 + l1x * p01) + l1y * (l0x * p10 + l1x * p11). */
size_t mdtile_retouch_mask_ws_size(int H, int W, int kernel_size);
int mdtile_retouch_mask(const uint8_t* d_img, int H, int W, int channels, int kernel_size, float* d_mask, void* d_ws, mdtile_stream_t stream);
int mdtile_renoise_resize(const float* d_mask, int H, int W, float strength, float* d_out, int h, int w, mdtile_stream_t stream);

/* 8-bit image resize (the img2img upscale of scripts/tilediffusion.py:141-147, which the host's Upscaler.upscale runs with Pillow on one CPU thread).
 * The result is DEFINED as Pillow's Image.resize on "RGB" / "L" images for LANCZOS and NEAREST, restated here so that it is checked bit for bit
 * (DESIGN.md 3.10).  Per axis, in -> out, a table of out rows: bounds[xx] = (first source index xmin, taps n), coef[xx][0 .. ksize-1] taps in 22-bit
 * fixed point, zero from n on.  mdtile_resample_table computes it on the HOST in double, every step one IEEE operation (sin is libm's):
 *   LANCZOS   f(x) = sinc(x) * sinc(x / 3) for -3 <= x < 3, else 0;   sinc(0) = 1, sinc(x) = sin(x * pi) / (x * pi)
 *             scale = in / out;  fs = max(scale, 1.0);  support = 3.0 * fs;  ksize = 2 * ceil(support) + 1;  ss = 1.0 / fs
 *             center = (xx + 0.5) * scale;   xmin = max((int)(center - support + 0.5), 0);   n = min((int)(center + support + 0.5), in) - xmin
 *             w[x] = f((x + xmin - center + 0.5) * ss) for x < n;   ww = w[0] + w[1] + ... in index order;   if ww != 0: w[x] /= ww
 *             coef[xx][x] = w[x] < 0 ? (int)(-0.5 + w[x] * 2^22) : (int)(0.5 + w[x] * 2^22)
 *   NEAREST   ksize = 1, coef = 2^22, bounds[xx] = ((int)xo, 1) with xo = 0.5 * a for xx = 0 and xo += a from one output to the next, a = in / out
 *             in double: the ACCUMULATED sum (the closed form (int)((xx + 0.5) * a) rounds differently and moves thousands of pixels)
 *   pixel     acc = 2^21 + sum over x < n of src[xmin + x] * coef[xx][x]   (int32, exact);    out = clamp(acc >> 22, 0, 255)
 * The horizontal pass runs first and leaves a uint8 intermediate [H, outW, C], the vertical pass runs on it; channels are independent, layout HWC
 * interleaved.  An axis whose size does not change is skipped for LANCZOS (pass NULL, NULL, 0 for its tables); NEAREST takes both tables always.
 *   mdtile_resample_ksize      ksize of one axis; 0 for arguments mdtile_resample_table refuses (a size below 1, an unknown filter, out * ksize >= 2^31)
 *   mdtile_resample_table      h_coef [out][ksize], h_bounds [out][2]: HOST pointers
 *   mdtile_resample_u8_ws_size bytes of the intermediate (H * outW * C; 0 for arguments the call would refuse)
 *   mdtile_resample_u8         d_src [H, W, C] -> d_dst [outH, outW, C] bytes at any alignment; d_cx / d_bx / kx, d_cy / d_by / ky: DEVICE copies of the
 *                              tables of (W -> outW) and (H -> outH); d_ws is read only when both axes have tables.  C is 1 or 3, every size >= 1,
 *                              H * W * C and outH * outW * C below 2^31; anything else: MDTILE_E_ARG.  The kernels are integer only: no byte depends on
 *                              block shape or summation order.  Tables from elsewhere may give other bytes, never an access outside the buffers. */
#define MDTILE_RESAMPLE_NEAREST 0
#define MDTILE_RESAMPLE_LANCZOS 1
int mdtile_resample_ksize(int in_size, int out_size, int filter);
int mdtile_resample_table(int in_size, int out_size, int filter, int32_t* h_coef, int32_t* h_bounds);
size_t mdtile_resample_u8_ws_size(int H, int W, int C, int outH, int outW);
int mdtile_resample_u8(const uint8_t* d_src, int H, int W, int C, uint8_t* d_dst, int outH, int outW, const int32_t* d_cx, const int32_t* d_bx, int kx,
                       const int32_t* d_cy, const int32_t* d_by, int ky, void* d_ws, mdtile_stream_t stream);

/* Colour fix of an img2img result against its init image (StableSR's wavelet / AdaIN colour fix, which exists upstream only as CPU float code of
 * another extension), on bytes and DEFINED here, so that it is checked bit for bit.
 * Inputs: content (the decoded result) and style (the init image), both uint8, [H, W, C] interleaved or [H, W], C in {1, 3}, the same shape,
 * H * W * C < 2^31.  Channels are independent.  Anything else: MDTILE_E_ARG.
 *   WAVELET   The literal definition works per channel on byte values as reals:
 *               blur_r(x)    the 3x3 kernel [[1,2,1],[2,4,2],[1,2,1]] / 16 with dilation r, after replicate padding by r
 *               decompose(x) for i = 0 .. 4:  low = blur_{2^i}(x);  high += x - low;  x = low
 *               out = clamp(floor(high(content) + low(style) + 1/2), 0, 255)
 *             Three steps reduce it to integers: high(content) telescopes to content - low5(content); every step is linear, so
 *             out = content + low5(style - content); the 3x3 kernel is [1,2,1] (x) [1,2,1] and operators on different axes commute, so low5 is
 *             five 1-D levels along one axis, then five along the other.  The integer form:
 *               d = style - content                                                                   (int, |d| <= 255)
 *               level k on an axis of length n, r = 2^k:
 *                   v'[i] = v[clamp(i - r, 0, n - 1)] + 2 * v[i] + v[clamp(i + r, 0, n - 1)]           (no division)
 *               after 10 levels |v| <= 255 * 2^20 < 2^28;  out = clamp((content * 2^20 + v + 2^19) >> 20, 0, 255)   (int32, arithmetic shift)
 *             No byte depends on block shape, pass order or summation order.  THE CLAMP IS PER LEVEL: padding the input once by 31 and then
 *             convolving is a different function.
 *   ADAIN     per channel and pointwise, hence a 256-entry table:
 *               mdtile_hist_u8   the exact uint32 counts [C][256] of an image, on the device
 *               on the host (mdtile.adain_lut), per channel from the counts as integers: n, S1 = sum x * count[x], S2 = sum x^2 * count[x]
 *                   mean = S1 / n
 *                   var  = (n * S2 - S1^2) / (n * (n - 1))         (integer numerator and denominator, one division; 0 when n == 1)
 *                   std  = sqrt(var + 0.65025)                     (StableSR's eps 1e-5 in [0, 1] units, times 255^2)
 *                   lut[c][x] = clamp(floor((x - mean_c) / std_c * std_s + mean_s + 1/2), 0, 255)      (float64, in the order written; _c of the
 *                                                                                                       content, _s of the style)
 *               mdtile_lut_u8    applies lut[c] to channel c, on the device
 *             AdaIN needs no resize of the style image.  A flat content channel maps through std = sqrt(0.65025) and stays finite.
 *   mdtile_colorfix_wavelet_ws_size  bytes of the int32 intermediate [H, W, C] (0 for arguments the call would refuse)
 *   mdtile_colorfix_wavelet          d_content, d_style -> d_out, bytes at any alignment; d_ws: that many bytes, 16-byte aligned
 *   mdtile_hist_u8                   d_hist [C][256] uint32 is zeroed and filled on the stream
 *   mdtile_lut_u8                    d_lut [C][256] uint8 on the device; d_out [H, W, C] */
size_t mdtile_colorfix_wavelet_ws_size(int H, int W, int C);
int mdtile_colorfix_wavelet(const uint8_t* d_content, const uint8_t* d_style, uint8_t* d_out, int H, int W, int C, void* d_ws, mdtile_stream_t stream);
int mdtile_hist_u8(const uint8_t* d_img, int H, int W, int C, uint32_t* d_hist, mdtile_stream_t stream);
int mdtile_lut_u8(const uint8_t* d_img, int H, int W, int C, const uint8_t* d_lut, uint8_t* d_out, mdtile_stream_t stream);

/* ControlNet / StableSR tile slicing (tile_methods/abstractdiffusion.py:475-544, 548-588): num_rects (<= 16) rectangles of size w x h
 * at rects_xy[2 i], rects_xy[2 i + 1] of d_x_in [N,C,H,W] are cut out, concatenated (tile-major, then the N samples: torch.cat over
 * the bboxes) and repeated `repeat` times for the sampler's cond / uncond copies:
 *   tile_major = 1: out row j * repeat + r = row j (k-diffusion, :528-533);   tile_major = 0: out row r * (num_rects * N) + j (DDIM, :535).
 * d_out [num_rects * N * repeat, C, h, w], same dtype.  Pass the latent-grid rectangles multiplied by opt_f = 8 for ControlNet hints. */
int mdtile_gather_rects(int dtype, int N, int C, int W, int H, const void* d_x_in, const int* rects_xy, int num_rects, int w, int h,
                        int repeat, int tile_major, void* d_out, mdtile_stream_t stream);

/* DemoFusion model evaluation (tile_methods/demofusion.py:219-324).  Tensors NCHW in `dtype`, fp32 accumulation; Hp x Wp is the latent padded
 * by the jitter range J on every side (forward_one_step, :201-205).
 *   mdtile_window_blend       local path (:244-257): the T = rows*cols equally sized windows (origins d_window_xy[2 w], [2 w + 1] in the padded
 *                             canvas, row-major; nominal, un-jittered origins d_nomx[cols] / d_nomy[rows]; every origin lies within
 *                             [nominal, nominal + 2 J]) are summed in list order and divided by the hit count (0 -> 1).
 *                             d_tiles [T*N, C, window, window] tile-major (the concatenated model outputs), d_out [N,C,Hp,Wp].
 *   mdtile_dilated_gather     global path, inputs (:268-283): cell i = (cells_xy[2 i], cells_xy[2 i + 1]) of the S x S lattice ->
 *                             x[:, :, by+J : Wp-J : S, bx+J : Wp-J : S]; the first num_from_x cells read d_x, the others d_x_filtered (mixture
 *                             mode); d_out [num_cells*N, C, h0, w0], cells in list order.
 *   mdtile_demofusion_combine global path, scatter + mix (:284-322): x_global = scatter of d_global_out [cells*N, C, h0, w0] back onto the lattice
 *                             (mixture: the two copies of a cell are added and halved), out = x_local * (1 - c2) + x_global * c2.
 *   mdtile_depthwise_blur     Gaussian filter (:173-178): depthwise K x K conv (odd K), zero padding, kernel [K*K] fp32 on the device.
 *   mdtile_restandardize      (x - st[0]) / st[1] * st[3] + st[2]  with st = { mean, std, target mean, target std } on the device (:264). */
int mdtile_window_blend(int dtype, const void* d_tiles, void* d_out, const int* d_window_xy, const int* d_nomx, const int* d_nomy, int rows,
                        int cols, int jitter, int window, int N, int C, int Hp, int Wp, mdtile_stream_t stream);
int mdtile_dilated_gather(int dtype, const void* d_x, const void* d_x_filtered, int num_from_x, void* d_out, const int* cells_xy, int num_cells,
                          int N, int C, int Hp, int Wp, int S, int jitter, int h0, int w0, mdtile_stream_t stream);
int mdtile_demofusion_combine(int dtype, const void* d_x_local, const void* d_global_out, void* d_out, int N, int C, int Hp, int Wp, int S,
                              int jitter, int h0, int w0, int mixture, float c2, mdtile_stream_t stream);
int mdtile_depthwise_blur(int dtype, const void* d_x, const float* d_kernel, void* d_out, int planes, int H, int W, int K, mdtile_stream_t stream);
int mdtile_restandardize(int dtype, const void* d_x, const float* d_stats4, void* d_out, size_t n, mdtile_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * Tiled VAE (scripts/tilevae.py).  All tensors fp32 NCHW.
 * -------------------------------------------------------------------------------------------------------- */
/* split_tiles + get_best_tile_size (tilevae.py:390-462).  in_bboxes/out_bboxes: [4*n] as [x1,x2,y1,y2].
 * Returns the tile count (>=1) or a negative error; pass cap = capacity in tiles (call with cap=0 to query). */
int mdtile_vae_split_tiles(int h, int w, int tile_size, int is_decoder, int* in_bboxes, int* out_bboxes, int cap);
/* VAEHook.get_best_tile_size (scripts/tilevae.py:390-403): the size split_tiles shrinks a [lowerbound, upperbound] tile to. */
int mdtile_vae_best_tile_size(int lowerbound, int upperbound);

/* get_var_mean (tilevae.py:207-215): biased var & mean per (sample, group); x [B,C,HW]; out [B*groups] each.
 * Deterministic two-stage reduction (fp64 accumulators, no atomics); d_ws: mdtile_gn_stats_ws_size(B, groups) bytes. */
size_t mdtile_gn_stats_ws_size(int B, int groups);
int mdtile_gn_stats(const float* d_x, int B, int C, int HW, int groups, float* d_mean, float* d_var, void* d_ws,
                    mdtile_stream_t stream);
/* GroupNormParam.summary (tilevae.py:320-335): pixel-weighted pooling of T per-tile stat rows.
 * d_means/d_vars [T, BG]; d_frac[T] = the normalised pixel fractions p_i (tilevae.py:328-331, T host-side floats
 * computed by the caller and copied to the device); out [BG]:  var = sum_i p_i var_i, mean = sum_i p_i mean_i. */
int mdtile_gn_pool(const float* d_means, const float* d_vars, const float* d_frac, int T, int BG, float* d_mean,
                   float* d_var, mdtile_stream_t stream);
/* custom_group_norm (tilevae.py:218-245) fused with the following in-place SiLU (tilevae.py:102-104):
 * y = ((x - mean_g) / sqrt(var_g + eps)) * gamma_c + beta_c ; if silu: y = y * sigmoid(y).  gamma/beta may be NULL.
 * In place (d_y == d_x) allowed. */
int mdtile_gn_apply(const float* d_x, float* d_y, int B, int C, int HW, int groups, const float* d_mean,
                    const float* d_var, const float* d_gamma, const float* d_beta, float eps, int silu,
                    mdtile_stream_t stream);
/* standalone SiLU / residual add (queue tasks 'silu', 'add_res', tilevae.py:102-104, 614-616) */
int mdtile_silu(const float* d_x, float* d_y, size_t n, mdtile_stream_t stream);
int mdtile_tanh(const float* d_x, float* d_y, size_t n, mdtile_stream_t stream);   /* Decoder.tanh_out, scripts/tilevae.py:192-193 */
int mdtile_add(const float* d_a, const float* d_b, float* d_y, size_t n, mdtile_stream_t stream);

/* Conv tiles (queue tasks conv_in/conv1/conv2/nin_shortcut/upsample/conv_out/q/k/v/proj_out, tilevae.py:115-195).
 * stride 1, 'same' zero padding, ksize 1 or 3.  Weights are pre-packed once by mdtile_conv_pack (OIHW -> [tap][cin][cout] fp32,
 * followed by the split-bf16 fragment-order image for the shapes the bf16x3 kernel takes; mdtile_conv_packed_size covers both).
 *   MDTILE_CONV_UPSAMPLE2X : input is read through a nearest 2x upsample (ldm Upsample: interpolate then conv)
 *   d_residual != NULL     : y = conv(x) + bias + residual   ('add_res' fused)
 *   out_layout             : 0 = [B,Cout,H,W];  1 = token-major [B,H*W,Cout] (V operand of mdtile_vae_attn)
 * H, W are the OUTPUT spatial size. */
#define MDTILE_CONV_UPSAMPLE2X 1
#define MDTILE_CONV_EXACT_F32 2   /* force the exact-fp32 MFMA kernel (default: split-bf16 "bf16x3" MFMA where the shape allows,
                                     fp32 accumulate, ~1e-5 relative vs fp32; env MDTILE_CONV_MODE=f32 forces it globally) */
#define MDTILE_CONV_W_F16 128     /* mdtile_conv2d_gn / _gn_stats in MDTILE_PRECISION_F16: d_w_packed is the fp16 plane of mdtile_conv_pack_f16 -> the fp16
                                     one-term kernel (without the flag the call keeps its three terms; with it outside that mode, or together with
                                     MDTILE_CONV_EXACT_F32: an error) */
#define MDTILE_CONV_ATTN_PROJ 256 /* mdtile_conv2d, ksize 1: the conv is q / k / v / proj_out of the attention -- one-term bf16 in MDTILE_PRECISION_F16
                                     (any other 1x1 conv reads the raw stream and keeps three terms there); no effect in the other modes */
size_t mdtile_conv_packed_size(int cout, int cin, int ksize); /* floats */
int mdtile_conv_pack(const float* d_w_oihw, float* d_w_packed, int cout, int cin, int ksize, mdtile_stream_t stream);
/* fp16 weight plane of MDTILE_PRECISION_F16: fp16_rn(w) (clamped to +-65504) in the layout and K order of the hi plane of the split-bf16 image,
 * built from the packed buffer of mdtile_conv_pack (its fp32 image holds the exact weights) into a buffer of its own of
 * mdtile_conv_pack_f16_size floats (0: no fp16 kernel takes the shape; 3x3 only).  The packed buffer and mdtile_conv_packed_size are unchanged. */
size_t mdtile_conv_pack_f16_size(int cout, int cin, int ksize); /* floats */
int mdtile_conv_pack_f16(const float* d_w_packed, float* d_w_f16, int cout, int cin, int ksize, mdtile_stream_t stream);
int mdtile_conv2d(const float* d_x, const float* d_w_packed, const float* d_bias, const float* d_residual, float* d_y,
                  int B, int cin, int cout, int H, int W, int ksize, int flags, int out_layout, mdtile_stream_t stream);

/* ldm Downsample (encoder 'downsample' task, tilevae.py:155-171): y = conv3x3_stride2(pad(x, right 1, bottom 1)) + bias,
 * y is [B, cout, (Hin-2)/2+1, (Win-2)/2+1].  d_w_packed: mdtile_conv_pack(ksize 3) of the conv's OIHW weights. */
int mdtile_conv2d_down2(const float* d_x, const float* d_w_packed, const float* d_bias, float* d_y, int B, int cin, int cout,
                        int Hin, int Win, mdtile_stream_t stream);

/* Fused pre-activation: the fixed-statistics GroupNorm + SiLU that precedes conv1 / conv2 of every ResnetBlock
 * (custom_group_norm + inplace_nonlinearity, tilevae.py:218-245, 102-104; queue order pre_norm, silu, conv1 ... :115-137)
 * is applied while the conv stages its input, so the normalised activation never makes a round trip through HBM.
 *   mdtile_gn_coeffs           : d_coef[B][2][C] = { a = gamma / sqrt(var + eps), s = beta - mean * a } (same constants as mdtile_gn_apply)
 *   mdtile_conv2d_gn           : y = conv(silu(a * x + s)) + bias (+ residual); 3x3, stride 1, split-bf16 kernel only
 *   mdtile_conv2d_gn_supported : 1 when such a kernel exists for the shape / flags (else use mdtile_gn_apply + mdtile_conv2d) */
int mdtile_gn_coeffs(const float* d_mean, const float* d_var, const float* d_gamma, const float* d_beta, int B, int C, int groups,
                     float eps, float* d_coef, mdtile_stream_t stream);
int mdtile_conv2d_gn_supported(int cout, int cin, int ksize, int flags, int out_layout);
int mdtile_conv2d_gn(const float* d_x, const float* d_coef, const float* d_w_packed, const float* d_bias, const float* d_residual,
                     float* d_y, int B, int cin, int cout, int H, int W, int ksize, int flags, mdtile_stream_t stream);

/* Slow mode (round 5): the conv whose output is the input of a POOLED GroupNorm leaves that output's statistics itself -- what
 * GroupNormParam.add_tile asks of get_var_mean (tilevae.py:207-215, 300-307) without the pass that re-reads the activation.  The kernels'
 * epilogues write (sum, sum of squares) per block and 4-cout quad (fp32 inside a lane's <= 16 values, fp64 from there on); two small kernels combine them in a fixed order
 * (deterministic, no atomics) into d_mean / d_var [B * groups] (biased variance, as mdtile_gn_stats).  d_y is bit-identical to the call
 * without statistics.  d_ws: mdtile_conv_stats_ws_size(B, cout, H, W, groups) bytes (H, W = OUTPUT size), 16-byte aligned.
 *   mdtile_conv2d_gn_stats(_supported)  : mdtile_conv2d_gn + statistics (128-cout blocks: cout % 128 == 0; (cout / groups) % 4 == 0)
 *   mdtile_conv2d_rec_stats(_supported) : mdtile_conv2d_rec (fp32 output only; MDTILE_CONV_UPSAMPLE2X allowed) + statistics, declared below.
 *                                         Launches of only a few item rounds keep the kernel family mdtile_conv2d_rec would choose and
 *                                         run the statistics pass inside the call (same results contract, one entry point). */
size_t mdtile_conv_stats_ws_size(int B, int cout, int H, int W, int groups);
int mdtile_conv2d_gn_stats_supported(int cout, int cin, int ksize, int flags, int groups);
int mdtile_conv2d_gn_stats(const float* d_x, const float* d_coef, const float* d_w_packed, const float* d_bias, const float* d_residual,
                           float* d_y, int B, int cin, int cout, int H, int W, int ksize, int flags, int groups, float* d_mean, float* d_var,
                           void* d_ws, mdtile_stream_t stream);

/* Record-image conv path (fast mode: every GroupNorm's statistics are frozen before the tiles run, tilevae.py:464-505, 542-563).
 * A "record image" of an activation [B, C, H, W] (C % 32 == 0) is its split-bf16 form in MFMA fragment order with a
 * 1-pixel zero border:  rec[b][hl][C/8][H+2][pitch] x 16 bytes, hl = 0: bf16(x), hl = 1: bf16(x - hi); plane p = 2*kstep + kg
 * holds channels 32*(kstep>>1) + 16*(kstep&1) + 4*kg + (j&3) + 8*(j>>2), j = 0..7  -- 4 bytes per element, like fp32.
 * Rows: pitch = (W + 9 + 7) & ~7 records; pixel x sits at column x + 8, the border records at columns 7 and W + 8, the rest of a row
 * is padding nobody reads -- so that every 32-pixel run the kernels store is four whole 128-byte lines (round 4; the size is
 * opaque to callers: mdtile_rec_size).
 * The PRODUCER applies the following norm's (a, s) + SiLU (custom_group_norm + inplace_nonlinearity, tilevae.py:218-245,
 * 102-104) and splits; the consuming conv stages its input by DMA only.
 *   mdtile_rec_size            : bytes of the record image of [B, C, H, W]
 *   mdtile_rec_from_f32        : rec = split(silu(a x + s)) (d_coef = mdtile_gn_coeffs output [B][2][C]) or split(x) (d_coef NULL)
 *   mdtile_rec_to_f32          : x = hi + lo (inspection / tests)
 *   mdtile_conv2d_rec_supported: 1 when the record kernels take the shape (3x3, cin % 32 == 0, cout % 128 == 0; or cout < 32 -- conv_out:
 *                                fp32 output only, no residual / upsample, d_bias padded with zeros to 32 floats by the caller)
 *   mdtile_conv2d_rec          : y = conv3x3(x_rec) + bias (+ residual), written as fp32 NCHW (d_y, may be NULL) and / or as the
 *                                record image d_y_rec = split(silu(a y + s)) (d_y_coef [B][2][cout]) or split(y) (d_y_coef NULL);
 *                                MDTILE_CONV_UPSAMPLE2X: x_rec is the HALF-size input of the fused nearest-2x upsample conv
 *                                (ldm Upsample, tilevae.py:139-153).  H, W = output size.  d_w_packed: mdtile_conv_pack(ksize 3).
 * Second form (MDTILE_PRECISION_F16): an ACTIVATED record image (d_coef / d_y_coef given) written in that mode holds fp16_rn(clamp(x, +-65504)) in
 * the hi half -- the same 16-byte records, plane order and mdtile_rec_size; its lo half is NOT written (and its border is zeroed in the hi half
 * only).  A raw record image (coefficients NULL) is a bf16 (hi, lo) split in every mode.  The caller carries the form with the buffer:
 *   MDTILE_REC_BF16X2 / MDTILE_REC_F16        the format tag of mdtile_rec_from_f32_fmt / mdtile_rec_to_f32_fmt (the calls without _fmt: BF16X2)
 *   MDTILE_CONV_REC_X_F16                      mdtile_conv2d_rec(_stats): d_x_rec is the fp16 form AND d_w_packed is the plane of mdtile_conv_pack_f16
 *   MDTILE_CONV_REC_Y_F16                      mdtile_conv2d_rec / mdtile_upconv2d_rec_window: d_y_rec is to be the fp16 form
 * A tag that disagrees with what the mode writes (fp16 asked outside MDTILE_PRECISION_F16 or for a raw record; an activated record output in that
 * mode without _Y_F16; _X_F16 on an upsample conv; _Y_F16 on a direct conv whose input record is a bf16 split) is MDTILE_E_ARG with "record format mismatch" in the error text -- never a reinterpretation. */
#define MDTILE_REC_BF16X2 0
#define MDTILE_REC_F16 1
#define MDTILE_CONV_REC_X_F16 32
#define MDTILE_CONV_REC_Y_F16 64
#define MDTILE_CONV_REC_ONE_BLOCK 4   /* mdtile_conv2d_rec / mdtile_upconv2d_rec_window flags: name the kernel family instead of letting the */
#define MDTILE_CONV_REC_TWO_BLOCKS 8  /* launcher choose per launch (one 8-wave block per CU / two 4-wave blocks per CU; identical results) */
size_t mdtile_rec_size(int B, int C, int H, int W);
int mdtile_rec_from_f32(const float* d_x, const float* d_coef, void* d_rec, int B, int C, int H, int W, mdtile_stream_t stream);
int mdtile_rec_to_f32(const void* d_rec, float* d_x, int B, int C, int H, int W, mdtile_stream_t stream);
int mdtile_rec_from_f32_fmt(const float* d_x, const float* d_coef, void* d_rec, int B, int C, int H, int W, int fmt, mdtile_stream_t stream);
int mdtile_rec_to_f32_fmt(const void* d_rec, float* d_x, int B, int C, int H, int W, int fmt, mdtile_stream_t stream);
int mdtile_conv2d_rec_supported(int cout, int cin, int ksize, int flags);
int mdtile_conv2d_rec(const void* d_x_rec, const float* d_w_packed, const float* d_bias, const float* d_residual, float* d_y,
                      void* d_y_rec, const float* d_y_coef, int B, int cin, int cout, int H, int W, int flags,
                      mdtile_stream_t stream);
int mdtile_conv2d_rec_stats_supported(int cout, int cin, int ksize, int flags, int groups);
int mdtile_conv2d_rec_stats(const void* d_x_rec, const float* d_w_packed, const float* d_bias, const float* d_residual, float* d_y,
                            int B, int cin, int cout, int H, int W, int flags, int groups, float* d_mean, float* d_var, void* d_ws,
                            mdtile_stream_t stream);
/* Live-window narrowing of a decoder tile (fast mode only: frozen GroupNorm statistics make every later layer local).  Upstream decodes the
 * whole padded tile and crop_valid_region (tilevae.py:248-259, applied at :630-632) throws the padding away at the end; a pixel the remaining
 * 3x3 convs cannot carry into the valid region need not be computed at all.  The narrowing happens where the resolution doubles:
 *   mdtile_upconv2d_rec_window : the fused nearest-2x upsample conv (ldm Upsample, tilevae.py:139-153) of the window
 *                                [y0[b] : y0[b] + h, x0[b] : x0[b] + w] of image b of the record image of [B, cin, Hin, Win] (y0, x0: HOST arrays
 *                                of B ints -- stacked tiles of one shape keep their own origins; beyond 8 images the origins must repeat every 8); outputs are [B, cout, 2h, 2w] (fp32 d_y
 *                                and / or record image d_y_rec with d_y_coef as in mdtile_conv2d_rec).  Window edges inside the image read the
 *                                image's real neighbours, so the outputs equal the same pixels of the whole-image call bit for bit. */
int mdtile_upconv2d_rec_window(const void* d_x_rec, const float* d_w_packed, const float* d_bias, float* d_y, void* d_y_rec,
                               const float* d_y_coef, int B, int cin, int cout, int Hin, int Win, const int* y0, const int* x0, int h, int w,
                               int flags, mdtile_stream_t stream);

/* Row-band pieces of get_var_mean (tilevae.py:207-215) for an activation that is split by rows across GPUs (sequence-parallel
 * fast-mode estimator): every plane holds plane_stride floats of which [offset, offset+len) are this rank's own rows.
 *   mdtile_gn_sums      : d_sums[B*groups][2] = fp64 (sum, sum of squares) over the own rows of each (sample, group);
 *                         d_ws: mdtile_gn_stats_ws_size(B, groups) bytes.  Ranks all-reduce(sum) d_sums.
 *   mdtile_gn_from_sums : mean = s1/count, var = s2/count - mean^2 (biased), count = elements per (sample, group) over ALL ranks */
int mdtile_gn_sums(const float* d_x, int B, int C, size_t plane_stride, size_t offset, size_t len, int groups, double* d_sums,
                   void* d_ws, mdtile_stream_t stream);
int mdtile_gn_from_sums(const double* d_sums, double count, int BG, float* d_mean, float* d_var, mdtile_stream_t stream);

/* attn_forward body between the 1x1 convs (tile_utils/attn.py:55-70): single head,
 * out[b,c,i] = sum_j v[b,c,j] * softmax_j(scale * sum_c' q[b,c',i] k[b,c',j]).
 * q,k: [B,C,T] channel-major;  v: [B,T,C] token-major (conv out_layout 1);  out: [B,C,T].  C = 128, 256 or 512.
 * Flash formulation (no T x T matrix).  Default: split-bf16 ("bf16x3") matrix-core kernel -- q, k, v and the
 * probabilities are split into bf16 hi/lo pairs (16 significand bits), fp32 accumulation and fp32 softmax statistics,
 * ~1e-5 relative to fp32; it stages fragment-order copies of q, k, v in d_ws (mdtile_vae_attn_ws_size(B,C,T) bytes).
 * MDTILE_ATTN_EXACT_F32 (or env MDTILE_ATTN_MODE=f32) selects the exact-fp32 MFMA kernel, which needs no workspace. */
#define MDTILE_ATTN_EXACT_F32 1
#define MDTILE_ATTN_V_CHANNEL_MAJOR 2   /* v is [B,C,T] like q and k (split-bf16 kernel only): the v projection then runs on the same 1x1 kernels */
size_t mdtile_vae_attn_ws_size(int B, int C, int T);
/* 1 when mdtile_vae_attn(C, flags) will run the split-bf16 kernel and therefore accepts MDTILE_ATTN_V_CHANNEL_MAJOR -- the SAME conditions
 * the dispatch inside mdtile_vae_attn tests (flags, mdtile_set_precision, env MDTILE_ATTN_MODE=f32, C); 0: hand v over token-major. */
int mdtile_vae_attn_takes_channel_major(int C, int flags);
int mdtile_vae_attn(const float* d_q, const float* d_k, const float* d_v, float* d_out, int B, int C, int T, float scale,
                    int flags, void* d_ws, mdtile_stream_t stream);
/* Same contraction with separate query / key token counts: q [B,C,Tq], k [B,C,Tk], v [B,Tk,C] -> out [B,C,Tq]
 * (a row band of queries against the keys / values gathered from every band).  Split-bf16 kernel; workspace as above. */
size_t mdtile_vae_attn_qk_ws_size(int B, int C, int Tq, int Tk);
int mdtile_vae_attn_qk(const float* d_q, const float* d_k, const float* d_v, float* d_out, int B, int C, int Tq, int Tk, float scale,
                       void* d_ws, mdtile_stream_t stream);

/* crop_valid_region + result[...] = tile (tilevae.py:248-259, 630-632): copies the valid window of one finished tile
 * [N,C,th,tw] into result [N,C,RH,RW].  in_bbox/out_bbox as returned by mdtile_vae_split_tiles. */
int mdtile_crop_store(const float* d_tile, int N, int C, int th, int tw, const int* in_bbox4, const int* out_bbox4,
                      int is_decoder, float* d_result, int RH, int RW, mdtile_stream_t stream);
/* tile extraction z[:, :, y1:y2, x1:x2] (tilevae.py:532-535) == mdtile_gather_rect with dtype f32 */

/* mdtile_crop_store of every finished tile of one call into result [N,C,RH,RW] (fp32, on the calling device), one launch per
 * MDTILE_VAE_ASSEMBLE_CHUNK tiles.  A tile [N,C,th,tw] may live on another device: it is read through the peer mapping, which the call
 * enables (mdtile_enable_peer_access); a tile on a device the calling device cannot read, a bad bbox or a window outside the result
 * returns an error before anything is launched. */
#define MDTILE_VAE_ASSEMBLE_CHUNK 32
typedef struct mdtile_vae_tile {
    const float* tile;
    int th, tw;
    int in_bbox4[4];
    int out_bbox4[4];
} mdtile_vae_tile;
int mdtile_vae_assemble(const mdtile_vae_tile* tiles, int n_tiles, int N, int C, int is_decoder, float* d_result, int RH, int RW,
                        mdtile_stream_t stream);
/* mdtile_vae_assemble with the tile borders cross-faded over the padding that crop_valid_region throws away (opt-in; upstream pastes
 * edge to edge).  tiles: the rows x cols tiles of one call in row-major order, as mdtile_vae_split_tiles yields them; their out boxes
 * partition the result as a tensor-product grid.
 *   Band and weights.  band = b >= 1 output px.  At an interior vertical border at column X (the left tile's out_x2 == the right tile's
 *     out_x1) the band is the columns x in [X - b, X + b) with the integer ramp through the pixel centres
 *         aR(x) = 2 (x - X + b) + 1,   aL(x) = 4 b - aR(x)          (both odd, in [1, 4 b - 1], never zero);
 *     a horizontal border at row Y has aB(y), aT(y) in the same way.
 *   Outside every band: the owning tile's value, copied bit for bit -- there the image is mdtile_vae_assemble's (NaN payloads, -0.0
 *     and denormals included).
 *   In one band only: the two tiles on either side contribute with (aL, aR) or (aT, aB), D = 4 b.
 *   In a column band and a row band: four tiles with aT aL, aT aR, aB aL, aB aR, D = 16 b^2 (b <= 1024: every weight < 2^24, exact in fp32).
 *   A band pixel:  acc = +0.0f;  for the contributing tiles in ascending tile index: acc = acc + (float)w_k * v_k (product and sum each
 *     rounded once; the library is built with -ffp-contract=off);  out = acc / (float)D (IEEE division).  v_k is read from tile k's
 *     PADDED output at the pixel's position.
 *   Legality, checked for the whole table before anything is launched (MDTILE_E_ARG, tile and reason in mdtile_last_error, nothing
 *     written): the out boxes form the grid (shared borders, covering [0, RW) x [0, RH)); a tile next to a border is at least b wide
 *     (tall) there and one with a border on both sides of an axis at least 2 b (bands may touch, not overlap); every tile's padded
 *     output contains its out box grown by b on each side that has a neighbour (margins from in_bbox4 by the is_decoder rule of
 *     mdtile_vae_assemble: in * 8 / in / 8); the peer, device and size checks of mdtile_vae_assemble.
 * Every pixel of the result is written exactly once (no atomics, no read-modify-write: the result need not be zeroed); the table travels
 * in the kernel arguments, each tile with its neighbours (MDTILE_VAE_BLEND_CHUNK tiles per launch): stream-ordered, no allocation, no
 * host synchronisation, no host memory referenced after the call returns. */
#define MDTILE_VAE_BLEND_CHUNK 16
int mdtile_vae_assemble_blend(const mdtile_vae_tile* tiles, int rows, int cols, int N, int C, int is_decoder, int band, float* d_result,
                              int RH, int RW, mdtile_stream_t stream);
/* idempotent: kernels running on `device` may read memory of `peer` afterwards (MDTILE_E_ARG when the hardware cannot) */
int mdtile_enable_peer_access(int device, int peer);

/* ----------------------------------------------------------------------------------------------------------
 * Tiled VAE tile skipping (img2img inpainting, decoder): decode only the tiles the job's overlay mask touches and complete the image
 * without the others.  Nothing upstream corresponds to it.
 *
 * mdtile_mask_activity_u8: d_mask uint8 [RH, RW] (row pitch RW bytes), d_boxes4 int32 [n_boxes][4] = (x1, x2, y1, y2) in image px as
 *   mdtile_vae_split_tiles returns them, d_active int32 [n_boxes], all on the calling device.  active[i] = 1 iff some byte of
 *   mask[y1:y2, x1:x2] is not zero, else 0.  The call writes every entry (a stream-ordered clear, then ONE kernel over blocks
 *   (chunk of rows, box): 16-byte reads where the row segment allows, scalar bytes in front of the first and behind the last 16-byte
 *   boundary, the OR per wave, a wave that saw a non-zero byte stores 1); the caller does not zero d_active.  The boxes are copied to the
 *   host and checked before anything is written, which waits for `stream` once.  MDTILE_E_ARG, the reason in mdtile_last_error, nothing
 *   written: a null pointer, RH or RW < 1, n_boxes outside 1 .. MDTILE_MASK_ACTIVITY_MAX_BOXES (4096: an 8K image at decoder tile 48 has 441 tiles),
 *   a box that is empty or not inside RW x RH.
 * mdtile_vae_assemble_sparse (decoder: out = in * 8): the tiles go into result [N,C,RH,RW] exactly as mdtile_vae_assemble(...,
 *   is_decoder = 1, ...) puts them -- its checks, its peer mapping, its kernel, its bits -- and every fill box (x1, x2, y1, y2; host ints) is
 *   written as
 *       result[n, c, y, x] = (float)fill[y, x, c] / 127.5f - 1.0f      (one IEEE fp32 division, one subtraction; every n)
 *   from d_fill_u8, ONE uint8 image [RH, RW, C] (interleaved, on the calling device), or as +0.0f when d_fill_u8 is NULL.  The fill's bytes
 *   are read as one contiguous run per row, the planes written in 16-byte stores from the row's first 16-byte boundary on.  Checked for the
 *   whole call before anything is launched (MDTILE_E_ARG, nothing written): mdtile_vae_assemble's tests of every tile; every fill box
 *   non-empty and inside RW x RH; no fill box equal to a tile's out box; no two boxes (tile out boxes and fill boxes together) overlapping;
 *   their areas summing to RH * RW; n_tiles + n_fill <= MDTILE_VAE_SPARSE_MAX_BOXES.  Together: the boxes partition the result and every
 *   pixel is written exactly once (the result need not be zeroed).  n_tiles == 0 (tiles may be NULL) and n_fill == 0 (fill_boxes4 may be
 *   NULL) are allowed.  The tables travel in the kernel arguments (MDTILE_VAE_ASSEMBLE_CHUNK tiles, MDTILE_VAE_FILL_CHUNK fill boxes per
 *   launch): stream-ordered, no allocation, no host synchronisation, no host memory referenced after the call returns.
 * -------------------------------------------------------------------------------------------------------- */
#define MDTILE_MASK_ACTIVITY_MAX_BOXES 4096
#define MDTILE_VAE_SPARSE_MAX_BOXES 4096
#define MDTILE_VAE_FILL_CHUNK 128
int mdtile_mask_activity_u8(const uint8_t* d_mask, int RH, int RW, const int* d_boxes4, int n_boxes, int* d_active, mdtile_stream_t stream);
int mdtile_vae_assemble_sparse(const mdtile_vae_tile* tiles, int n_tiles, const int* fill_boxes4, int n_fill, const uint8_t* d_fill_u8, int N, int C,
                               float* d_result, int RH, int RW, mdtile_stream_t stream);

/* fast-mode estimator input (tilevae.py:545-559): scale_factor = tile_size / max(H, W); nearest-exact resample of
 * z [N,C,H,W] to [N,C,oh,ow] (sizes from mdtile_vae_fast_size), per-channel re-standardisation (unbiased std over
 * N,H,W of both), clamp to [min z, max z].  d_ws: mdtile_vae_fast_ws_size(C) bytes. */
int mdtile_vae_fast_size(int H, int W, int tile_size, int* oh, int* ow);
size_t mdtile_vae_fast_ws_size(int C);
int mdtile_vae_fast_input(const float* d_z, int N, int C, int H, int W, int tile_size, float* d_out, void* d_ws,
                          mdtile_stream_t stream);

/* ----------------------------------------------------------------------------------------------------------
 * Multi-GPU (upstream is single-device: scripts/tilediffusion.py:257-383 drives one `p`).
 * A shard context owns one RCCL communicator and one HIP stream per LOCAL rank.  RCCL is dlopen'ed on first use.
 *   mdtile_shard_init(ndev, dev_ids)      single process, one rank per listed device (ncclCommInitAll): usable from inside a webui.
 *                                         Listing a device twice (or MDTILE_SHARD_TRANSPORT=copy) selects the "copy" transport:
 *                                         hipMemcpyAsync + events instead of RCCL, same packing and summation (1-GPU functional runs)
 *   mdtile_shard_unique_id / _init_rank   one rank of a process-per-GPU job: rank 0 draws the 128-byte id, the host distributes it
 *   mdtile_shard_info                     info4 = { ranks, local ranks, first local rank, 1 = RCCL | 0 = copy transport }
 * Per-rank arrays below have one entry per LOCAL rank; streams == NULL uses the context's own streams (mdtile_shard_stream).
 *   mdtile_halo_exchange   band_rows[2 r], [2 r + 1] = canvas rows [lo, hi) the tiles of rank r touch (contiguous bands of tile rows).
 *                          d_partial[i] [N,C,H,W] fp32 holds rank i's partial sums (mdtile_blend with MDTILE_BLEND_PARTIAL); rows shared
 *                          with other bands are packed, swapped (grouped ncclSend / ncclRecv) and summed in ascending rank order on
 *                          every side (bit-identical everywhere); then mdtile_blend_finalize.  d_scratch[i]: mdtile_halo_scratch_bytes.
 *   mdtile_allreduce_stats all-reduce(sum) of `count` doubles in place (slow-mode GroupNorm pooling across ranks, tilevae.py:320-335)
 *   mdtile_shard_bcast     `bytes` from rank `root` to all ranks (a region's model output to the bands that composite it)
 *   mdtile_shard_p2p       grouped point-to-point (one ncclGroup per call): ops[i][0 .. n_ops[i]) are local rank i's transfers; an op
 *                          sends and / or receives (bytes == 0 skips that half); the k-th send of a to b pairs with b's k-th receive
 *                          from a.  Carries the row halos of the sequence-parallel estimator (both directions in one group) and the
 *                          gather of the decoded tile rectangles to the rank that returns the image
 *   mdtile_shard_allgather every rank contributes `bytes`; d_recv[i] (nranks * bytes) holds them in rank order (K / V of the
 *                          sequence-parallel estimator's attention, tile_utils/attn.py:55-67)
 *   mdtile_shard_selfcheck bring-up check: all-reduce, broadcast, grouped ring send / receive (a self send / receive on one rank) and
 *                          all-gather of small payloads, verified on the host; d_scratch[i] >= mdtile_shard_selfcheck_bytes(sh).
 *                          MDTILE_SHARD_TRANSPORT=rccl makes a one-device context use a 1-rank RCCL communicator (it needs none).
 *   mdtile_shard_probe_rank  interruptible bring-up probe of a process-per-GPU communicator: the same rendezvous as mdtile_shard_init_rank on a
 *                          NON-BLOCKING communicator, polled until it is up or `timeout_s` has passed, then aborted (ncclCommAbort) -- the calling
 *                          thread is never left blocked inside RCCL.  Every rank calls it with the same id (an id of its own, not the one the
 *                          real communicator will use).  MDTILE_OK: the rendezvous works, go on to mdtile_shard_init_rank. */
typedef struct mdtile_shard mdtile_shard;
mdtile_shard* mdtile_shard_init(int ndev, const int* dev_ids);
int mdtile_shard_unique_id(void* id128);
mdtile_shard* mdtile_shard_init_rank(int nranks, int rank, const void* id128, int device);
int mdtile_shard_probe_rank(int nranks, int rank, const void* id128, int device, double timeout_s);
void mdtile_shard_destroy(mdtile_shard* sh);
int mdtile_shard_info(const mdtile_shard* sh, int* info4);
mdtile_stream_t mdtile_shard_stream(const mdtile_shard* sh, int local_rank);
size_t mdtile_halo_scratch_bytes(int nranks, int rank, const int* band_rows, int N, int C, int W);
int mdtile_halo_exchange(mdtile_shard* sh, float* const* d_partial, void* const* d_scratch, int N, int C, int H, int W,
                         const int* band_rows, const mdtile_stream_t* streams);
int mdtile_allreduce_stats(mdtile_shard* sh, double* const* d_buf, int count, const mdtile_stream_t* streams);
int mdtile_shard_bcast(mdtile_shard* sh, void* const* d_buf, size_t bytes, int root, const mdtile_stream_t* streams);
typedef struct mdtile_p2p {
    int peer;
    const void* send;
    size_t send_bytes;
    void* recv;
    size_t recv_bytes;
} mdtile_p2p;
int mdtile_shard_p2p(mdtile_shard* sh, const mdtile_p2p* const* ops, const int* n_ops, const mdtile_stream_t* streams);
int mdtile_shard_allgather(mdtile_shard* sh, const void* const* d_send, void* const* d_recv, size_t bytes, const mdtile_stream_t* streams);
size_t mdtile_shard_selfcheck_bytes(const mdtile_shard* sh);
int mdtile_shard_selfcheck(mdtile_shard* sh, void* const* d_scratch, const mdtile_stream_t* streams);

#ifdef __cplusplus
}
#endif
#endif /* MDTILE_H */
