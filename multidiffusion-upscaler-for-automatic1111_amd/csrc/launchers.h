// Every function of libmdtile that one .hip file defines and another calls, grouped by the file that defines it.  Default arguments are
// written here and nowhere else.  The defining files include this header and define these functions by their qualified names
// (`int mdt::conv_rec_launch(...)`), which only compiles against a matching declaration: a signature that drifts is a compile error.
// (conv_rec2_launch and the probes-only conv_recd_* take the kernels' ConvRParams: conv_rec_common.h declares them next to it.)
// The two 3x3 conv families take their launch as ONE struct with named fields (HandoverConvCall, RecConvCall); inside the defining files every
// matrix-core family picks its kernel in one function that returns the function pointer, and launches it in one statement.
#pragma once
#include "common.h"

namespace mdt {

// ---- wrap.hip: wrap-x, wrap-y and torus plans (mdtile_plan_create_wrap) and sparse plans (mdtile_plan_create_subset, the tiles an inpaint
// mask touches), one kernel set for all of them; the public entry points hand such a plan (mdt::plan_wraps, mdt::plan_sparse) to these
// launchers.  walk_gather fills the batches of the positions [s_lo, s_hi): tiles, or the active slots of a sparse plan.  walk_blend takes
// d_fill for a sparse plan only.  gather_check: what every mdtile_gather* asks of its arguments.
int wrap_weight_map(const struct ::mdtile_plan* plan, const float* d_tile_w, float* d_weights, hipStream_t s);
int gather_check(const struct ::mdtile_plan* plan, int dtype, int N, int C, const void* d_x_in, void* const* ptrs);
// shift = {sx, sy}: the shifted grid of mdtile_gather_all_shift / mdtile_blend_shift (wrap.hip, which checks it); null: not shifted.
int walk_gather(const struct ::mdtile_plan* plan, int dtype, int N, int C, const void* d_x_in, void* const* ptrs, int nptrs, int s_lo, int s_hi,
                hipStream_t s, const int* shift = nullptr);
int walk_blend(const struct ::mdtile_plan* plan, const ::mdtile_blend_args* args, const void* const* batch_out, int num_batches,
               int num_regions, const void* d_fill, hipStream_t s, const int* shift = nullptr);
// the blend with custom regions on a wrap-around plan: mdtile_blend_wrap_regions (wrap_regions.hip) has checked the arguments and counted the
// foreground regions
int walk_blend_regions(const struct ::mdtile_plan* plan, const ::mdtile_blend_args* args, const void* const* batch_out, int num_batches,
                       const ::mdtile_wrap_regions* wr, int num_fg, hipStream_t s);
// what every shifted entry point (wrap.hip, wrap_regions.hip) asks of the plan and the shift before anything else is looked at; errors name `fn`
int shift_check(const char* fn, const struct ::mdtile_plan* plan, int sx, int sy);

// ---- blend.hip: the plain blend with a coverage map per region: mdtile_blend_mask_regions (mask_regions.hip) has refused what the call does not
// take and checked the list; k_blend<..., MASKED = true>, whose text has the arithmetic
int blend_masked(const struct ::mdtile_plan* plan, const ::mdtile_blend_args* args, const void* const* batch_out, int num_batches,
                 const struct ::mdtile_mask_region* regions, int num_regions, hipStream_t s);

// ---- vae_assemble.hip: mdtile_vae_assemble in two halves, for vae_skip.hip (mdtile_vae_assemble_sparse pastes its tiles with them).
// vae_assemble_check: every test of the table and the result, the peer mapping of every source device; errors name `who`.
int device_of(const void* p);      // the device that owns `p` (device memory of this process), or -1
int vae_assemble_check(const char* who, const ::mdtile_vae_tile* tiles, int n_tiles, int N, int C, int is_decoder, const float* d_result, int RH,
                       int RW);
int vae_assemble_launch(const ::mdtile_vae_tile* tiles, int n_tiles, int N, int C, int is_decoder, float* d_result, int RH, int RW, hipStream_t s);

// ---- plan.hip
int device_cus();     // multiProcessorCount of the device that was current at the first call (256 if it cannot be read), cached

// ---- vae_conv_bf16x3.hip
bool conv_bf16x3_eligible(int cout, int cin, int ksize);
size_t conv_bf16x3_direct_records(int cout, int cin);
size_t conv_bf16x3_packed_floats(int cout, int cin);
int conv_bf16x3_pack(const float* d_w_oihw, void* d_out, int cout, int cin, hipStream_t s);
bool conv_rec_narrow_eligible(int cout, int cin, int ksize);
size_t conv_rec_narrow_packed_floats(int cin);
int conv_rec_narrow_pack(const float* d_w_oihw, void* d_out, int cout, int cin, hipStream_t s);
size_t conv_f16_plane_floats(int cout, int cin);
int conv_f16_pack(const float* d_w_f32img, void* d_out, int cout, int cin, hipStream_t s);
bool conv_bf16x3_gn_supported(int cout, int cin, int ksize, int up);
bool conv_bf16x3_stats_supported(int cout, int cin, int ksize, int up);
size_t conv_bf16x3_stats_part_doubles(int B, int cout, int H, int W);
// One hand-over 3x3 conv (fp32 NCHW in and out) as a C entry point (vae_conv.hip) hands it to conv_bf16x3_launch.  Host side only: the kernels
// take ConvBParams.
struct HandoverConvCall {
    const float* x = nullptr;        // fp32 input
    const void* w_rec = nullptr;     // split-bf16 record image of the weights (direct records, then the sub-pixel ones); w16: the fp16 plane
    const float* bias = nullptr;
    const float* res = nullptr;      // fp32 residual or null
    float* y = nullptr;              // fp32 output
    const float* coef = nullptr;     // fused GroupNorm + SiLU on the input, (a, s) per image and channel, or null (direct stride-1 kernels only)
    double* d_part = nullptr;        // statistics of the output from the epilogue: the per-block partials (128-cout blocks with coef only)
    int B = 0, cin = 0, cout = 0, H = 0, W = 0;      // H, W: OUTPUT size
    int up = 0;                      // nearest-2x in front of the conv (sub-pixel kernels)
    int stride = 1;                  // 2: ldm's Downsample, conv over pad(x, right 1, bottom 1); no residual, no coef
    int Hin = 0, Win = 0;            // stride 2 only: the input size (H = (Hin - 2) / 2 + 1 does not determine it); else derived from H, W, up
    int w16 = 0;                     // MDTILE_PRECISION_F16: w_rec is the fp16 weight plane -> the fp16 kernels (coef required, never up / stride 2)
};
int conv_bf16x3_launch(const HandoverConvCall& c, hipStream_t s);

// ---- vae_conv1x1_bf16x3.hip
bool conv1x1_bf16x3_eligible(int cout, int cin);
size_t conv1x1_bf16x3_packed_floats(int cout, int cin);
int conv1x1_bf16x3_pack(const float* d_w_oihw, void* d_out, int cout, int cin, hipStream_t s);
int conv1x1_bf16x3_launch(const float* d_x, const void* d_w_rec, const float* d_bias, const float* d_res, float* d_y, int B, int cin,
                          int cout, size_t HW, hipStream_t s, bool attn_proj = false);

// ---- vae_norm.hip
int conv_stats_finish_launch(const double* d_cpart, int B, int cout, size_t HW, int units, int NCB, int QB, int groups, float* d_mean, float* d_var,
                             void* d_gnws, hipStream_t s);

// ---- vae_conv_rec.hip
bool conv_rec_supported(int cout, int cin, int ksize);
size_t rec_image_bytes(int B, int C, int H, int W);
size_t rec_plane_records(int H, int W);
int rec_from_f32_launch(const float* d_x, const float* d_coef, void* d_rec, int B, int C, int H, int W, hipStream_t s, int f16 = 0);
int rec_to_f32_launch(const void* d_rec, float* d_x, int B, int C, int H, int W, hipStream_t s, int f16 = 0);
// One record conv as a C entry point (vae_conv.hip) hands it to conv_rec_launch.  Host side only: the kernels take ConvRParams.
struct RecConvCall {
    const void* x_rec = nullptr;     // input record image
    const void* w_rec = nullptr;     // split-bf16 record image of the weights (direct records, then the sub-pixel ones); x16: the fp16 plane
    const float* bias = nullptr;
    const float* res = nullptr;      // fp32 residual or null
    float* y32 = nullptr;            // fp32 output or null
    void* y_rec = nullptr;           // record output or null
    const float* y_coef = nullptr;   // activation of the record output, (a, s) per image and channel, or null
    int B = 0, cin = 0, cout = 0, H = 0, W = 0;      // H, W: OUTPUT size
    int up = 0;                      // nearest-2x in front of the conv (sub-pixel kernels)
    // win (sub-pixel upsample kernel only, else null): {HinF, WinF, y0[0], x0[0], ..., y0[7], x0[7]} -- x_rec is the record image of
    // [B, cin, HinF, WinF] and image b's conv reads its window [y0[b & 7] : .. + H/2, x0[b & 7] : .. + W/2]  (all 8 slots filled)
    const int* win = nullptr;
    int family = 0;                  // 0 = chosen per launch, 1 / 2 = one / two blocks per CU, 3 = the dripped-epilogue kernel (PROBES twin only)
    double* d_part = nullptr;        // statistics of the output from the epilogue: the per-wave partials (one-block family only)
    // x16 (MDTILE_PRECISION_F16): x_rec is an activated record image in its fp16 form and w_rec the fp16 weight plane -> the fp16 kernels;
    // y16: the (activated) record output is written in the fp16 form.  The C entry points have checked both against the mode.
    int x16 = 0, y16 = 0;
};
int conv_rec_launch(const RecConvCall& c, hipStream_t s);
bool conv_rec_stats_in_epilogue(int B, int cout, int H, int W, int up);
int conv_rec_stats_units(int H, int W, int up);

// ---- vae_attn_bf16x3.hip
bool attn_bf16x3_eligible(int C);
size_t attn_bf16x3_ws_bytes(int B, int C, int Tq, int Tk);
int attn_bf16x3_launch(const float* d_q, const float* d_k, const float* d_v_tok, float* d_out, int B, int C, int Tq, int Tk, float scale,
                       void* d_ws, hipStream_t s, bool v_channel_major = false);

}  // namespace mdt
