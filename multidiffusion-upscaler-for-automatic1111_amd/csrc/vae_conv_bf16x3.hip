// 3x3 conv tiles of the Tiled-VAE task queue on the bf16 matrix cores with SPLIT-fp32 operands ("bf16x3").
//
// Why: the decoder's 3x3 convs are ~70 % of an 8K decode and gfx950 has no TF32; exact-fp32 MFMA peaks at 157 TFLOP/s,
// bf16 MFMA at 2.5 PFLOP/s.  Every fp32 operand is split x = hi + lo (hi = bf16(x), lo = bf16(x - hi): 16 significand
// bits together) and a product is formed as  a_lo*b_hi + a_hi*b_lo + a_hi*b_hi  with fp32 accumulation inside the MFMA:
// three bf16 MFMAs per fp32-class product = 16/3 x the fp32-MFMA rate.  The dropped a_lo*b_lo term and the split residue
// are <= 2^-16 relative per product (measured end-to-end against the fp32 reference in tests/test_gpu_vae.py: ~1e-5, the
// stated tolerance is 1e-3).  The exact-fp32 kernel (vae_conv.hip) stays available (MDTILE_CONV_EXACT_F32).
//
// Upstream call sites replaced: the nn.Conv2d tasks conv1 / conv2 / upsample.conv of scripts/tilevae.py:115-195 (+ the
// queue's add_res, tilevae.py:614-616, and F.interpolate(nearest, 2x) of ldm's Upsample, both fused as in vae_conv.hip).
//
// GEMM view (implicit, no im2col):  D[cout][px] = sum_{tap, cin} W[cout][cin][tap] * X[cin][px + tap]
//   MFMA v_mfma_f32_32x32x16_bf16:  A = weights (M = 32 couts, K = 16 cin of one tap), B = input (K = 16 cin, N = 32 px of a row)
//   lane l supplies 8 consecutive k of row/col (l & 31): k-half (l >> 5)  ->  both operands want "8 channels of one
//   cout / one pixel" as one 16-byte LDS record:
//     input  LDS image  [hl][cg = 2][rows = 10][cols = 34] x 16 B   (cg = 8-channel group; halo tile of an 8 x 32 px block)
//     weight LDS image  [hl][dx = 3][mtile][lane = 64]     x 16 B   (exactly the global pre-packed order: straight copy)
//   every fragment read is one conflict-free ds_read_b128 (32 consecutive 16-byte records per half-wave).
// Block = 512 threads = 8 waves (2 per SIMD), output tile BM couts x 8 rows x 32 px; wave = 64 couts x NROW rows.
// K loop = phases (16-channel K-step, dy): 3 taps x (2 x NROW) tiles x 3 MFMAs per wave and phase, ONE barrier per phase;
// the next phase's weights (24 KB, L2-resident) and the next K-step's input slab are fetched into registers at the start
// of a phase and written to the other LDS stage at its end (fp32 -> hi/lo split happens on that write).
#include "launchers.h"
#include "f16_convert.h"

using namespace mdt;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));   // one 16-byte record (plain vector type: stays in registers)

namespace {

struct ConvBParams {
    const float* x;      // [B, Cin, Hin, Win] fp32
    const u32x4* w;      // packed bf16 hi/lo records, see k_conv_pack_bf16x3
    const float* bias;   // [Cout] or null
    const float* res;    // residual [B, Cout, H, W] or null
    float* y;            // [B, Cout, H, W]
    int B, Cin, Cout, H, W;   // H, W: OUTPUT spatial size
    int Hin, Win, up;         // input spatial size; up = 1: sub-pixel upsample kernel (output = 2x input)
    int ptiles, PX, NCB, NK;  // pixel tiles, tiles per row, cout blocks, 16-channel K-steps
    const float* coef;        // fused pre-activation (GNS kernels): [B][2][Cin] = per-channel scale a, shift s; x' = silu(a x + s)
    int perm;                 // channel order inside a K-step, see kstep_c0 / kstep_cj
    double* gn_part;          // ST kernels: per-block partial (sum, sum of squares) of the OUTPUT per 4-cout quad, see the epilogue
};

constexpr int MAX_GN_CIN = 512;   // the fused pre-activation keeps a[Cin], s[Cin] in LDS

constexpr int TH = 8, TW = 32, ROWS = TH + 2, COLS = TW + 2;
constexpr int IN_REC = 2 * ROWS * COLS;                 // 680 records (16 B) per hl per stage

__device__ __forceinline__ void split8(const float (&v)[8], u32x4& hi, u32x4& lo) {
    bf16x8 h, l;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        h[i] = (__bf16)v[i];                            // v_cvt_pk_bf16_f32 (RNE)
        l[i] = (__bf16)(v[i] - (float)h[i]);            // exact residue, rounded once
    }
    hi = __builtin_bit_cast(u32x4, h);
    lo = __builtin_bit_cast(u32x4, l);
}

// Channel order inside a 16-channel K-step.  perm = 1 (cin % 32 == 0): K index (kg, j) of K-step k is channel
//     32*(k>>1) + 16*(k&1) + 4*kg + (j&3) + 8*(j>>2)
// = the channels one lane of a 32x32 MFMA accumulator tile owns, which is the order the record-image conv family
// (vae_conv_rec.hip) stores activations in; ONE packed weight image then serves both families.  perm = 0: k*16 + kg*8 + j.
__device__ __host__ __forceinline__ int kstep_c0(int k, int kg, int perm) { return perm ? 32 * (k >> 1) + 16 * (k & 1) + 4 * kg : k * 16 + kg * 8; }
__device__ __host__ __forceinline__ int kstep_cj(int j, int perm) { return perm ? (j & 3) + 8 * (j >> 2) : j; }

// GNS = true: the fixed-statistics GroupNorm + SiLU that precedes conv1 / conv2 in every resblock (custom_group_norm +
// inplace_nonlinearity, scripts/tilevae.py:218-245, 102-104) is applied to the input while it is staged:
// x' = silu(fma(x, a[c], s[c])) with a = gamma * rstd, s = beta - mean * a (mdtile_gn_coeffs) -- the normalised activation is
// never written to HBM (1R + 1W of every pre-conv activation saved).  Zero padding applies to x' (mask after the transform).
// Two block shapes (every other variant was measured and dropped):
//   MT = 4 (128 couts): weights by LDS-DMA (already in fragment order), ONE input stage (an extra barrier before it is
//           overwritten, once per K-step), 124 VGPR + 71 KB LDS -> TWO blocks per CU (4 waves per SIMD); MFMAs issued
//           term-major across the accumulators of a tap column (a dependent MFMA is >= 4 MFMAs away)
//   MT = 2 (64 couts, small decoders): weights through VGPRs, two input stages
// S = 2 (round 3): ldm's Downsample of the ENCODER (scripts/tilevae.py:155-171: conv 3x3, stride 2, over pad(x, right 1, bottom 1)) on
// the same split-bf16 arithmetic.  Output tile 8 x 32 px, input halo tile 17 x 65; the LDS image keeps the two COLUMN PARITIES of a
// row apart ([cg][row 17][parity 2][33]) so that the fragment of tap dx -- input columns 2 x + dx of 32 consecutive output px -- is
// again 32 consecutive records (a stride-2 ds_read_b128 would be a 2-way bank conflict).  Zero padding only right / bottom.
// ST = true (slow mode, round 5): the conv whose output feeds a POOLED GroupNorm (GroupNormParam.add_tile -> get_var_mean,
// scripts/tilevae.py:207-215, 300-307) also leaves the statistics of that output: every block writes (sum, sum of squares) of its
// BM couts x 8 x 32 px in 4-cout quads -- gn_part[(b * ptiles + ptile) * NCB + cb][BM / 4][2] fp64, combined in a fixed order by
// k_conv_stats_partial / k_gn_final (vae_norm.hip): the separate pass that re-read the whole activation is gone.  y is bit-identical.
#define MDT_OPERAND_F16 0      // mfma_operand.h: bf16 fragments
#define MDT_B3_TERMS 3
#define MDT_B3_KERNEL k_conv3x3_bf16x3
#include "vae_conv_bf16x3_direct_body.h"
#undef MDT_B3_KERNEL
#undef MDT_B3_TERMS
#define MDT_B3_TERMS 1
#define MDT_B3_KERNEL k_conv3x3_bf16x1
#include "vae_conv_bf16x3_direct_body.h"
#undef MDT_B3_KERNEL
#undef MDT_B3_TERMS

// fp16 form (MDTILE_PRECISION_F16): launched only with the fused pre-activation (GNS) -- the one operand this family can prove normalised
#undef MDT_OPERAND_F16
#define MDT_OPERAND_F16 1
#define MDT_B3_TERMS 1
#define MDT_B3_KERNEL k_conv3x3_f16
#include "vae_conv_bf16x3_direct_body.h"
#undef MDT_B3_KERNEL
#undef MDT_B3_TERMS
#undef MDT_OPERAND_F16
#define MDT_OPERAND_F16 0

// OIHW fp32 -> records [cb][k][dy][hl][dx][mt][lane] of 8 bf16:  cout = cb*BM + mt*32 + (lane & 31),
// cin = k*16 + (lane >> 5)*8 + j,  tap = (dy, dx);  hl = 0: bf16(w), hl = 1: bf16(w - hi).  Zero outside [Cout) x [Cin).
__global__ void k_conv_pack_bf16x3(const float* __restrict__ w, u32x4* __restrict__ out, int Cout, int Cin, int MT, int NCB, int NK, int perm) {
    const size_t n = (size_t)NCB * NK * 3 * 2 * 3 * MT * 64;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    size_t r = i;
    const int lane = (int)(r % 64); r /= 64;
    const int mt = (int)(r % MT); r /= MT;
    const int dx = (int)(r % 3); r /= 3;
    const int hl = (int)(r % 2); r /= 2;
    const int dy = (int)(r % 3); r /= 3;
    const int k = (int)(r % NK); r /= NK;
    const int cb = (int)r;
    const int co = cb * MT * 32 + mt * 32 + (lane & 31);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = kstep_c0(k, lane >> 5, perm) + kstep_cj(j, perm);
        const float v = (co < Cout && ci < Cin) ? w[(((size_t)co * Cin + ci) * 3 + dy) * 3 + dx] : 0.0f;
        const __bf16 h = (__bf16)v;
        o[j] = hl == 0 ? h : (__bf16)(v - (float)h);
    }
    out[i] = __builtin_bit_cast(u32x4, o);
}

// fp16 weight plane (MDTILE_PRECISION_F16): fp16_rn(w) in the layout and K order of k_conv_pack_bf16x3's hi plane -- the same record array
// [cb][k][dy][hl][dx][mt][lane], hl = 0: 8 fp16, hl = 1: zeros (the one-term kernels DMA both halves of a chunk and read the first), so the
// fp16 kernels address it exactly as their bf16 twins address the split image.  Source: the fp32 image [tap][cin][CoutP] at the head of the
// packed buffer of mdtile_conv_pack (the exact weights), so the plane can be built long after the OIHW tensor is gone.
__global__ void k_conv_pack_f16(const float* __restrict__ wp, u32x4* __restrict__ out, int Cout, int Cin, int CoutP, int MT, int NCB, int NK, int perm) {
    const size_t n = (size_t)NCB * NK * 3 * 2 * 3 * MT * 64;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    size_t r = i;
    const int lane = (int)(r % 64); r /= 64;
    const int mt = (int)(r % MT); r /= MT;
    const int dx = (int)(r % 3); r /= 3;
    const int hl = (int)(r % 2); r /= 2;
    const int dy = (int)(r % 3); r /= 3;
    const int k = (int)(r % NK); r /= NK;
    const int cb = (int)r;
    const int co = cb * MT * 32 + mt * 32 + (lane & 31);
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = kstep_c0(k, lane >> 5, perm) + kstep_cj(j, perm);
        v[j] = (hl == 0 && co < Cout && ci < Cin) ? wp[((size_t)(dy * 3 + dx) * Cin + ci) * CoutP + co] : 0.0f;
    }
    u32x4 o;
    cvt8h(v, o);
    out[i] = o;
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused nearest-2x upsample + 3x3 conv as FOUR 2x2 convs on the un-upsampled input ("sub-pixel" form): 2.25x fewer MACs.
//
// ldm's Upsample is F.interpolate(x, 2.0, 'nearest') followed by a 3x3 'same' conv (the queue's upsample.conv task,
// scripts/tilevae.py:139-153).  up[i][j] = in[i >> 1][j >> 1], so for output pixel (2y + a, 2x + b), a, b in {0, 1}, the
// three up-rows 2y+a-1 .. 2y+a+1 land on only TWO input rows:
//     a = 0:  rows {y-1, y, y}   ->  tap u=0 = w[dy=0] on row y-1,        tap u=1 = w[dy=1] + w[dy=2] on row y
//     a = 1:  rows {y, y, y+1}   ->  tap u=0 = w[dy=0] + w[dy=1] on row y, tap u=1 = w[dy=2] on row y+1
// i.e. input row offset = a + u - 1; columns alike with (b, v).  Zero padding is preserved exactly: up-row -1 <-> input
// row -1 and up-row 2H <-> input row H are the only out-of-range taps and the merged taps never straddle the border.
// The merged weights are summed in fp32 once at pack time (k_upconv_pack_bf16x3), then hi/lo split like the others.
//
// Block = 512 threads, BM couts x (8 x 32 INPUT px) = 16 x 64 output px of ONE row parity a (blockIdx carries a) and BOTH
// column parities: the accumulators of b = 0 and b = 1 sit in the same lane, so the epilogue stores float2 (x = 2X, 2X+1).
// K loop = phases (16-channel K-step, u): column shifts s = b + v in {0, 1, 2} share their input fragments between the
// parities -> per phase and wave 3 x NROW x 2 input + 4 x 2 x 2 weight fragment reads feed 4 x 2 x NROW x 3 MFMAs.
#define MDT_B3_TERMS 3
#define MDT_B3_KERNEL k_upconv_bf16x3
#include "vae_conv_bf16x3_upconv_body.h"
#undef MDT_B3_KERNEL
#undef MDT_B3_TERMS
#define MDT_B3_TERMS 1
#define MDT_B3_KERNEL k_upconv_bf16x1
#include "vae_conv_bf16x3_upconv_body.h"
#undef MDT_B3_KERNEL
#undef MDT_B3_TERMS

// OIHW fp32 -> merged-tap records [a][cb][k][u][hl][b][v][mt][lane] of 8 bf16 (see k_upconv_bf16x3): the taps of a row
// parity a / tap u are dy in {0} | {1,2} (a = 0) or {0,1} | {2} (a = 1); columns alike.  The merged weight is the fp32 sum
// in (dy, dx) order.
__global__ void k_upconv_pack_bf16x3(const float* __restrict__ w, u32x4* __restrict__ out, int Cout, int Cin, int MT, int NCB, int NK, int perm) {
    const size_t n = (size_t)2 * NCB * NK * 2 * 2 * 2 * 2 * MT * 64;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    size_t r = i;
    const int lane = (int)(r % 64); r /= 64;
    const int mt = (int)(r % MT); r /= MT;
    const int v = (int)(r % 2); r /= 2;
    const int bb = (int)(r % 2); r /= 2;
    const int hl = (int)(r % 2); r /= 2;
    const int u = (int)(r % 2); r /= 2;
    const int k = (int)(r % NK); r /= NK;
    const int cb = (int)(r % NCB); r /= NCB;
    const int a = (int)r;
    const int co = cb * MT * 32 + mt * 32 + (lane & 31);
    // tap sets: parity p, tap t -> [lo, hi) over the 3x3 index
    const int dy_lo = a == 0 ? (u == 0 ? 0 : 1) : (u == 0 ? 0 : 2), dy_hi = a == 0 ? (u == 0 ? 1 : 3) : (u == 0 ? 2 : 3);
    const int dx_lo = bb == 0 ? (v == 0 ? 0 : 1) : (v == 0 ? 0 : 2), dx_hi = bb == 0 ? (v == 0 ? 1 : 3) : (v == 0 ? 2 : 3);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = kstep_c0(k, lane >> 5, perm) + kstep_cj(j, perm);
        float val = 0.0f;
        if (co < Cout && ci < Cin)
            for (int dy = dy_lo; dy < dy_hi; ++dy)
                for (int dx = dx_lo; dx < dx_hi; ++dx) val += w[(((size_t)co * Cin + ci) * 3 + dy) * 3 + dx];
        const __bf16 h = (__bf16)val;
        o[j] = hl == 0 ? h : (__bf16)(val - (float)h);
    }
    out[i] = __builtin_bit_cast(u32x4, o);
}

}  // namespace

// shapes the split-bf16 3x3 kernel takes; everything else stays on the exact-fp32 kernel
bool mdt::conv_bf16x3_eligible(int cout, int cin, int ksize) { return ksize == 3 && cin % 16 == 0 && cout >= 32; }
// cout tiles per block: 128-cout blocks for the wide convs, 64-cout blocks for the small decoders' narrow ones
static int conv_bf16x3_mt(int cout) { return cout <= 64 ? 2 : 4; }
// K-step channel order (kstep_c0 / kstep_cj): the accumulator-lane order whenever whole 32-channel groups exist
static int conv_bf16x3_perm(int cin) { return cin % 32 == 0 ? 1 : 0; }

// record image = [ direct 3x3 records (9 taps) | sub-pixel upsample records (4 parities x 4 merged taps) ]
size_t mdt::conv_bf16x3_direct_records(int cout, int cin) {
    const int MT = conv_bf16x3_mt(cout), NCB = round_up(cout, MT * 32) / (MT * 32), NK = cin / 16;
    return (size_t)NCB * NK * 3 * 2 * 3 * MT * 64;
}
static size_t upconv_records(int cout, int cin) {
    const int MT = conv_bf16x3_mt(cout), NCB = round_up(cout, MT * 32) / (MT * 32), NK = cin / 16;
    return (size_t)2 * NCB * NK * 2 * 2 * 2 * 2 * MT * 64;
}
size_t mdt::conv_bf16x3_packed_floats(int cout, int cin) {   // size of the record array in floats (4 per 16-byte record)
    return (conv_bf16x3_direct_records(cout, cin) + upconv_records(cout, cin)) * 4;
}

int mdt::conv_bf16x3_pack(const float* d_w_oihw, void* d_out, int cout, int cin, hipStream_t s) {
    const int MT = conv_bf16x3_mt(cout), NCB = round_up(cout, MT * 32) / (MT * 32), NK = cin / 16, perm = conv_bf16x3_perm(cin);
    const size_t n = conv_bf16x3_direct_records(cout, cin);
    hipLaunchKernelGGL(k_conv_pack_bf16x3, dim3(cdiv((long long)n, 256)), dim3(256), 0, s, d_w_oihw, (u32x4*)d_out, cout, cin, MT, NCB, NK, perm);
    MDT_LAUNCH_CHECK();
    const size_t nu = upconv_records(cout, cin);
    hipLaunchKernelGGL(k_upconv_pack_bf16x3, dim3(cdiv((long long)nu, 256)), dim3(256), 0, s, d_w_oihw, (u32x4*)d_out + n, cout, cin, MT, NCB, NK, perm);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

// narrow convs (cout < 32: conv_out) only exist as a record-image kernel (vae_conv_rec.hip, one 32-cout tile per block): their
// packed image is the direct 3x3 records with MT = 1, NCB = 1, permuted K order
bool mdt::conv_rec_narrow_eligible(int cout, int cin, int ksize) { return ksize == 3 && cin % 32 == 0 && cout >= 1 && cout < 32; }
size_t mdt::conv_rec_narrow_packed_floats(int cin) { return (size_t)(cin / 16) * 3 * 2 * 3 * 1 * 64 * 4; }
int mdt::conv_rec_narrow_pack(const float* d_w_oihw, void* d_out, int cout, int cin, hipStream_t s) {
    const int NK = cin / 16;
    const size_t n = (size_t)NK * 3 * 2 * 3 * 64;
    hipLaunchKernelGGL(k_conv_pack_bf16x3, dim3(cdiv((long long)n, 256)), dim3(256), 0, s, d_w_oihw, (u32x4*)d_out, cout, cin, 1, 1, NK, 1);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

// fp16 weight plane of a 3x3 conv the record / hand-over kernels take: the size and geometry of the direct records of the split image
size_t mdt::conv_f16_plane_floats(int cout, int cin) {
    if (conv_rec_narrow_eligible(cout, cin, 3)) return conv_rec_narrow_packed_floats(cin);
    return conv_bf16x3_eligible(cout, cin, 3) ? conv_bf16x3_direct_records(cout, cin) * 4 : 0;
}
int mdt::conv_f16_pack(const float* d_w_f32img, void* d_out, int cout, int cin, hipStream_t s) {
    const bool narrow = conv_rec_narrow_eligible(cout, cin, 3);
    const int MT = narrow ? 1 : conv_bf16x3_mt(cout), NCB = narrow ? 1 : round_up(cout, MT * 32) / (MT * 32), NK = cin / 16;
    const int perm = narrow ? 1 : conv_bf16x3_perm(cin);
    const size_t n = (size_t)NCB * NK * 3 * 2 * 3 * MT * 64;
    hipLaunchKernelGGL(k_conv_pack_f16, dim3(cdiv((long long)n, 256)), dim3(256), 0, s, d_w_f32img, (u32x4*)d_out, cout, cin, round_up(cout, 32), MT, NCB, NK,
                       perm);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

bool mdt::conv_bf16x3_gn_supported(int cout, int cin, int ksize, int up) {
    return conv_bf16x3_eligible(cout, cin, ksize) && !up && cin <= MAX_GN_CIN;
}

// statistics in the epilogue (k_conv3x3_bf16x3<4, true, 1, true>): 128-cout blocks with the fused pre-activation, whole blocks of couts
bool mdt::conv_bf16x3_stats_supported(int cout, int cin, int ksize, int up) {
    return conv_bf16x3_gn_supported(cout, cin, ksize, up) && conv_bf16x3_mt(cout) == 4 && cout % 128 == 0;
}
// doubles of the per-block partials: [B][ptiles][NCB][32 quads][2]
size_t mdt::conv_bf16x3_stats_part_doubles(int B, int cout, int H, int W) {
    return (size_t)B * ((W + TW - 1) / TW) * ((H + TH - 1) / TH) * (cout / 128) * 64;
}

// The kernel of a launch from the seven facts that tell the instantiations apart: upsample, one-term arithmetic (MDTILE_PRECISION_BF16), the fp16
// weight plane, couts per block (MT x 32), fused pre-activation, statistics, stride.  conv_bf16x3_launch has refused every combination that has no kernel.
using ConvBKernel = void (*)(const ConvBParams);
static ConvBKernel conv_b_kernel(int up, bool one, int w16, int MT, bool gn, bool st, int stride) {
    const bool m4 = MT == 4;
    if (up) return one ? (m4 ? k_upconv_bf16x1<4> : k_upconv_bf16x1<2>) : (m4 ? k_upconv_bf16x3<4> : k_upconv_bf16x3<2>);
    if (stride == 2) return one ? (m4 ? k_conv3x3_bf16x1<4, false, 2> : k_conv3x3_bf16x1<2, false, 2>) : (m4 ? k_conv3x3_bf16x3<4, false, 2> : k_conv3x3_bf16x3<2, false, 2>);
    if (w16) return st ? k_conv3x3_f16<4, true, 1, true> : m4 ? k_conv3x3_f16<4, true> : k_conv3x3_f16<2, true>;
    if (one) return st ? k_conv3x3_bf16x1<4, true, 1, true> : gn ? (m4 ? k_conv3x3_bf16x1<4, true> : k_conv3x3_bf16x1<2, true>) : (m4 ? k_conv3x3_bf16x1<4, false> : k_conv3x3_bf16x1<2, false>);
    return st ? k_conv3x3_bf16x3<4, true, 1, true> : gn ? (m4 ? k_conv3x3_bf16x3<4, true> : k_conv3x3_bf16x3<2, true>) : (m4 ? k_conv3x3_bf16x3<4, false> : k_conv3x3_bf16x3<2, false>);
}

int mdt::conv_bf16x3_launch(const HandoverConvCall& c, hipStream_t s) {
    const int cin = c.cin, cout = c.cout, up = c.up, down = c.stride == 2, MT = conv_bf16x3_mt(cout);
    MDT_CHECK_ARG(c.stride == 1 || (down && !up && !c.res && !c.coef), "conv_bf16x3_launch: the stride-2 conv takes no upsample, residual or pre-activation (stride=%d)", c.stride);
    MDT_CHECK_ARG(!(up && c.coef), "conv_bf16x3_launch: no fused pre-activation in the sub-pixel upsample kernel");
    // w16 (MDTILE_PRECISION_F16, fused pre-activation only): w_rec is the fp16 weight plane -> k_conv3x3_f16
    MDT_CHECK_ARG(!c.w16 || (c.coef && !up), "conv_bf16x3_launch: the fp16 form exists for the fused pre-activation conv only");
    MDT_CHECK_ARG(!c.d_part || (MT == 4 && c.coef && !up && cout % 128 == 0), "conv_bf16x3_launch: no statistics kernel for cout=%d", cout);
    const ConvBKernel kernel = conv_b_kernel(up, mfma_single_term(), c.w16, MT, c.coef != nullptr, c.d_part != nullptr, c.stride);
    ConvBParams P;
    P.perm = conv_bf16x3_perm(cin);
    P.coef = c.coef;
    P.gn_part = c.d_part;
    // (up: the sub-pixel records, four 2x2 convs on the input grid, follow the direct ones)
    P.x = c.x; P.w = (const u32x4*)c.w_rec + (up ? conv_bf16x3_direct_records(cout, cin) : 0); P.bias = c.bias; P.res = c.res; P.y = c.y;
    P.B = c.B; P.Cin = cin; P.Cout = cout; P.H = c.H; P.W = c.W;
    P.Hin = down ? c.Hin : up ? c.H / 2 : c.H; P.Win = down ? c.Win : up ? c.W / 2 : c.W; P.up = up;
    P.NCB = round_up(cout, MT * 32) / (MT * 32);
    P.NK = cin / 16;
    // pixel tiles of 8 x 32 on the OUTPUT grid; sub-pixel form: on the INPUT grid, once per row parity
    P.PX = ((up ? P.Win : c.W) + TW - 1) / TW;
    P.ptiles = P.PX * (((up ? P.Hin : c.H) + TH - 1) / TH);
    dim3 grid(((P.ptiles + 7) / 8) * 8 * P.NCB * (up ? 2 : 1), c.B), block(512);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, P);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}
