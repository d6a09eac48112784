// 1x1 conv tiles of the Tiled-VAE task queue (nin_shortcut of the channel-changing ResnetBlocks, q / k / proj_out of the
// mid-block attention; scripts/tilevae.py:115-137, tile_utils/attn.py:50-70) on the bf16 matrix cores with SPLIT-fp32
// operands -- the same arithmetic contract as vae_conv_bf16x3.hip (x = hi + lo, three bf16 MFMAs per product, fp32
// accumulation, ~1e-5 relative to fp32).  The exact-fp32 kernel (vae_conv.hip) remains behind MDTILE_CONV_EXACT_F32.
//
// A 1x1 conv is point-wise in space, so the image is treated as ONE flat run of H*W pixels: a block owns 256 consecutive
// pixels (8 MFMA column tiles of 32) x BM couts; every global load is a full 256-byte row per wave, there are no halos and
// no ragged rows.  GEMM view: D[cout][px] = sum_cin W[cout][cin] X[cin][px], MFMA v_mfma_f32_32x32x16_bf16 with
// A = weights (M = 32 couts, K = 16 cin), B = input (K = 16 cin, N = 32 px).
//   phase = 32 input channels (two 16-channel K-steps), ONE barrier per phase, register-prefetched double-buffered LDS:
//     input  LDS image  [hl][ks 2][kg 2][px 256] x 16 B   (record = 8 channels of one pixel)
//     weight LDS image  [hl][ks 2][mtile][lane 64] x 16 B  (exactly the pre-packed global order: straight copy)
//   every fragment read is a conflict-free ds_read_b128 of 32 consecutive records per half-wave.
// Block = 512 threads = 8 waves; wave = 64 couts x NCOL column tiles.
// These convs are HBM-bound on the wide images (nin_shortcut 256 -> 128 at 2224^2: 7.6 GB against 0.32 TFLOP), so (round 3)
//   * the operands of phase ph + 2 are requested while phase ph computes (two register sets): two phases = 64 KB of input per CU
//     in flight instead of one (measured before: 3.4 TB/s of traffic at one phase in flight, ~6 B/clk/CU);
//   * BM goes up to 256 couts (MT = 8: eight accumulator tiles per wave): 512 -> 256 reads its input once instead of twice.
#include <type_traits>

#include "launchers.h"

using namespace mdt;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace {

struct Conv1Params {
    const float* x;      // [B, Cin, HW] fp32
    const u32x4* w;      // packed bf16 hi/lo records, see k_conv1x1_pack_bf16x3
    const float* bias;   // [Cout] or null
    const float* res;    // residual [B, Cout, HW] or null
    float* y;            // [B, Cout, HW]
    int B, Cin, Cout;
    size_t HW;
    int ptiles, NCB, NP; // 256-pixel tiles, cout blocks, 32-channel phases
};


__device__ __forceinline__ void split8c(const float (&v)[8], u32x4& hi, u32x4& lo) {
    bf16x8 h, l;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        h[i] = (__bf16)v[i];
        l[i] = (__bf16)(v[i] - (float)h[i]);
    }
    hi = __builtin_bit_cast(u32x4, h);
    lo = __builtin_bit_cast(u32x4, l);
}

// PXT = pixels per block.  128-cout blocks take 128 px: 64 KB of LDS and ~100 registers -> TWO blocks per CU, so that the store-bound
// epilogue of one block (128 couts x 128 px x 4 B through 4-byte-per-lane stores) runs under the K loop of the other; with one
// resident block per CU the epilogue was fully exposed (256 -> 128 at 2224^2: ~30 us per block of which ~half epilogue).
#define MDT_C1_TERMS 3
#define MDT_C1_KERNEL k_conv1x1_bf16x3
#include "vae_conv1x1_body.h"
#undef MDT_C1_KERNEL
#undef MDT_C1_TERMS
#define MDT_C1_TERMS 1
#define MDT_C1_KERNEL k_conv1x1_bf16x1
#include "vae_conv1x1_body.h"
#undef MDT_C1_KERNEL
#undef MDT_C1_TERMS

// =====================================================================================================================
// Streaming form for the wide images (round 3): the convs above are HBM-bound there (7.6 GB against 0.32 TFLOP for 256 -> 128 at 2224^2)
// and moved their bytes with 4-byte-per-lane accesses in 0.5 .. 1 KB pieces per channel plane (3.4 - 3.6 TB/s).  Here
//   * a block owns 512 consecutive pixels x 128 couts; a phase is ONE 16-channel K-step: 16 rows of 2 KB, each fetched by two
//     back-to-back 1 KB LDS-DMA pieces (global_load_lds_dwordx4: 16 B per lane, no VGPRs, DRAM-page-sized runs per plane) into a
//     3-stage ring of raw fp32 [16 ch][512 px] (32 KB per stage); the weights of the K-step (8 KB of pre-packed records) ride the same
//     ring.  Two phases are in flight while one computes (the counted wait is vmcnt(5): every wave issues 4 + 1 pieces per phase);
//   * the hi / lo split happens on the LDS -> register path (8 ds_read_b32 of one pixel's channels + the split per B fragment): the
//     matrix pipe has time to spare here, the memory pipe has none;
//   * the epilogue goes through an LDS transpose (the ring is free by then): every global store -- and every residual load -- is
//     16 B per lane in 512-byte runs along a cout row, instead of 4 B per lane.
// Needs H*W % 4 == 0 (16-byte rows), cin % 32 == 0, cout % 128 == 0; everything else stays on the kernel above.
__device__ __forceinline__ void dma16s(const void* base, unsigned voff, const void* lds_dst) {
    const unsigned l = (unsigned)(__UINTPTR_TYPE__)(const __attribute__((address_space(3))) void*)lds_dst;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 2\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(base), "s"(l)
                 : "memory");
}

constexpr int S_NST = 3;

// WM = waves along the couts (64 each): WM = 2 -> block of 128 couts x 512 px, WM = 4 -> 256 couts x 256 px (a conv with cout % 256 == 0
// reads its input once).  Every wave owns 64 couts x 128 px = 2 x 4 accumulator tiles in both forms.
#define MDT_C1_TERMS 3
#define MDT_C1_KERNEL k_conv1x1_stream
#include "vae_conv1x1_stream_body.h"
#undef MDT_C1_KERNEL
#undef MDT_C1_TERMS
#define MDT_C1_TERMS 1
#define MDT_C1_KERNEL k_conv1x1_stream1t
#include "vae_conv1x1_stream_body.h"
#undef MDT_C1_KERNEL
#undef MDT_C1_TERMS

// OI fp32 -> records [cb][phase][hl][ks][mt][lane] of 8 bf16: cout = cb*BM + mt*32 + (lane & 31),
// cin = phase*32 + ks*16 + (lane >> 5)*8 + j.  Zero outside [Cout).
__global__ void k_conv1x1_pack_bf16x3(const float* __restrict__ w, u32x4* __restrict__ out, int Cout, int Cin, int MT, int NCB, int NP) {
    const size_t n = (size_t)NCB * NP * 2 * 2 * MT * 64;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    size_t r = i;
    const int lane = (int)(r % 64); r /= 64;
    const int mt = (int)(r % MT); r /= MT;
    const int ks = (int)(r % 2); r /= 2;
    const int hl = (int)(r % 2); r /= 2;
    const int ph = (int)(r % NP); r /= NP;
    const int cb = (int)r;
    const int co = cb * MT * 32 + mt * 32 + (lane & 31);
    bf16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ci = ph * 32 + ks * 16 + (lane >> 5) * 8 + j;
        const float v = (co < Cout && ci < Cin) ? w[(size_t)co * Cin + ci] : 0.0f;
        const __bf16 h = (__bf16)v;
        o[j] = hl == 0 ? h : (__bf16)(v - (float)h);
    }
    out[i] = __builtin_bit_cast(u32x4, o);
}

}  // namespace

bool mdt::conv1x1_bf16x3_eligible(int cout, int cin) { return cin % 32 == 0 && cout >= 32; }
// couts per block: 256 (one pass over the input for cout % 256 == 0), 128, or 64 for the small decoders' narrow convs
// (PROBES twin: MDTILE_C1X1_MT=4 keeps 128-cout blocks -- k_conv1x1_stream<2>, 512-px strips -- for cout % 256 == 0 too; read once: the
// weight packing depends on it.  Round 6 looked for the roof of k_conv1x1_stream<4> (2.2-3.4 TB/s, 280 TF-eq, 0.39 MFMA-busy, 7.1 VALU per
// MFMA; profiles/r6h): the block shape does not matter (256 x 256 vs 128 x 512: +-2 %), and neither does the VALU count -- a cooperative
// once-per-block split of the input into fragment records (1.9 VALU per MFMA, bit-identical, diff in profiles/r6h) ran the same times.  With
// cin = 512 the kernel needs ~5 TB/s of HBM AND ~10 TB/s of L2 -> LDS weight stream at full matrix rate: it sits at ~45 % of both.)
static int conv1x1_mt(int cout) {
    static const int cap = [] { const char* e = probe_env("MDTILE_C1X1_MT"); return e ? atoi(e) : 8; }();
    const int mt = cout > 128 ? 8 : (cout > 64 ? 4 : 2);
    return mt > cap ? cap : mt;
}
// MDTILE_C1X1_STREAM=0 (probes build only, read per launch): keep the plain kernel on the wide images too
static bool conv1x1_stream_on() {
    const char* e = probe_env("MDTILE_C1X1_STREAM");
    return !(e && e[0] == '0');
}

size_t mdt::conv1x1_bf16x3_packed_floats(int cout, int cin) {
    const int MT = conv1x1_mt(cout), NCB = round_up(cout, MT * 32) / (MT * 32), NP = cin / 32;
    return (size_t)NCB * NP * 2 * 2 * MT * 64 * 4;
}

int mdt::conv1x1_bf16x3_pack(const float* d_w_oihw, void* d_out, int cout, int cin, hipStream_t s) {
    const int MT = conv1x1_mt(cout), NCB = round_up(cout, MT * 32) / (MT * 32), NP = cin / 32;
    const size_t n = (size_t)NCB * NP * 2 * 2 * MT * 64;
    hipLaunchKernelGGL(k_conv1x1_pack_bf16x3, dim3(cdiv((long long)n, 256)), dim3(256), 0, s, d_w_oihw, (u32x4*)d_out, cout, cin, MT, NCB, NP);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

// The streaming kernel takes whole blocks of couts (MT = 4: k_conv1x1_stream<2>, 8: <4>) over 16-byte rows of a wide image
static bool conv1x1_streams(int MT, int cout, size_t HW) { return MT >= 4 && cout % (MT * 32) == 0 && HW % 4 == 0 && HW >= 2048 && conv1x1_stream_on(); }

// The kernel of a launch from (streaming, one-term arithmetic, MT) and the pixel strip of its blocks
using Conv1Kernel = void (*)(const Conv1Params);
static Conv1Kernel conv1x1_kernel(bool stream, bool one, int MT, int& strip) {
    strip = stream ? (MT == 4 ? 512 : 256) : (MT == 4 ? 128 : 256);
    if (stream) return one ? (MT == 4 ? k_conv1x1_stream1t<2> : k_conv1x1_stream1t<4>) : (MT == 4 ? k_conv1x1_stream<2> : k_conv1x1_stream<4>);
    if (one) return MT == 8 ? k_conv1x1_bf16x1<8, 256> : MT == 4 ? k_conv1x1_bf16x1<4, 128> : k_conv1x1_bf16x1<2, 256>;
    return MT == 8 ? k_conv1x1_bf16x3<8, 256> : MT == 4 ? k_conv1x1_bf16x3<4, 128> : k_conv1x1_bf16x3<2, 256>;
}

int mdt::conv1x1_bf16x3_launch(const float* d_x, const void* d_w_rec, const float* d_bias, const float* d_res, float* d_y, int B, int cin,
                          int cout, size_t HW, hipStream_t s, bool attn_proj) {
    // MDTILE_PRECISION_F16: q / k / v / proj_out of the attention (the caller says so: MDTILE_CONV_ATTN_PROJ) run one-term bf16 like the attention
    // itself; every other 1x1 conv (nin_shortcut) reads the raw stream and keeps its three terms
    const bool one = mfma_single_term() || (attn_proj && mode_f16());
    const int MT = conv1x1_mt(cout);
    int strip;
    const Conv1Kernel kernel = conv1x1_kernel(conv1x1_streams(MT, cout, HW), one, MT, strip);
    Conv1Params P;
    P.x = d_x; P.w = (const u32x4*)d_w_rec; P.bias = d_bias; P.res = d_res; P.y = d_y;
    P.B = B; P.Cin = cin; P.Cout = cout; P.HW = HW;
    P.ptiles = (int)((HW + strip - 1) / strip);
    P.NCB = round_up(cout, MT * 32) / (MT * 32);
    P.NP = cin / 32;
    dim3 grid(((P.ptiles + 7) / 8) * 8 * P.NCB, B), block(512);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, P);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}
