// 8-bit image resampling, bit for bit what Pillow's Image.resize gives for Lanczos and Nearest on "RGB" and "L" images (the img2img upscale
// of scripts/tilediffusion.py, which the host runs on one CPU thread).  The result is DEFINED in include/mdtile.h:
//
//   mdtile_resample_table   per axis, on the HOST in double: for every output index the first source index, the tap count and the taps as
//                           22-bit fixed-point integers (Nearest: one tap of 2^22 at the accumulated-sum index)
//   k_resample_h            horizontal pass: src [H, W, C] -> [H, outW, C] bytes          (a wave = 64 output pixels of one row)
//   k_resample_v            vertical pass on rows of W * C flat bytes -> [outH, ...]      (a thread = 16 consecutive bytes of one row)
//
// The device code is integer only: int32 sums of byte x tap products are exact, so no byte depends on block shape or summation order.
#include "common.h"

#include <cmath>
#include <vector>

using namespace mdt;

namespace {
constexpr int RS_THREADS = 256;
constexpr int RS_WAVES = RS_THREADS / 64;
constexpr int RS_HCOLS = 64;                        // output columns of a block of the horizontal pass: one per lane
constexpr int RS_HROWS = 16;                        // rows of such a block: every wave walks RS_HROWS / RS_WAVES of them
constexpr int RS_HSEG = 4096;                       // LDS bytes per wave for the stretch of the input row its 64 columns read
constexpr int RS_KREG = 8;                          // taps per output held in registers (every upscale has ksize 7)
constexpr int RS_VBYTES = 16;                       // bytes of a row one thread of the vertical pass owns
constexpr int RS_PRECISION = 22;
constexpr double RS_PI = 3.14159265358979323846;    // M_PI

double sinc(double x) {
    if (x == 0.0) return 1.0;
    x = x * RS_PI;
    return std::sin(x) / x;
}
double lanczos3(double x) { return (-3.0 <= x && x < 3.0) ? sinc(x) * sinc(x / 3) : 0.0; }

// ksize of one axis, or 0 where the call is refused (the table [out][ksize] must stay below 2^31 entries)
int ksize_of(int in, int out, int filter) {
    if (in < 1 || out < 1) return 0;
    if (filter == MDTILE_RESAMPLE_NEAREST) return 1;
    if (filter != MDTILE_RESAMPLE_LANCZOS) return 0;
    const double scale = (double)in / (double)out;
    const double support = 3.0 * (scale < 1.0 ? 1.0 : scale);
    const double k = 2.0 * std::ceil(support) + 1.0;
    if (k * (double)out >= 2147483648.0) return 0;
    return (int)k;
}

// (first source index, taps) of one output as the table holds them, forced into the axis: a table that did not come from
// mdtile_resample_table may give wrong bytes, never an access outside the image
__device__ __forceinline__ int2 window_of(int2 b, int k, int size) {
    const int lo = min(max(b.x, 0), size - 1);
    return make_int2(lo, min(max(b.y, 0), min(k, size - lo)));
}

// clamp(acc >> 22, 0, 255), written as the clamp of acc to [0, 2^30) BEFORE the shift: the same value for every int acc.  In the shift-then-clamp
// form hipcc fuses two bytes of a packed word into one v_ashr_pk_u8_i32 and relies on the upper half of its result being zero, which an MI355X
// does not give (csrc/colorfix.hip: fix8).
__device__ __forceinline__ uint8_t clip8(int acc) { return (uint8_t)((uint32_t)min(max(acc, 0), (256 << RS_PRECISION) - 1) >> RS_PRECISION); }

// the taps of one output pixel over `px` (its first source pixel), from registers (REG: n <= RS_KREG, taps past n are zero) or from the table
template <int C, bool REG, typename P>
__device__ __forceinline__ void taps_h(P px, int n, const int (&creg)[RS_KREG], const int32_t* __restrict__ crow, int (&acc)[C]) {
    if constexpr (REG) {
#pragma unroll
        for (int t = 0; t < RS_KREG; ++t)
            if (t < n) {
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] += (int)px[t * C + c] * creg[t];
            }
    } else {
        for (int t = 0; t < n; ++t) {
            const int w = crow[t];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += (int)px[t * C + c] * w;
        }
    }
}

// Block = RS_HCOLS output columns x RS_HROWS rows; lane = column, wave = row (RS_HROWS / RS_WAVES rows each).  The windows of a strip's
// columns move right with the column, so the strip reads source pixels [first column's start, last column's end): that stretch of the row is
// staged in the wave's LDS slice when it fits RS_HSEG bytes (every upscale, downscales to about 1 / 19), and read from global memory otherwise.
template <int C, bool REG>
__global__ __launch_bounds__(RS_THREADS) void k_resample_h(const uint8_t* __restrict__ src, int H, int W, uint8_t* __restrict__ dst, int outW,
                                                            const int32_t* __restrict__ coef, const int2* __restrict__ bounds, int k, int strips) {
    __shared__ uint8_t seg[RS_WAVES][RS_HSEG];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int chunk = blockIdx.x / strips;
    const int x0 = (blockIdx.x - chunk * strips) * RS_HCOLS;
    const int xx = x0 + lane;
    const bool live = xx < outW;
    const int2 bf = window_of(bounds[x0], k, W), bl = window_of(bounds[min(x0 + RS_HCOLS, outW) - 1], k, W);
    const int s0 = bf.x, s1 = max(bl.x + bl.y, s0);
    const bool staged = (s1 - s0) * C <= RS_HSEG;                  // the same for the whole block
    int2 b = make_int2(s0, 0);
    if (live) b = window_of(bounds[xx], k, W);
    if (staged) {                                                  // holds for every table of mdtile_resample_table; see window_of
        b.x = min(max(b.x, s0), s1);
        b.y = min(b.y, s1 - b.x);
    }
    const int32_t* __restrict__ crow = coef + (size_t)(live ? xx : x0) * k;
    int creg[RS_KREG];
#pragma unroll
    for (int t = 0; t < RS_KREG; ++t) creg[t] = (REG && t < b.y) ? crow[t] : 0;
    const int nseg = (s1 - s0) * C;
    for (int r = 0; r < RS_HROWS / RS_WAVES; ++r) {
        const int y = chunk * RS_HROWS + r * RS_WAVES + wave;
        const bool row = y < H;
        const uint8_t* __restrict__ srow = src + (size_t)(row ? y : 0) * W * C;
        if (staged) {
            if (row)
                for (int j = lane; j < nseg; j += 64) seg[wave][j] = srow[(size_t)s0 * C + j];
            __syncthreads();
        }
        if (row && live) {
            int acc[C];
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] = 1 << (RS_PRECISION - 1);
            if (staged) taps_h<C, REG>(&seg[wave][(b.x - s0) * C], b.y, creg, crow, acc);
            else taps_h<C, REG>(srow + (size_t)b.x * C, b.y, creg, crow, acc);
            uint8_t* __restrict__ o = dst + ((size_t)y * outW + xx) * C;
#pragma unroll
            for (int c = 0; c < C; ++c) o[c] = clip8(acc[c]);
        }
        if (staged) __syncthreads();                               // the slice is rewritten for the next row
    }
}

// 16 bytes at any address (rows of W * C bytes start anywhere; gfx950 runs in unaligned-access mode: one 16-byte access)
struct __attribute__((packed, aligned(1))) u8x16_u { uint32_t v[4]; };

// Block = RS_THREADS * 16 consecutive bytes of ONE output row: first row, tap count and taps are the same for the whole block (uniform loads),
// every tap is one 16-byte load per thread of a contiguous 4 KiB run of source row ymin + t.
__global__ __launch_bounds__(RS_THREADS) void k_resample_v(const uint8_t* __restrict__ src, int H, int rowbytes, uint8_t* __restrict__ dst,
                                                            const int32_t* __restrict__ coef, const int2* __restrict__ bounds, int k, int colblocks) {
    const int yy = blockIdx.x / colblocks;
    const long long b0 = ((long long)(blockIdx.x - yy * colblocks) * RS_THREADS + threadIdx.x) * RS_VBYTES;
    if (b0 >= rowbytes) return;
    const int2 b = window_of(bounds[yy], k, H);
    const int32_t* __restrict__ crow = coef + (size_t)yy * k;
    const uint8_t* __restrict__ p = src + (size_t)b.x * rowbytes + b0;
    uint8_t* __restrict__ o = dst + (size_t)yy * rowbytes + b0;
    int acc[RS_VBYTES];
#pragma unroll
    for (int j = 0; j < RS_VBYTES; ++j) acc[j] = 1 << (RS_PRECISION - 1);
    if (b0 + RS_VBYTES <= rowbytes) {
        for (int t = 0; t < b.y; ++t, p += rowbytes) {
            const int w = crow[t];
            const u8x16_u v = *reinterpret_cast<const u8x16_u*>(p);
#pragma unroll
            for (int j = 0; j < RS_VBYTES; ++j) acc[j] += (int)((v.v[j >> 2] >> (8 * (j & 3))) & 255u) * w;
        }
        u8x16_u r;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            r.v[q] = (uint32_t)clip8(acc[4 * q]) | ((uint32_t)clip8(acc[4 * q + 1]) << 8) | ((uint32_t)clip8(acc[4 * q + 2]) << 16) |
                     ((uint32_t)clip8(acc[4 * q + 3]) << 24);
        *reinterpret_cast<u8x16_u*>(o) = r;
    } else {                                                       // the last bytes of a row, one by one
        const int m = (int)(rowbytes - b0);
        for (int t = 0; t < b.y; ++t, p += rowbytes) {
            const int w = crow[t];
#pragma unroll
            for (int j = 0; j < RS_VBYTES; ++j)
                if (j < m) acc[j] += (int)p[j] * w;
        }
#pragma unroll
        for (int j = 0; j < RS_VBYTES; ++j)
            if (j < m) o[j] = clip8(acc[j]);
    }
}

template <int C>
void launch_h(const uint8_t* src, int H, int W, uint8_t* dst, int outW, const int32_t* coef, const int32_t* bounds, int k, int strips,
              unsigned blocks, hipStream_t s) {
    if (k <= RS_KREG)
        hipLaunchKernelGGL((k_resample_h<C, true>), dim3(blocks), dim3(RS_THREADS), 0, s, src, H, W, dst, outW, coef, (const int2*)bounds, k, strips);
    else
        hipLaunchKernelGGL((k_resample_h<C, false>), dim3(blocks), dim3(RS_THREADS), 0, s, src, H, W, dst, outW, coef, (const int2*)bounds, k, strips);
}
}  // namespace

extern "C" int mdtile_resample_ksize(int in_size, int out_size, int filter) { return ksize_of(in_size, out_size, filter); }

extern "C" int mdtile_resample_table(int in_size, int out_size, int filter, int32_t* h_coef, int32_t* h_bounds) {
    MDT_CHECK_ARG(h_coef && h_bounds, "mdtile_resample_table: null argument");
    MDT_CHECK_ARG(filter == MDTILE_RESAMPLE_NEAREST || filter == MDTILE_RESAMPLE_LANCZOS, "mdtile_resample_table: unknown filter %d", filter);
    const int ksize = ksize_of(in_size, out_size, filter);
    MDT_CHECK_ARG(ksize > 0, "mdtile_resample_table: bad sizes %d -> %d (each >= 1, out * ksize below 2^31)", in_size, out_size);
    if (filter == MDTILE_RESAMPLE_NEAREST) {
        const double a = (double)in_size / (double)out_size;
        double xo = 0.5 * a;
        for (int xx = 0; xx < out_size; ++xx, xo += a) {           // the accumulated sum, not (xx + 0.5) * a: they differ in the last bit
            const int i = (int)xo;
            h_coef[xx] = 1 << RS_PRECISION;
            h_bounds[2 * xx] = i < in_size ? i : in_size - 1;
            h_bounds[2 * xx + 1] = 1;
        }
        return MDTILE_OK;
    }
    const double scale = (double)in_size / (double)out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * fs, ss = 1.0 / fs;
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = lanczos3((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int32_t* c = h_coef + (size_t)xx * ksize;
        for (int x = 0; x < ksize; ++x) {
            double v = 0.0;
            if (x < n) v = ww != 0.0 ? w[x] / ww : w[x];
            c[x] = v < 0 ? (int)(-0.5 + v * (1 << RS_PRECISION)) : (int)(0.5 + v * (1 << RS_PRECISION));
        }
        h_bounds[2 * xx] = xmin;
        h_bounds[2 * xx + 1] = n;
    }
    return MDTILE_OK;
}

static bool resample_sizes_ok(int H, int W, int C, int outH, int outW) {
    return H >= 1 && W >= 1 && outH >= 1 && outW >= 1 && (C == 1 || C == 3) && (long long)H * W * C < (1ll << 31) &&
           (long long)outH * outW * C < (1ll << 31);
}

extern "C" size_t mdtile_resample_u8_ws_size(int H, int W, int C, int outH, int outW) {
    if (!resample_sizes_ok(H, W, C, outH, outW)) return 0;
    return (size_t)H * outW * C;
}

extern "C" int mdtile_resample_u8(const uint8_t* d_src, int H, int W, int C, uint8_t* d_dst, int outH, int outW, const int32_t* d_cx,
                                  const int32_t* d_bx, int kx, const int32_t* d_cy, const int32_t* d_by, int ky, void* d_ws,
                                  mdtile_stream_t stream) {
    MDT_CHECK_ARG(d_src && d_dst, "mdtile_resample_u8: null argument");
    MDT_CHECK_ARG(C == 1 || C == 3, "mdtile_resample_u8: %d channels (1 = grey, 3 = RGB interleaved)", C);
    MDT_CHECK_ARG(resample_sizes_ok(H, W, C, outH, outW),
                  "mdtile_resample_u8: bad sizes %d x %d -> %d x %d (each >= 1, H * W * C and outH * outW * C below 2^31)", H, W, outH, outW);
    MDT_CHECK_ARG(kx >= 0 && ky >= 0, "mdtile_resample_u8: negative ksize (%d, %d)", kx, ky);
    MDT_CHECK_ARG(kx ? (d_cx && d_bx) : (!d_cx && !d_bx && outW == W),
                  "mdtile_resample_u8: the horizontal tables and kx go together; kx = 0 (no tables) needs outW == W (%d -> %d, kx %d)", W, outW, kx);
    MDT_CHECK_ARG(ky ? (d_cy && d_by) : (!d_cy && !d_by && outH == H),
                  "mdtile_resample_u8: the vertical tables and ky go together; ky = 0 (no tables) needs outH == H (%d -> %d, ky %d)", H, outH, ky);
    MDT_CHECK_ARG(!(kx && ky) || d_ws, "mdtile_resample_u8: two passes need the workspace of mdtile_resample_u8_ws_size");
    hipStream_t s = as_stream(stream);
    if (!kx && !ky) {
        MDT_HIP(hipMemcpyAsync(d_dst, d_src, (size_t)H * W * C, hipMemcpyDeviceToDevice, s));
        return MDTILE_OK;
    }
    const long long rowbytes = (long long)outW * C;
    const int strips = cdiv(outW, RS_HCOLS);
    const long long blocks_h = (long long)strips * cdiv(H, RS_HROWS);
    const int colblocks = cdiv(rowbytes, RS_THREADS * RS_VBYTES);
    const long long blocks_v = (long long)colblocks * outH;
    MDT_CHECK_ARG(rowbytes < (1ll << 31) && blocks_h < (1ll << 31) && blocks_v < (1ll << 31),
                  "mdtile_resample_u8: %d x %d -> %d x %d needs too many blocks", H, W, outH, outW);
    const uint8_t* vsrc = d_src;
    if (kx) {
        uint8_t* hdst = ky ? (uint8_t*)d_ws : d_dst;
        if (C == 3) launch_h<3>(d_src, H, W, hdst, outW, d_cx, d_bx, kx, strips, (unsigned)blocks_h, s);
        else launch_h<1>(d_src, H, W, hdst, outW, d_cx, d_bx, kx, strips, (unsigned)blocks_h, s);
        MDT_LAUNCH_CHECK();
        vsrc = hdst;
    }
    if (ky) {
        hipLaunchKernelGGL(k_resample_v, dim3((unsigned)blocks_v), dim3(RS_THREADS), 0, s, vsrc, H, (int)rowbytes, d_dst, d_cy, (const int2*)d_by, ky,
                           colblocks);
        MDT_LAUNCH_CHECK();
    }
    return MDTILE_OK;
}
