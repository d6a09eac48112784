// Colour fix of an img2img result against its init image, on bytes (the results are DEFINED in include/mdtile.h).
//
//   wavelet   out = clamp((content * 2^20 + low5(style - content) + 2^19) >> 20, 0, 255), low5 = five [1,2,1] levels of dilation 1, 2, 4, 8, 16
//             along y, then five along x, every level's index clamped to the image.  Two launches around an int32 intermediate:
//     k_cf_vert   d = style - content from the bytes, the five y levels   -> int32 [H, W * C]      (block = 64 rows x 64 flat columns + 31 rows of halo)
//     k_cf_horz   the five x levels on the intermediate, + content, round, clamp -> bytes          (block = 1024 pixels of one row + 31 pixels of halo)
//   adain     k_hist_u8 (exact uint32 counts per channel), the 256-entry tables on the host (mdtile/__init__.py: adain_lut), k_lut_u8.
//
// Integer only: sums of integers are exact, so no byte depends on block shape, pass order or summation order.
//
// The halo argument, for both passes.  A block stages the stretch [lo, hi) = [max(o0 - 31, 0), min(o1 + 31, n)) of an axis of length n around its
// outputs [o0, o1), and every level clamps its index to [lo, hi).  Where lo = 0 or hi = n that IS the clamp to the image.  Where it is not, the
// clamped read is wrong for that position -- and a wrong value at level k spreads by 2^k positions, 1 + 2 + 4 + 8 + 16 = 31 in all, so it ends
// just outside [o0, o1).  Wrong values are still sums of staged values with the same weights: the 2^28 bound of the header holds for them too.
#include "common.h"

using namespace mdt;

namespace {
constexpr int CF_THREADS = 256;
constexpr int CF_LEVELS = 5;
constexpr int CF_HALO = 31;                          // 2^5 - 1
constexpr int CF_SHIFT = 20;                         // ten levels of weight 4
constexpr int CF_VROWS = 64;                         // output rows of a block of the vertical pass
constexpr int CF_VCOLS = 64;                         // its flat columns (bytes of a row): 16 threads x 4
constexpr int CF_VSTAGE = CF_VROWS + 2 * CF_HALO;    // 126 staged rows; 2 buffers x 126 x 64 x 4 B = 63 KiB of LDS
constexpr int CF_HPIX = 1024;                        // output pixels of a block of the horizontal pass
constexpr int CF_HSTAGE = CF_HPIX + 2 * CF_HALO;     // 1086 staged pixels; 2 buffers x 1086 x C x 4 B = 25.5 KiB of LDS for RGB
constexpr int CF_PW_BYTES = 16;                      // bytes per thread and step of the pointwise kernels (histogram, table)
constexpr int CF_PW_BLOCKS = 2048;                   // grid cap of the pointwise kernels (grid-stride beyond)

// 4 / 16 bytes and 4 ints at any address (rows of W * C bytes start anywhere; gfx950 runs in unaligned-access mode)
struct __attribute__((packed, aligned(1))) u8x4_u { uint32_t v; };
struct __attribute__((packed, aligned(1))) u8x16_u { uint32_t v[4]; };
struct __attribute__((packed, aligned(4))) i32x4_u { int v[4]; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
// clamp(t >> 20, 0, 255), written as the clamp of t to [0, 2^28) BEFORE the shift: the same value for every int t.  In the shift-then-clamp
// form hipcc fuses two such bytes into one v_ashr_pk_u8_i32 and ORs the other two bytes of the word onto its result as if the upper half of that
// result were zero; on an MI355X it was not (bytes 2 and 3 of every packed word came back ORed with bits 16 .. 31 of byte 0's sum).
__device__ __forceinline__ uint32_t fix8(uint32_t content, int v) {
    const int t = (int)(content << CF_SHIFT) + v + (1 << (CF_SHIFT - 1));
    return (uint32_t)clampi(t, 0, (256 << CF_SHIFT) - 1) >> CF_SHIFT;
}

// Vertical pass.  Block = rows [y0, y0 + 64) x flat columns [c0, c0 + 64) of the image seen as [H, rowbytes]; thread = 4 columns of a row, so
// every LDS access is one 16-byte slot and a wave touches 4 whole rows of 256 B: conflict-free.
__global__ __launch_bounds__(CF_THREADS) void k_cf_vert(const uint8_t* __restrict__ content, const uint8_t* __restrict__ style,
                                                         int* __restrict__ mid, int H, int rowbytes, int colblocks) {
    __shared__ int4 buf[2][CF_VSTAGE][CF_VCOLS / 4];
    const int rb = blockIdx.x / colblocks;
    const int c0 = (blockIdx.x - rb * colblocks) * CF_VCOLS;
    const int y0 = rb * CF_VROWS;
    const int lo = max(y0 - CF_HALO, 0), hi = min(y0 + CF_VROWS + CF_HALO, H);
    const int nr = hi - lo;                                        // 1 .. 126
    const int ncols = min(CF_VCOLS, rowbytes - c0);                // 1 .. 64
    const int items = nr * (CF_VCOLS / 4);
    for (int it = threadIdx.x; it < items; it += CF_THREADS) {
        const int row = it >> 4, q = it & 15, col = q * 4;
        int4 d = make_int4(0, 0, 0, 0);
        const size_t off = (size_t)(lo + row) * rowbytes + c0 + col;
        if (col + 4 <= ncols) {
            const uint32_t c = reinterpret_cast<const u8x4_u*>(content + off)->v, s = reinterpret_cast<const u8x4_u*>(style + off)->v;
            d.x = (int)(s & 255u) - (int)(c & 255u);
            d.y = (int)((s >> 8) & 255u) - (int)((c >> 8) & 255u);
            d.z = (int)((s >> 16) & 255u) - (int)((c >> 16) & 255u);
            d.w = (int)(s >> 24) - (int)(c >> 24);
        } else if (col < ncols) {                                  // the last bytes of a row, one by one
            int t[4] = {0, 0, 0, 0};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (col + j < ncols) t[j] = (int)style[off + j] - (int)content[off + j];
            d = make_int4(t[0], t[1], t[2], t[3]);
        }
        buf[0][row][q] = d;
    }
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int k = 0; k < CF_LEVELS; ++k) {
        const int r = 1 << k;
        for (int it = threadIdx.x; it < items; it += CF_THREADS) {
            const int row = it >> 4, q = it & 15;
            const int4 a = buf[cur][max(row - r, 0)][q], b = buf[cur][row][q], c = buf[cur][min(row + r, nr - 1)][q];
            buf[cur ^ 1][row][q] = make_int4(a.x + 2 * b.x + c.x, a.y + 2 * b.y + c.y, a.z + 2 * b.z + c.z, a.w + 2 * b.w + c.w);
        }
        __syncthreads();
        cur ^= 1;
    }
    const int nout = min(CF_VROWS, H - y0);
    for (int it = threadIdx.x; it < nout * (CF_VCOLS / 4); it += CF_THREADS) {
        const int row = it >> 4, q = it & 15, col = q * 4;
        const int4 v = buf[cur][y0 - lo + row][q];
        int* __restrict__ o = mid + (size_t)(y0 + row) * rowbytes + c0 + col;
        if (col + 4 <= ncols) {
            i32x4_u t;
            t.v[0] = v.x, t.v[1] = v.y, t.v[2] = v.z, t.v[3] = v.w;
            *reinterpret_cast<i32x4_u*>(o) = t;
        } else if (col < ncols) {
            const int t[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (col + j < ncols) o[j] = t[j];
        }
    }
}

// Horizontal pass.  Block = pixels [x0, x0 + 1024) of one row; the staged stretch holds np pixels of C ints, element e = pixel * C + channel, and a
// level reads the same channel of the pixels r to the left and right: lanes read consecutive ints, conflict-free.
template <int C>
__global__ __launch_bounds__(CF_THREADS) void k_cf_horz(const uint8_t* __restrict__ content, const int* __restrict__ mid, uint8_t* __restrict__ out,
                                                         int W, int strips) {
    __shared__ int buf[2][CF_HSTAGE * C];
    const int y = blockIdx.x / strips;
    const int x0 = (blockIdx.x - y * strips) * CF_HPIX;
    const int lo = max(x0 - CF_HALO, 0), hi = min(x0 + CF_HPIX + CF_HALO, W);
    const int np = hi - lo, ne = np * C;                           // 1 .. 1086 pixels
    const size_t rowoff = (size_t)y * W * C;
    const int* __restrict__ m = mid + rowoff + (size_t)lo * C;
    for (int e = threadIdx.x; e < ne; e += CF_THREADS) buf[0][e] = m[e];
    __syncthreads();
    int cur = 0;
#pragma unroll
    for (int k = 0; k < CF_LEVELS; ++k) {
        const int r = 1 << k;
        for (int e = threadIdx.x; e < ne; e += CF_THREADS) {
            const int p = e / C, c = e - p * C;
            buf[cur ^ 1][e] = buf[cur][max(p - r, 0) * C + c] + 2 * buf[cur][e] + buf[cur][min(p + r, np - 1) * C + c];
        }
        __syncthreads();
        cur ^= 1;
    }
    const int nout = (min(x0 + CF_HPIX, W) - x0) * C;              // bytes this block writes
    const int* __restrict__ v = &buf[cur][(x0 - lo) * C];
    const size_t o0 = rowoff + (size_t)x0 * C;
    for (int e = threadIdx.x * 4; e < nout; e += CF_THREADS * 4) {
        if (e + 4 <= nout) {
            const uint32_t c = reinterpret_cast<const u8x4_u*>(content + o0 + e)->v;
            u8x4_u t;
            t.v = fix8(c & 255u, v[e]) | (fix8((c >> 8) & 255u, v[e + 1]) << 8) | (fix8((c >> 16) & 255u, v[e + 2]) << 16) | (fix8(c >> 24, v[e + 3]) << 24);
            *reinterpret_cast<u8x4_u*>(out + o0 + e) = t;
        } else {
            for (int j = e; j < nout; ++j) out[o0 + j] = (uint8_t)fix8(content[o0 + j], v[j]);
        }
    }
}

// Counts of every byte value per channel.  Block-private counts in LDS (integer adds: any order gives the same counts), then one integer add per
// non-empty bin and block into the global table, which the caller has zeroed.  Thread = 16 consecutive bytes per step; the channel of flat byte f
// is f % C.
template <int C>
__global__ __launch_bounds__(CF_THREADS) void k_hist_u8(const uint8_t* __restrict__ img, unsigned n, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[C * 256];
    for (int i = threadIdx.x; i < C * 256; i += CF_THREADS) h[i] = 0;
    __syncthreads();
    const unsigned chunks = (n + CF_PW_BYTES - 1) / CF_PW_BYTES;
    for (unsigned i = blockIdx.x * CF_THREADS + threadIdx.x; i < chunks; i += gridDim.x * CF_THREADS) {
        const unsigned f0 = i * CF_PW_BYTES;                       // below 2^31
        const unsigned c0 = f0 % C;
        if (f0 + CF_PW_BYTES <= n) {
            const u8x16_u v = *reinterpret_cast<const u8x16_u*>(img + f0);
#pragma unroll
            for (int j = 0; j < CF_PW_BYTES; ++j) atomicAdd(&h[((c0 + j) % C) * 256 + ((v.v[j >> 2] >> (8 * (j & 3))) & 255u)], 1u);
        } else {
            for (unsigned j = 0; f0 + j < n; ++j) atomicAdd(&h[((c0 + j) % C) * 256 + img[f0 + j]], 1u);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * 256; i += CF_THREADS)
        if (h[i]) atomicAdd(&hist[i], h[i]);
}

// out[f] = lut[f % C][img[f]]; the tables sit in LDS
template <int C>
__global__ __launch_bounds__(CF_THREADS) void k_lut_u8(const uint8_t* __restrict__ img, unsigned n, const uint8_t* __restrict__ lut,
                                                        uint8_t* __restrict__ out) {
    __shared__ uint8_t t[C * 256];
    for (int i = threadIdx.x; i < C * 256; i += CF_THREADS) t[i] = lut[i];
    __syncthreads();
    const unsigned chunks = (n + CF_PW_BYTES - 1) / CF_PW_BYTES;
    for (unsigned i = blockIdx.x * CF_THREADS + threadIdx.x; i < chunks; i += gridDim.x * CF_THREADS) {
        const unsigned f0 = i * CF_PW_BYTES;
        const unsigned c0 = f0 % C;
        if (f0 + CF_PW_BYTES <= n) {
            const u8x16_u v = *reinterpret_cast<const u8x16_u*>(img + f0);
            u8x16_u r;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t w = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) w |= (uint32_t)t[((c0 + 4 * q + b) % C) * 256 + ((v.v[q] >> (8 * b)) & 255u)] << (8 * b);
                r.v[q] = w;
            }
            *reinterpret_cast<u8x16_u*>(out + f0) = r;
        } else {
            for (unsigned j = 0; f0 + j < n; ++j) out[f0 + j] = t[((c0 + j) % C) * 256 + img[f0 + j]];
        }
    }
}

bool image_ok(int H, int W, int C) { return H >= 1 && W >= 1 && (C == 1 || C == 3) && (long long)H * W * C < (1ll << 31); }

unsigned pointwise_blocks(unsigned n) {
    const unsigned chunks = (n + CF_PW_BYTES - 1) / CF_PW_BYTES;
    const unsigned blocks = (chunks + CF_THREADS - 1) / CF_THREADS;
    return blocks < (unsigned)CF_PW_BLOCKS ? blocks : (unsigned)CF_PW_BLOCKS;
}
}  // namespace

extern "C" size_t mdtile_colorfix_wavelet_ws_size(int H, int W, int C) {
    if (!image_ok(H, W, C)) return 0;
    return (size_t)H * W * C * sizeof(int);
}

extern "C" int mdtile_colorfix_wavelet(const uint8_t* d_content, const uint8_t* d_style, uint8_t* d_out, int H, int W, int C, void* d_ws,
                                       mdtile_stream_t stream) {
    MDT_CHECK_ARG(d_content && d_style && d_out && d_ws, "mdtile_colorfix_wavelet: null argument");
    MDT_CHECK_ARG(C == 1 || C == 3, "mdtile_colorfix_wavelet: %d channels (1 = grey, 3 = RGB interleaved)", C);
    MDT_CHECK_ARG(image_ok(H, W, C), "mdtile_colorfix_wavelet: bad sizes %d x %d (each >= 1, H * W * C below 2^31)", H, W);
    MDT_CHECK_ARG(((uintptr_t)d_ws & 15) == 0, "mdtile_colorfix_wavelet: the workspace must be 16-byte aligned");
    const long long rowbytes = (long long)W * C;
    const int colblocks = cdiv(rowbytes, CF_VCOLS), strips = cdiv(W, CF_HPIX);
    const long long blocks_v = (long long)colblocks * cdiv(H, CF_VROWS), blocks_h = (long long)strips * H;
    MDT_CHECK_ARG(blocks_v < (1ll << 31) && blocks_h < (1ll << 31), "mdtile_colorfix_wavelet: %d x %d needs too many blocks", H, W);
    hipStream_t s = as_stream(stream);
    int* mid = (int*)d_ws;
    hipLaunchKernelGGL(k_cf_vert, dim3((unsigned)blocks_v), dim3(CF_THREADS), 0, s, d_content, d_style, mid, H, (int)rowbytes, colblocks);
    MDT_LAUNCH_CHECK();
    if (C == 3) hipLaunchKernelGGL(k_cf_horz<3>, dim3((unsigned)blocks_h), dim3(CF_THREADS), 0, s, d_content, mid, d_out, W, strips);
    else hipLaunchKernelGGL(k_cf_horz<1>, dim3((unsigned)blocks_h), dim3(CF_THREADS), 0, s, d_content, mid, d_out, W, strips);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_hist_u8(const uint8_t* d_img, int H, int W, int C, uint32_t* d_hist, mdtile_stream_t stream) {
    MDT_CHECK_ARG(d_img && d_hist, "mdtile_hist_u8: null argument");
    MDT_CHECK_ARG(C == 1 || C == 3, "mdtile_hist_u8: %d channels (1 = grey, 3 = RGB interleaved)", C);
    MDT_CHECK_ARG(image_ok(H, W, C), "mdtile_hist_u8: bad sizes %d x %d (each >= 1, H * W * C below 2^31)", H, W);
    hipStream_t s = as_stream(stream);
    const unsigned n = (unsigned)((long long)H * W * C);
    MDT_HIP(hipMemsetAsync(d_hist, 0, (size_t)C * 256 * sizeof(uint32_t), s));
    if (C == 3) hipLaunchKernelGGL(k_hist_u8<3>, dim3(pointwise_blocks(n)), dim3(CF_THREADS), 0, s, d_img, n, d_hist);
    else hipLaunchKernelGGL(k_hist_u8<1>, dim3(pointwise_blocks(n)), dim3(CF_THREADS), 0, s, d_img, n, d_hist);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_lut_u8(const uint8_t* d_img, int H, int W, int C, const uint8_t* d_lut, uint8_t* d_out, mdtile_stream_t stream) {
    MDT_CHECK_ARG(d_img && d_lut && d_out, "mdtile_lut_u8: null argument");
    MDT_CHECK_ARG(C == 1 || C == 3, "mdtile_lut_u8: %d channels (1 = grey, 3 = RGB interleaved)", C);
    MDT_CHECK_ARG(image_ok(H, W, C), "mdtile_lut_u8: bad sizes %d x %d (each >= 1, H * W * C below 2^31)", H, W);
    hipStream_t s = as_stream(stream);
    const unsigned n = (unsigned)((long long)H * W * C);
    if (C == 3) hipLaunchKernelGGL(k_lut_u8<3>, dim3(pointwise_blocks(n)), dim3(CF_THREADS), 0, s, d_img, n, d_lut, d_out);
    else hipLaunchKernelGGL(k_lut_u8<1>, dim3(pointwise_blocks(n)), dim3(CF_THREADS), 0, s, d_img, n, d_lut, d_out);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}
