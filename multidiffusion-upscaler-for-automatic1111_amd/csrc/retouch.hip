// Noise Inversion's renoise mask (tile_utils/utils.py:216-247 and tile_methods/abstractdiffusion.py:607-621 upstream): where the init
// image carries detail, as the residue of a self-guided box filter (guided filter with guide = input, eps 0.01) quantised to uint8 levels,
// then resized to the latent grid and scaled by the renoise strength.  Upstream runs the filter with OpenCV on the CPU over the full-size
// image; here it is three kernels whose result is DEFINED exactly (include/mdtile.h), so that it can be checked bit for bit:
//
//   k_retouch_rows   grey conversion + horizontal window sums of L and L^2 per row       (block scan, O(1) per pixel for every k)
//   k_retouch_cols   vertical sliding sums of the row sums + the fp32 filter arithmetic   (O(k) start-up per chunk of rows)
//   k_renoise_resize clamp((1 - bilinear(mask)) * strength, 0, 1) on the latent grid      (torch's align_corners = False rule)
//
// Window sums are exact integers (independent of summation order, block shape and chunking); everything after them is a fixed sequence of
// single correctly rounded operations (this library is built with -ffp-contract=off; / is IEEE in fp32 and fp64).
#include "common.h"

using namespace mdt;

namespace {
constexpr int RT_THREADS = 256;
constexpr int RT_ELEMS = 8;                        // consecutive row elements one thread scans
constexpr int RT_N = RT_THREADS * RT_ELEMS;        // 2048 staged elements per block = segment + window halo
constexpr int RT_SEG_MAX = 1536;                   // output pixels per block: RT_SEG_MAX + 512 - 1 <= RT_N - 1
constexpr int RT_KMAX = 512;
static_assert(RT_SEG_MAX + RT_KMAX - 1 < RT_N, "a segment and its halo must fit one block scan");

// BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba) as the triangle wave of period 2 (n - 1): any distance outside the image is legal.
__device__ __forceinline__ int reflect101(int i, int n) {
    if ((unsigned)i < (unsigned)n) return i;
    if (n == 1) return 0;
    const long long p = 2ll * (n - 1);
    long long r = (long long)i % p;
    if (r < 0) r += p;
    return (int)(r < n ? r : p - r);
}

// PIL's "L" conversion (ITU-R 601-2 luma in 16.16 fixed point, rounded): exact against Image.convert("L").
template <int CH>
__device__ __forceinline__ unsigned grey_of(const uint8_t* __restrict__ px) {
    if constexpr (CH == 1) return px[0];
    else return (19595u * px[0] + 38470u * px[1] + 7471u * px[2] + 0x8000u) >> 16;
}

// prefix arrays are padded by one word per 8 so that the 8-element runs of neighbouring lanes start on different LDS banks
__device__ __forceinline__ int pidx(int j) { return j + (j >> 3); }

// One block = one row segment of `seg` (<= RT_SEG_MAX) output pixels.  Element j of the block is the grey value at column
// x0 - k/2 + j (reflected); output i sums elements i .. i + k - 1 and its own pixel is element i + k/2.
// ws[y * W + x] = { rowsum(L) | L << 24,  rowsum(L^2) }   (rowsum(L) <= 512 * 255 < 2^24, rowsum(L^2) <= 512 * 65025 < 2^32)
template <int CH>
__global__ __launch_bounds__(RT_THREADS) void k_retouch_rows(const uint8_t* __restrict__ img, int W, int k, int seg, int nseg,
                                                              uint2* __restrict__ ws) {
    __shared__ __attribute__((aligned(8))) uint8_t G[RT_N];
    __shared__ unsigned P1[RT_N + RT_N / 8 + 1], P2[RT_N + RT_N / 8 + 1];
    __shared__ unsigned wtot[2][RT_THREADS / 64];
    const int t = threadIdx.x;
    const int y = blockIdx.x / nseg, x0 = (blockIdx.x - y * nseg) * seg;
    const int nout = min(seg, W - x0);
    if (nout <= 0) return;               // rounding seg up can leave the last segments of a very wide row empty (whole block, before any barrier)
    const int need = nout + k - 1;
    const uint8_t* __restrict__ row = img + (size_t)y * W * CH;
    const int xs0 = x0 - k / 2;
    for (int j = t; j < RT_N; j += RT_THREADS) {
        unsigned g = 0;
        if (j < need) g = grey_of<CH>(row + (size_t)reflect101(xs0 + j, W) * CH);
        G[j] = (uint8_t)g;
    }
    __syncthreads();
    unsigned a1[RT_ELEMS], a2[RT_ELEMS];
    {
        const uint2 g8 = *reinterpret_cast<const uint2*>(&G[t * RT_ELEMS]);
        unsigned s1 = 0, s2 = 0;
#pragma unroll
        for (int e = 0; e < RT_ELEMS; ++e) {
            const unsigned g = ((e < 4 ? g8.x : g8.y) >> (8 * (e & 3))) & 255u;
            s1 += g;
            s2 += g * g;
            a1[e] = s1;
            a2[e] = s2;
        }
    }
    // exclusive block scan of the per-thread totals: inclusive wave scan, then the totals of the waves in front.  The L^2 prefix may
    // pass 2^32 on no row this block can see (2048 * 65025 < 2^32), and differences of unsigned words would be exact even so.
    unsigned v1 = a1[RT_ELEMS - 1], v2 = a2[RT_ELEMS - 1];
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned n1 = __shfl_up(v1, off, 64), n2 = __shfl_up(v2, off, 64);
        if (lane >= off) { v1 += n1; v2 += n2; }
    }
    if (lane == 63) { wtot[0][wave] = v1; wtot[1][wave] = v2; }
    __syncthreads();
    unsigned e1 = v1 - a1[RT_ELEMS - 1], e2 = v2 - a2[RT_ELEMS - 1];
    for (int w = 0; w < wave; ++w) { e1 += wtot[0][w]; e2 += wtot[1][w]; }
    if (t == 0) { P1[0] = 0; P2[0] = 0; }
#pragma unroll
    for (int e = 0; e < RT_ELEMS; ++e) {       // P[j] = sum of the elements in front of j
        const int j = t * RT_ELEMS + e + 1;
        P1[pidx(j)] = e1 + a1[e];
        P2[pidx(j)] = e2 + a2[e];
    }
    __syncthreads();
    uint2* __restrict__ out = ws + (size_t)y * W + x0;
    const int half = k / 2;
    for (int i = t; i < nout; i += RT_THREADS) {
        const unsigned s1 = P1[pidx(i + k)] - P1[pidx(i)];
        const unsigned s2 = P2[pidx(i + k)] - P2[pidx(i)];
        out[i] = make_uint2(s1 | ((unsigned)G[i + half] << 24), s2);
    }
}

// One thread = one column of one chunk of R rows: the window sums of the first row are gathered from k row sums, every further row adds
// the row entering the window and subtracts the one leaving it.  S2 <= 512^2 * 65025 = 1.7e10 needs 64 bits.  The row indices are uniform
// over the block (scalar), the 8-byte loads of a wave are one contiguous 512-byte run.
__global__ __launch_bounds__(RT_THREADS) void k_retouch_cols(const uint2* __restrict__ ws, int H, int W, int k, int R, int colblocks,
                                                              float* __restrict__ mask) {
    const int chunk = blockIdx.x / colblocks;
    const int x = (blockIdx.x - chunk * colblocks) * RT_THREADS + threadIdx.x;
    if (x >= W) return;
    const int y0 = chunk * R, y1 = min(y0 + R, H);      // y0 + R <= H + R: no overflow (H * W < 2^31, R <= 256)
    const int half = k / 2;
    unsigned S1 = 0;
    unsigned long long S2 = 0;
    for (int r = 0; r < k; ++r) {
        const uint2 v = ws[(size_t)reflect101(y0 - half + r, H) * W + x];
        S1 += v.x & 0xffffffu;
        S2 += v.y;
    }
    const double n = (double)k * (double)k;
    const double d1 = 255.0 * n, d2 = 65025.0 * n;
    for (int y = y0; y < y1; ++y) {
        const size_t o = (size_t)y * W + x;
        const float img = (float)(ws[o].x >> 24) / 255.0f;
        const float mean = (float)((double)S1 / d1);
        const float msq = (float)((double)S2 / d2);
        const float var = msq - mean * mean;
        const float a = var / (var + 0.01f);           // cov(I, I) / (var(I) + eps)
        const float b = mean - a * mean;
        const float gf = ((a * img + b) - img) * 255.0f;
        const int q = (int)truncf(gf) & 255;           // upstream's astype(uint8): toward zero, negatives wrap
        mask[o] = (float)q / 255.0f;
        if (y + 1 < y1) {
            const uint2 in = ws[(size_t)reflect101(y - half + k, H) * W + x];
            const uint2 ou = ws[(size_t)reflect101(y - half, H) * W + x];
            S1 += (in.x & 0xffffffu) - (ou.x & 0xffffffu);
            S2 += in.y;
            S2 -= ou.y;
        }
    }
}

// area_pixel_compute_source_index of torch's bilinear resize with align_corners = False, in fp32
__device__ __forceinline__ void bilinear_tap(int dst, float scale, int n, int& i0, int& i1, float& l0, float& l1) {
    const float src = fmaxf(scale * ((float)dst + 0.5f) - 0.5f, 0.0f);
    i0 = min((int)src, n - 1);
    i1 = min(i0 + 1, n - 1);
    l1 = src - (float)i0;
    l0 = 1.0f - l1;
}

__global__ __launch_bounds__(256) void k_renoise_resize(const float* __restrict__ mask, int H, int W, float strength, float* __restrict__ out,
                                                        int h, int w, float sy, float sx) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= h * w) return;
    const int oy = idx / w, ox = idx - oy * w;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    bilinear_tap(oy, sy, H, y0, y1, ly0, ly1);
    bilinear_tap(ox, sx, W, x0, x1, lx0, lx1);
    const float* __restrict__ r0 = mask + (size_t)y0 * W;
    const float* __restrict__ r1 = mask + (size_t)y1 * W;
    const float v = ly0 * (lx0 * r0[x0] + lx1 * r0[x1]) + ly1 * (lx0 * r1[x0] + lx1 * r1[x1]);
    out[idx] = fminf(fmaxf((1.0f - v) * strength, 0.0f), 1.0f);
}
}  // namespace

extern "C" size_t mdtile_retouch_mask_ws_size(int H, int W, int kernel_size) {
    if (H <= 0 || W <= 0 || (long long)H * W >= (1ll << 31) || kernel_size < 1 || kernel_size > RT_KMAX) return 0;
    return (size_t)H * W * sizeof(uint2);
}

extern "C" int mdtile_retouch_mask(const uint8_t* d_img, int H, int W, int channels, int kernel_size, float* d_mask, void* d_ws,
                                   mdtile_stream_t stream) {
    MDT_CHECK_ARG(d_img && d_mask && d_ws, "mdtile_retouch_mask: null argument");
    MDT_CHECK_ARG(H > 0 && W > 0 && (long long)H * W < (1ll << 31), "mdtile_retouch_mask: bad image size %d x %d (H * W must be below 2^31)", H, W);
    MDT_CHECK_ARG(channels == 1 || channels == 3, "mdtile_retouch_mask: %d channels (1 = grey, 3 = RGB interleaved)", channels);
    MDT_CHECK_ARG(kernel_size >= 1 && kernel_size <= RT_KMAX, "mdtile_retouch_mask: kernel_size %d outside 1..%d", kernel_size, RT_KMAX);
    const int k = kernel_size;
    const int nseg = cdiv(W, RT_SEG_MAX);
    const int seg = cdiv(W, nseg);                    // <= RT_SEG_MAX; equal segments instead of a nearly empty last one
    const long long blocks_r = (long long)nseg * H;
    const int R = k < 32 ? 32 : (k > 256 ? 256 : k);  // rows per chunk: the k-row start-up costs at most two more reads per pixel
    const int colblocks = cdiv(W, RT_THREADS);
    const long long blocks_c = (long long)colblocks * cdiv(H, R);
    MDT_CHECK_ARG(blocks_r < (1ll << 31) && blocks_c < (1ll << 31), "mdtile_retouch_mask: %d x %d needs too many blocks", H, W);
    hipStream_t s = as_stream(stream);
    uint2* ws = (uint2*)d_ws;
    if (channels == 3)
        hipLaunchKernelGGL(k_retouch_rows<3>, dim3((unsigned)blocks_r), dim3(RT_THREADS), 0, s, d_img, W, k, seg, nseg, ws);
    else
        hipLaunchKernelGGL(k_retouch_rows<1>, dim3((unsigned)blocks_r), dim3(RT_THREADS), 0, s, d_img, W, k, seg, nseg, ws);
    MDT_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_retouch_cols, dim3((unsigned)blocks_c), dim3(RT_THREADS), 0, s, (const uint2*)ws, H, W, k, R, colblocks, d_mask);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_renoise_resize(const float* d_mask, int H, int W, float strength, float* d_out, int h, int w, mdtile_stream_t stream) {
    MDT_CHECK_ARG(d_mask && d_out, "mdtile_renoise_resize: null argument");
    MDT_CHECK_ARG(H > 0 && W > 0 && h > 0 && w > 0 && (long long)H * W < (1ll << 31) && (long long)h * w < (1ll << 31),
                  "mdtile_renoise_resize: bad sizes %d x %d -> %d x %d", H, W, h, w);
    const float sy = (float)H / (float)h, sx = (float)W / (float)w;
    hipLaunchKernelGGL(k_renoise_resize, dim3(cdiv((long long)h * w, 256)), dim3(256), 0, as_stream(stream), d_mask, H, W, strength, d_out, h, w,
                       sy, sx);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}
