// Free-form mask regions beside the rectangles.  A region keeps its rectangle and gains a coverage map [h, w] of bytes: it takes part
// in a canvas pixel only where that byte is non-zero (include/mdtile.h has the definitions).  Four entry points:
//   mdtile_mask_cover_u8        painted mask [Hm, Wm] -> coverage [H, W] on the latent canvas, its bounding box and count (two launches, no atomics)
//   mdtile_mask_region          coverage + rectangle -> the region's dense cover [h, w] and its chessboard-distance feather
//   mdtile_region_noise_masked  k_region_noise (maps.hip) with the coverage rule
//   mdtile_blend_mask_regions   the argument checks here, the kernel in blend.hip (k_blend<..., MASKED = true>, whose text has the arithmetic)
// The first three run once per region and job; integers decide every result but the feather's final (d / R)^2, which is mdtile_feather_mask's expression.
#include <climits>
#include <cmath>

#include "launchers.h"

using namespace mdt;

namespace {

// One thread per canvas cell: the byte sum of the cell's box of the mask, by the widest loads the box's rows allow (lane x + 1 reads the bytes right
// behind lane x's: a wave takes a contiguous run of each mask row).
__global__ __launch_bounds__(256) void k_mask_cover(const unsigned char* __restrict__ mask, int Wm, int Hm, int W, int H, unsigned char* __restrict__ cover) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W * H) return;
    const int y = idx / W, x = idx - y * W;
    const int r0 = (int)((long long)y * Hm / H), r1 = (int)((long long)(y + 1) * Hm / H);      // r1 <= Hm, r1 > r0 (Hm >= H)
    const int c0 = (int)((long long)x * Wm / W), c1 = (int)((long long)(x + 1) * Wm / W);      // c1 <= Wm, c1 > c0 (Wm >= W)
    const int bw = c1 - c0;
    const unsigned char* row = mask + (size_t)r0 * Wm + c0;
    unsigned s = 0u;
    for (int r = r0; r < r1; ++r, row += Wm) {
        if ((bw & 7) == 0 && ((uintptr_t)row & 7) == 0) {
            for (int c = 0; c < bw; c += 8) {
                const uint2 v = *reinterpret_cast<const uint2*>(row + c);
                s = __builtin_amdgcn_sad_u8(v.x, 0u, s);      // + the four bytes of v.x
                s = __builtin_amdgcn_sad_u8(v.y, 0u, s);
            }
        } else if ((bw & 3) == 0 && ((uintptr_t)row & 3) == 0) {
            for (int c = 0; c < bw; c += 4) s = __builtin_amdgcn_sad_u8(*reinterpret_cast<const unsigned*>(row + c), 0u, s);
        } else {
            for (int c = 0; c < bw; ++c) s += row[c];
        }
    }
    const unsigned n = (unsigned)(r1 - r0) * (unsigned)bw;      // <= 2^22 (host check): 2 * 255 * n stays below 2^32
    cover[idx] = (2u * s >= 255u * n) ? 1 : 0;
}

// ONE block reads the coverage (bytes 0 / 1, at most a few MB) and reduces it to the box and the count: min, max and integer sums do not depend on the
// order, so there is neither an atomic nor a buffer to clear.
__global__ __launch_bounds__(1024) void k_mask_box(const unsigned char* __restrict__ cover, int W, int H, int* __restrict__ box) {
    __shared__ int part[16][5];
    const int tid = threadIdx.x, n = W * H;
    int xmin = INT_MAX, ymin = INT_MAX, xmax = -1, ymax = -1, cnt = 0;
    if ((W & 15) == 0 && ((uintptr_t)cover & 15) == 0) {      // a 16-byte record lies inside one row
        const uint4* c16 = reinterpret_cast<const uint4*>(cover);
        for (int i = tid; i < n / 16; i += 1024) {
            const uint4 v = c16[i];
            if (!(v.x | v.y | v.z | v.w)) continue;
            const int y = (i * 16) / W, xb = i * 16 - y * W;
            const unsigned q[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (!q[k]) continue;
                const int lo = xb + 4 * k + ((__ffs(q[k]) - 1) >> 3), hi = xb + 4 * k + ((31 - __clz(q[k])) >> 3);
                xmin = min(xmin, lo); xmax = max(xmax, hi);
                cnt += __popc(q[k]);      // every byte is 0 or 1
            }
            ymin = min(ymin, y); ymax = max(ymax, y);
        }
    } else {
        for (int i = tid; i < n; i += 1024) {
            if (!cover[i]) continue;
            const int y = i / W, x = i - y * W;
            xmin = min(xmin, x); xmax = max(xmax, x); ymin = min(ymin, y); ymax = max(ymax, y);
            ++cnt;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        xmin = min(xmin, __shfl_xor(xmin, off, 64)); ymin = min(ymin, __shfl_xor(ymin, off, 64));
        xmax = max(xmax, __shfl_xor(xmax, off, 64)); ymax = max(ymax, __shfl_xor(ymax, off, 64));
        cnt += __shfl_xor(cnt, off, 64);
    }
    if ((tid & 63) == 0) {
        int* p = part[tid >> 6];
        p[0] = xmin; p[1] = ymin; p[2] = xmax; p[3] = ymax; p[4] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w) {
            xmin = min(xmin, part[w][0]); ymin = min(ymin, part[w][1]); xmax = max(xmax, part[w][2]); ymax = max(ymax, part[w][3]);
            cnt += part[w][4];
        }
        const bool any = cnt > 0;
        box[0] = any ? xmin : 0; box[1] = any ? ymin : 0; box[2] = any ? xmax + 1 : 0; box[3] = any ? ymax + 1 : 0; box[4] = cnt;
    }
}

// One thread per cell (i, j) of the rectangle.  Feather: rings of growing chessboard radius around a covered cell until one holds a cell that is not
// covered; the rings that would leave the rectangle are not walked (the rectangle's outside is at distance min(i + 1, j + 1, h - i, w - j)), nor those
// past R (d >= R gives 1.0 whatever d is).
__global__ __launch_bounds__(256) void k_mask_region(const unsigned char* __restrict__ cover, int W, int x0, int y0, int w, int h, int R,
                                                     unsigned char* __restrict__ rcover, float* __restrict__ feather) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= w * h) return;
    const int i = idx / w, j = idx - i * w;
    const unsigned char* c = cover + (size_t)(y0 + i) * W + x0 + j;      // c[di * W + dj]: the cell (i + di, j + dj)
    const bool cov = *c != 0;
    rcover[idx] = cov ? 1 : 0;
    if (!feather) return;
    float f = 0.0f;
    if (cov) {
        const int kb = min(min(i + 1, j + 1), min(h - i, w - j));      // to the nearest cell outside the rectangle
        const int lim = min(kb - 1, R);                                  // the rings 1 .. lim lie inside the rectangle
        int k = kb - 1 <= R ? kb : R + 1;                                // no hole within lim: the rectangle's edge, or "R or further"
        for (int r = 1; r <= lim; ++r) {
            bool hole = false;
            const ptrdiff_t up = -(ptrdiff_t)r * W, dn = (ptrdiff_t)r * W;
            for (int d = -r; d <= r && !hole; ++d) hole = c[up + d] == 0 || c[dn + d] == 0;
            for (int d = -r + 1; d < r && !hole; ++d) hole = c[(ptrdiff_t)d * W - r] == 0 || c[(ptrdiff_t)d * W + r] == 0;
            if (hole) { k = r; break; }
        }
        const int d = k - 1;
        f = 1.0f;
        if (d < R) {
            const double q = (double)d / (double)R;
            f = (float)(q * q);
        }
    }
    feather[idx] = f;
}

struct NoiseRegionsMasked {
    struct mdtile_mask_region r[MDTILE_MAX_REGIONS];   // .r.out = the region's own noise [1, C, h, w] fp32
    int n;
};

// k_region_noise (maps.hip) where a region counts only at the pixels it covers
__global__ __launch_bounds__(256) void k_region_noise_masked(float* __restrict__ noise, int C, int H, int W, const NoiseRegionsMasked R) {
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= H * W) return;
    const int plane = blockIdx.y, c = plane % C;     // plane = n*C + c; the region noise is shared by every sample n
    const int y = px / W, x = px - y * W;
    float bg = 0.0f, bgc = 0.0f, fg = 0.0f, fgc = 0.0f;
    for (int k = 0; k < R.n; ++k) {
        const mdtile_region& g = R.r[k].r;
        const int dx = x - g.x, dy = y - g.y;
        if (dx < 0 || dy < 0 || dx >= g.w || dy >= g.h) continue;
        const size_t off = (size_t)dy * g.w + dx;
        if (R.r[k].cover && R.r[k].cover[off] == 0) continue;
        const float v = reinterpret_cast<const float*>(g.out)[(size_t)c * g.h * g.w + off];
        if (g.mode == MDTILE_REGION_BG) { bg += v; bgc += 1.0f; }
        else { fg += v; fgc += 1.0f; }
    }
    const size_t o = (size_t)plane * H * W + px;
    float out = noise[o];
    if (bgc > 0.0f) out = bgc > 1.0f ? bg / bgc : bg;
    if (fgc > 0.0f) out = fgc > 1.0f ? fg / fgc : fg;
    noise[o] = out;
}

int rect_check(const char* fn, const char* what, int W, int H, int x, int y, int w, int h) {
    MDT_CHECK_ARG(x >= 0 && y >= 0 && w > 0 && h > 0 && w <= W && h <= H && x <= W - w && y <= H - h, "%s: %s (%d,%d,%d,%d) leaves the %dx%d canvas", fn, what, x,
                  y, w, h, W, H);
    return MDTILE_OK;
}

}  // namespace

extern "C" int mdtile_mask_cover_u8(const unsigned char* d_mask, int Wm, int Hm, int W, int H, unsigned char* d_cover, int* d_box, mdtile_stream_t stream) {
    const char* fn = "mdtile_mask_cover_u8";
    MDT_CHECK_ARG(d_mask && d_cover && d_box, "%s: null argument", fn);
    MDT_CHECK_ARG(W > 0 && H > 0 && (long long)W * H < 0x7fffffffLL, "%s: bad canvas %dx%d", fn, W, H);
    MDT_CHECK_ARG(Wm >= W && Hm >= H, "%s: the mask (%dx%d) is smaller than the latent canvas (%dx%d) on an axis: a cell would own no mask pixel", fn, Wm, Hm, W, H);
    MDT_CHECK_ARG((long long)(Wm / W + 1) * (Hm / H + 1) <= (1LL << 22), "%s: the mask (%dx%d) has more than 2^22 pixels per cell of the %dx%d canvas", fn, Wm, Hm,
                  W, H);
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(k_mask_cover, dim3(cdiv((long long)W * H, 256)), dim3(256), 0, s, d_mask, Wm, Hm, W, H, d_cover);
    hipLaunchKernelGGL(k_mask_box, dim3(1), dim3(1024), 0, s, d_cover, W, H, d_box);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_mask_region(const unsigned char* d_cover, int W, int H, int x, int y, int w, int h, double feather_ratio, unsigned char* d_rcover,
                                  float* d_feather, mdtile_stream_t stream) {
    const char* fn = "mdtile_mask_region";
    MDT_CHECK_ARG(d_cover && d_rcover, "%s: null argument", fn);
    MDT_CHECK_ARG(W > 0 && H > 0 && (long long)W * H < 0x7fffffffLL, "%s: bad canvas %dx%d", fn, W, H);
    if (int rc = rect_check(fn, "rect", W, H, x, y, w, h)) return rc;
    MDT_CHECK_ARG(feather_ratio >= 0.0 && feather_ratio <= 1.0, "%s: feather_ratio %g outside [0, 1]", fn, feather_ratio);      // NaN fails both
    const int half = (w / 2) < (h / 2) ? (w / 2) : (h / 2);
    const int radius = (int)((double)half * feather_ratio);      // as mdtile_feather_mask
    hipLaunchKernelGGL(k_mask_region, dim3(cdiv((long long)w * h, 256)), dim3(256), 0, as_stream(stream), d_cover, W, x, y, w, h, radius, d_rcover, d_feather);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_region_noise_masked(float* d_noise, int N, int C, int H, int W, const struct mdtile_mask_region* regions, int num_regions,
                                          mdtile_stream_t stream) {
    const char* fn = "mdtile_region_noise_masked";
    MDT_CHECK_ARG(d_noise, "%s: null noise", fn);
    MDT_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && N * C <= 65535 && (long long)W * H < 0x7fffffffLL, "%s: bad shape N=%d C=%d H=%d W=%d", fn, N, C, H, W);
    MDT_CHECK_ARG(num_regions >= 0 && num_regions <= MDTILE_MAX_REGIONS, "%s: %d regions (max %d)", fn, num_regions, MDTILE_MAX_REGIONS);
    MDT_CHECK_ARG(num_regions == 0 || regions, "%s: null regions", fn);
    if (num_regions == 0) return MDTILE_OK;
    NoiseRegionsMasked R;
    memset(&R, 0, sizeof(R));
    R.n = num_regions;
    for (int i = 0; i < num_regions; ++i) {
        const mdtile_region& g = regions[i].r;
        char what[32];
        snprintf(what, sizeof(what), "region %d rect", i);
        if (int rc = rect_check(fn, what, W, H, g.x, g.y, g.w, g.h)) return rc;
        MDT_CHECK_ARG(g.out, "%s: region %d has no noise", fn, i);
        MDT_CHECK_ARG(g.mode == MDTILE_REGION_BG || g.mode == MDTILE_REGION_FG, "%s: region %d has mode %d", fn, i, g.mode);
        R.r[i] = regions[i];
    }
    hipLaunchKernelGGL(k_region_noise_masked, dim3(cdiv((long long)H * W, 256), N * C), dim3(256), 0, as_stream(stream), d_noise, C, H, W, R);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_blend_mask_regions(const mdtile_plan* p, const mdtile_blend_args* a, const void* const* batch_out, int num_batches,
                                         const struct mdtile_mask_region* regions, int num_regions, mdtile_stream_t stream) {
    const char* fn = "mdtile_blend_mask_regions";
    MDT_CHECK_ARG(p && a, "%s: null plan / args", fn);
    MDT_CHECK_ARG(!plan_sparse(p), "%s: refused on a sparse plan: mask regions are not combined with tile skipping", fn);
    MDT_CHECK_ARG(!plan_wraps(p), "%s: refused on a %s plan: mask regions are not combined with wrap-around canvases", fn, wrap_kind(p));
    MDT_CHECK_ARG(a->flags == 0, "%s: takes no MDTILE_BLEND_* flags (flags=%d): no partial sums, tile range or packed buffer", fn, a->flags);
    MDT_CHECK_ARG(a->row_lo == 0 && a->row_hi == 0, "%s: takes no row band [%d,%d): mask regions are not combined with the multi-GPU path", fn, a->row_lo,
                  a->row_hi);
    MDT_CHECK_ARG(num_regions >= 0 && num_regions <= MDTILE_MAX_REGIONS, "%s: %d regions (max %d)", fn, num_regions, MDTILE_MAX_REGIONS);
    MDT_CHECK_ARG(num_regions == 0 || regions, "%s: null regions", fn);
    MDT_CHECK_ARG(a->N > 0 && a->C > 0 && a->N * a->C <= 65535, "%s: bad N=%d C=%d", fn, a->N, a->C);
    MDT_CHECK_ARG(a->method == MDTILE_METHOD_MD || a->method == MDTILE_METHOD_MOD, "%s: bad method %d", fn, a->method);
    MDT_CHECK_ARG(a->dtype >= 0 && a->dtype <= 2, "%s: bad dtype %d", fn, a->dtype);
    MDT_CHECK_ARG(a->d_x_out, "%s: null output", fn);
    MDT_CHECK_ARG(num_batches >= 0, "%s: bad num_batches %d", fn, num_batches);
    MDT_CHECK_ARG(num_batches == 0 || num_batches <= MDTILE_MAX_BATCHES, "%s: %d batches (max %d; the call has no packed form: raise the tile batch size)", fn,
                  num_batches, MDTILE_MAX_BATCHES);
    for (int k = 0; k < num_regions; ++k) {
        const mdtile_region& R = regions[k].r;
        char what[32];
        snprintf(what, sizeof(what), "region %d", k);
        if (int rc = rect_check(fn, what, p->w, p->h, R.x, R.y, R.w, R.h)) return rc;
        MDT_CHECK_ARG(R.out, "%s: region %d has no output", fn, k);
        MDT_CHECK_ARG(R.mode == MDTILE_REGION_BG || R.mode == MDTILE_REGION_FG, "%s: region %d bad mode %d", fn, k, R.mode);
        if (R.mode == MDTILE_REGION_FG || a->method == MDTILE_METHOD_MOD) MDT_CHECK_ARG(R.weight, "%s: region %d needs a weight / feather map", fn, k);
    }
    return blend_masked(p, a, batch_out, num_batches, regions, num_regions, as_stream(stream));      // blend.hip
}
