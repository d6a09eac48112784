// Region prompt control on a wrap-around canvas: rectangles that may cross x = W-1 -> 0 and y = H-1 -> 0 on the axes that wrap,
// on the grid at rest or displaced by this step's shift.  Four entry points, all of them new -- mdtile_blend, mdtile_blend_shift and the plain
// rect calls keep their kernels and their refusals:
//   mdtile_gather_rect_wrap, mdtile_weight_map_add_rect_wrap, mdtile_region_noise_wrap   the plain rect kernels (blend.hip, maps.hip) with the
//                                                                                        rectangle's coordinates taken on the circle (rel())
//   mdtile_blend_wrap_regions   k_walk_blend_regions below: the grid walk of k_walk_blend (wrap.hip) on the thread's quad of PLAN coordinates,
//                               then the region tail of blend_tail (blend.hip) at the quad's CANVAS coordinates.
//
// A region R covers canvas pixel (yc, xc) iff ry = rel(yc, R.y, H) < R.h and rx = rel(xc, R.x, W) < R.w; its value and weight are read at
// ry * R.w + rx.  The host has checked 0 <= R.x < W, 0 < R.w <= W (likewise y) and that a region passes an edge only on an axis that wraps, so on
// an axis that does not wrap rel() of a pixel in front of the region is >= extent - R.x >= R.w: not covered, with the same arithmetic.
//
// The weight sum is formed here, per pixel: the grid's map travels with the shift (plan coordinates), the background regions' map stays on the
// canvas, so their sum is another one every step and nothing made once per job holds it.  wsum = grid_w[yp, xp] + region_w[yc, xc], and for
// Mixture of Diffusers resc = 1.0f / wsum (IEEE division, as mdtile_reciprocal and k_lattice_blend).  Region weights arrive RAW and are
// multiplied by resc here -- mdtile_blend takes them premultiplied by its per-job reciprocal map.
//
// Order and arithmetic: grid tiles in ascending tile index from +0.0, then the background regions in list order, the MultiDiffusion division,
// then the foreground composite over the foreground regions in list order; fp32, -ffp-contract=off.  One thread writes each canvas pixel once;
// no LDS, no atomics.
#include "launchers.h"
#include "walk.h"

using namespace mdt;

namespace {

// ---- the three rect kernels ------------------------------------------------------------------------------------------------------------
// out[plane, i, j] = x_in[plane, (y0 + i) mod H, (x0 + j) mod W]: k_gather_rect on the circle.  y0 < H and i < h <= H: one subtraction.
template <typename T>
__global__ __launch_bounds__(256) void k_gather_rect_wrap(const T* __restrict__ x_in, T* __restrict__ out, int W, int H, int x0, int y0, int w, int h) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= w * h) return;
    const int i = idx / w, j = idx - i * w;
    const int plane = blockIdx.y;
    int y = y0 + i, x = x0 + j;
    if (y >= H) y -= H;
    if (x >= W) x -= W;
    out[(size_t)plane * w * h + idx] = x_in[((size_t)plane * H + y) * W + x];
}

// weights[(y0 + i) mod H, (x0 + j) mod W] += rect_w[i, j] (or scalar): k_weight_rect on the circle.  w <= W and h <= H: no canvas pixel is hit twice.
__global__ __launch_bounds__(256) void k_weight_rect_wrap(float* __restrict__ weights, int W, int H, int x0, int y0, int w, int h,
                                                          const float* __restrict__ rect_w, float scalar) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= w * h) return;
    const int i = idx / w, j = idx - i * w;
    int y = y0 + i, x = x0 + j;
    if (y >= H) y -= H;
    if (x >= W) x -= W;
    weights[(size_t)y * W + x] += rect_w ? rect_w[idx] : scalar;
}

struct NoiseRegionsWrap {
    mdtile_region r[MDTILE_MAX_REGIONS];   // .out = the region's own noise [1, C, h, w] fp32
    int n;
};

// k_region_noise (maps.hip) with coverage and offsets on the circle
__global__ __launch_bounds__(256) void k_region_noise_wrap(float* __restrict__ noise, int C, int H, int W, const NoiseRegionsWrap R) {
    const int px = blockIdx.x * 256 + threadIdx.x;
    if (px >= H * W) return;
    const int plane = blockIdx.y, c = plane % C;     // plane = n*C + c; the region noise is shared by every sample n
    const int y = px / W, x = px - y * W;
    float bg = 0.0f, bgc = 0.0f, fg = 0.0f, fgc = 0.0f;
    for (int k = 0; k < R.n; ++k) {
        const mdtile_region& g = R.r[k];
        const int dx = rel(x, g.x, W), dy = rel(y, g.y, H);
        if (dx >= g.w || dy >= g.h) continue;
        const float v = reinterpret_cast<const float*>(g.out)[((size_t)c * g.h + dy) * g.w + dx];
        if (g.mode == MDTILE_REGION_BG) { bg += v; bgc += 1.0f; }
        else { fg += v; fgc += 1.0f; }
    }
    const size_t o = (size_t)plane * H * W + px;
    float out = noise[o];
    if (bgc > 0.0f) out = bgc > 1.0f ? bg / bgc : bg;
    if (fgc > 0.0f) out = fgc > 1.0f ? fg / fgc : fg;
    noise[o] = out;
}

// ---- the blend ---------------------------------------------------------------------------------------------------------------------------
struct WrapRegionsParams {
    int W, H, tw, th, cols, rows, tile_bs, N, C;
    int num_batches;          // 0: no grid is drawn (grid_w null), only regions
    int num_regions, num_fg;
    int shift_x, shift_y;     // 0 <= shift_x < W, 0 <= shift_y < H; 0 on an axis that does not wrap
    const int *xs, *ys;
    const int4 *colquad, *rowinfo;
    const float* grid_w;      // [H, W] in PLAN coordinates
    const float* region_w;    // [H, W] in CANVAS coordinates
    const float* tile_w;
    void* out;
    mdtile_region regions[MDTILE_MAX_REGIONS];
    const void* batch[MDTILE_MAX_BATCHES];
};
static_assert(sizeof(WrapRegionsParams) <= 4096, "kernel argument block must stay under 4 KiB");

// One thread owns one quad of PLAN columns (y, x0 .. x0 + 3) for PP planes, as in k_walk_blend; the quad's canvas pixels are row
// yc = (y + shift_y) mod H, columns xc[j] = (x0 + shift_x + j) mod W -- consecutive in memory unless the seam cuts the displaced quad (`uncut`).
// Both weight maps are loaded, and for Mixture of Diffusers divided, in front of the walk; the walk is k_walk_blend's (vector loads where a
// tile row piece is whole and aligned, per-element loads where a tile edge or the seam cuts it); the region tail runs per element at xc[j], so
// a region that crosses a seam and a quad that the shift cut take the same path.
template <typename T, int METHOD, int PP>
__global__ __launch_bounds__(256) void k_walk_blend_regions(const WrapRegionsParams P) {
    using R4 = typename RawOf<T>::type;
    const int W4 = (P.W + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W4 * P.H) return;
    const int y = idx / W4, xq = idx - y * W4;
    const int x0 = xq << 2;
    const int p0 = blockIdx.y * PP;                        // the host guarantees N*C % PP == 0
    const int nvalid = P.W - x0 < 4 ? P.W - x0 : 4;
    const size_t tile_elems = (size_t)P.th * P.tw;

    int yc = y + P.shift_y;                                // y < H, shift_y < H: one subtraction
    if (yc >= P.H) yc -= P.H;
    int xd = x0 + P.shift_x;                               // x0 < W, shift_x < W: likewise
    if (xd >= P.W) xd -= P.W;
    const bool uncut = nvalid == 4 && xd + 3 < P.W;        // the four canvas columns are consecutive in memory
    int xc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) xc[j] = xd + j < P.W ? xd + j : xd + j - P.W;      // xd < W, j < 4: one subtraction

    // wsum = grid_w[yp, xp] + region_w[yc, xc]; Mixture of Diffusers: its reciprocal.  Pixels past the canvas (j >= nvalid) keep 0 and are never used.
    float wsum[4] = {0.f, 0.f, 0.f, 0.f}, resc[4] = {0.f, 0.f, 0.f, 0.f};
    {
        float gw[4] = {0.f, 0.f, 0.f, 0.f}, rw[4] = {0.f, 0.f, 0.f, 0.f};
        const float* rrow = P.region_w + (size_t)yc * P.W;
        if (uncut) {
            load4<float>(rrow + xd, rw);
            if (P.grid_w) load4<float>(P.grid_w + (size_t)y * P.W + x0, gw);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j >= nvalid) continue;
                rw[j] = rrow[xc[j]];
                if (P.grid_w) gw[j] = P.grid_w[(size_t)y * P.W + x0 + j];
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= nvalid) continue;
            wsum[j] = gw[j] + rw[j];
            if (METHOD == MDTILE_METHOD_MOD) resc[j] = 1.0f / wsum[j];      // inf where nothing covers the pixel: never multiplied there
        }
    }

    float acc[PP][4];
#pragma unroll
    for (int pp = 0; pp < PP; ++pp)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[pp][j] = 0.f;

    if (P.num_batches > 0) {
        const CyclicRun run(P.colquad[xq].x, P.cols), rrun(P.rowinfo[y].x, P.rows);
        for (int kr = 0; kr < rrun.count; ++kr) {          // ascending tile index: rows outer, columns inner
            const int r = rrun.at(kr);
            const int ty = rel(y, P.ys[r], P.H);           // < th: rowinfo holds exactly the rows that cover y
            const size_t roff = (size_t)ty * P.tw;         // the tile row inside a [th, tw] plane (and inside the tile-weight map)
            for (int k = 0; k < run.count; ++k) {
                const int c = run.at(k);
                const int t = r * P.cols + c;
                const int b = t / P.tile_bs, i = t - b * P.tile_bs;
                const int tx = rel(x0, P.xs[c], P.W);
                const T* row = reinterpret_cast<const T*>(P.batch[b]) + ((size_t)i * P.N * P.C + p0) * tile_elems + roff;
                const bool whole = nvalid == 4 && tx + 3 < P.tw;
                if (whole && (reinterpret_cast<uintptr_t>(row + tx) & (4 * sizeof(T) - 1)) == 0 && (tile_elems & 3) == 0) {
                    float wg[4] = {1.f, 1.f, 1.f, 1.f};
                    if (METHOD == MDTILE_METHOD_MOD) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) wg[j] = P.tile_w[roff + tx + j] * resc[j];
                    }
#pragma unroll
                    for (int pp = 0; pp < PP; ++pp) {
                        float v[4];
                        load4_aligned<T>(row + (size_t)pp * tile_elems + tx, v);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (METHOD == MDTILE_METHOD_MOD) acc[pp][j] += v[j] * wg[j];
                            else acc[pp][j] += v[j];
                        }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        int txj = tx + j;                  // tx < W, j < 4: one subtraction
                        if (txj >= P.W) txj -= P.W;
                        if (j >= nvalid || txj >= P.tw) continue;
                        float wgt = 1.0f;
                        if (METHOD == MDTILE_METHOD_MOD) wgt = P.tile_w[roff + txj] * resc[j];
#pragma unroll
                        for (int pp = 0; pp < PP; ++pp) {
                            const float v = to_f32<T>(row[(size_t)pp * tile_elems + txj]);
                            if (METHOD == MDTILE_METHOD_MOD) acc[pp][j] += v * wgt;
                            else acc[pp][j] += v;
                        }
                    }
                }
            }
        }
    }

    // background regions, in list order, after every grid tile; Mixture of Diffusers: the region's RAW weight times this pixel's reciprocal
    for (int k = 0; k < P.num_regions; ++k) {
        const mdtile_region& R = P.regions[k];
        if (R.mode != MDTILE_REGION_BG) continue;
        const int ry = rel(yc, R.y, P.H);
        if (ry >= R.h) continue;
        const size_t rplane = (size_t)R.h * R.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= nvalid) continue;
            const int rx = rel(xc[j], R.x, P.W);
            if (rx >= R.w) continue;
            const size_t off = (size_t)ry * R.w + rx;
            const T* src = reinterpret_cast<const T*>(R.out) + (size_t)p0 * rplane + off;
            float wgt = 1.0f;
            if (METHOD == MDTILE_METHOD_MOD) wgt = R.weight[off] * resc[j];
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) {
                const float v = to_f32<T>(src[(size_t)pp * rplane]);
                if (METHOD == MDTILE_METHOD_MOD) acc[pp][j] += v * wgt;
                else acc[pp][j] += v;
            }
        }
    }

    // MD normalisation: x = wsum > 1 ? buf / wsum : buf
    if (METHOD == MDTILE_METHOD_MD) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= nvalid || !(wsum[j] > 1.0f)) continue;
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) acc[pp][j] = acc[pp][j] / wsum[j];
        }
    }

    // foreground feather composite: blend_tail's (blend.hip), the coverage on the circle
    if (P.num_fg > 0) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j >= nvalid) continue;
            float fbuf[PP], fmask = 0.0f, fcnt = 0.0f;
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) fbuf[pp] = 0.0f;
            for (int k = 0; k < P.num_regions; ++k) {
                const mdtile_region& R = P.regions[k];
                if (R.mode != MDTILE_REGION_FG) continue;
                const int ry = rel(yc, R.y, P.H), rx = rel(xc[j], R.x, P.W);
                if (ry >= R.h || rx >= R.w) continue;
                const size_t rplane = (size_t)R.h * R.w, off = (size_t)ry * R.w + rx;
                const T* src = reinterpret_cast<const T*>(R.out) + (size_t)p0 * rplane + off;
#pragma unroll
                for (int pp = 0; pp < PP; ++pp) fbuf[pp] += to_f32<T>(src[(size_t)pp * rplane]);
                fmask += R.weight[off];
                fcnt += 1.0f;
            }
            if (fcnt > 0.0f) {
                if (fcnt > 1.0f) fmask = fmask / fcnt;
#pragma unroll
                for (int pp = 0; pp < PP; ++pp) {
                    float fb = fbuf[pp];
                    if (fcnt > 1.0f) fb = fb / fcnt;
                    acc[pp][j] = acc[pp][j] * (1.0f - fmask) + fb * fmask;
                }
            }
        }
    }

    // the store of k_walk_blend's SHIFT form: one element-aligned group of four when the canvas quad is not cut, per element when it is
#pragma unroll
    for (int pp = 0; pp < PP; ++pp) {
        R4* drow = reinterpret_cast<R4*>(P.out) + ((size_t)(p0 + pp) * P.H + yc) * P.W;
        if (uncut) {
            raw4_u<R4> o;
#pragma unroll
            for (int j = 0; j < 4; ++j) o.v[j] = raw_bits<T>(acc[pp][j]);
            *reinterpret_cast<raw4_u<R4>*>(drow + xd) = o;
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nvalid) drow[xc[j]] = raw_bits<T>(acc[pp][j]);
        }
    }
}

// planes per thread: sized as wrap.hip sizes k_walk_blend (4 while that leaves >= ~128k threads and divides N*C); whether another size pays
// with the region tail behind the walk is not measured
int planes_per_thread(const WrapRegionsParams& P) {
    const int planes = P.N * P.C;
    const long long work = (long long)P.H * ((P.W + 3) / 4) * planes;
    if (planes % 4 == 0 && work / 4 >= 131072) return 4;
    return planes % 2 == 0 && work / 2 >= 131072 ? 2 : 1;
}

using WrapRegionsKernel = void (*)(const WrapRegionsParams);
template <typename T, int PP>
WrapRegionsKernel wrap_regions_kernel(int method) {
    return method == MDTILE_METHOD_MD ? k_walk_blend_regions<T, MDTILE_METHOD_MD, PP> : k_walk_blend_regions<T, MDTILE_METHOD_MOD, PP>;
}

template <typename T>
void launch_wrap_regions(const WrapRegionsParams& P, int method, hipStream_t s) {
    const int pp = planes_per_thread(P);
    const WrapRegionsKernel k = pp == 4 ? wrap_regions_kernel<T, 4>(method) : pp == 2 ? wrap_regions_kernel<T, 2>(method) : wrap_regions_kernel<T, 1>(method);
    hipLaunchKernelGGL(k, dim3(cdiv((long long)P.H * ((P.W + 3) / 4), 256), (P.N * P.C) / pp), dim3(256), 0, s, P);
}

// a rectangle on a canvas that is closed on the axes whose flag is set: origin on the canvas, no larger than it, past an edge only where it wraps
int rect_wrap_check(const char* fn, const char* what, int W, int H, int x, int y, int w, int h, int wrap_x, int wrap_y) {
    MDT_CHECK_ARG(W > 0 && H > 0, "%s: bad canvas %dx%d", fn, W, H);
    MDT_CHECK_ARG(w > 0 && h > 0 && w <= W && h <= H && x >= 0 && x < W && y >= 0 && y < H,
                  "%s: %s (%d,%d,%d,%d) does not fit the %dx%d canvas: 0 <= x < W, 0 <= y < H, 0 < w <= W, 0 < h <= H", fn, what, x, y, w, h, W, H);
    MDT_CHECK_ARG(wrap_x || x + w <= W, "%s: %s (%d,%d,%d,%d) passes the right edge of the %dx%d canvas and the x axis does not wrap", fn, what, x, y, w,
                  h, W, H);
    MDT_CHECK_ARG(wrap_y || y + h <= H, "%s: %s (%d,%d,%d,%d) passes the bottom edge of the %dx%d canvas and the y axis does not wrap", fn, what, x, y, w,
                  h, W, H);
    return MDTILE_OK;
}

}  // namespace

extern "C" int mdtile_gather_rect_wrap(int dtype, int N, int C, int W, int H, const void* d_x_in, int x, int y, int w, int h, int wrap_x, int wrap_y,
                                       void* d_out, mdtile_stream_t stream) {
    const char* fn = "mdtile_gather_rect_wrap";
    MDT_CHECK_ARG(d_x_in && d_out, "%s: null argument", fn);
    MDT_CHECK_ARG(N > 0 && C > 0 && N * C <= 65535, "%s: bad N=%d C=%d", fn, N, C);
    MDT_CHECK_ARG(dtype >= 0 && dtype <= 2, "%s: bad dtype %d", fn, dtype);
    if (int rc = rect_wrap_check(fn, "rect", W, H, x, y, w, h, wrap_x, wrap_y)) return rc;
    dim3 grid(cdiv((long long)w * h, 256), N * C), block(256);
    hipStream_t s = as_stream(stream);
    with_dtype(dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        hipLaunchKernelGGL(k_gather_rect_wrap<T>, grid, block, 0, s, (const T*)d_x_in, (T*)d_out, W, H, x, y, w, h);
    });
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_weight_map_add_rect_wrap(float* d_weights, int W, int H, int x, int y, int w, int h, const float* d_rect_w, float scalar, int wrap_x,
                                               int wrap_y, mdtile_stream_t stream) {
    const char* fn = "mdtile_weight_map_add_rect_wrap";
    MDT_CHECK_ARG(d_weights, "%s: null weight map", fn);
    if (int rc = rect_wrap_check(fn, "rect", W, H, x, y, w, h, wrap_x, wrap_y)) return rc;
    hipLaunchKernelGGL(k_weight_rect_wrap, dim3(cdiv((long long)w * h, 256)), dim3(256), 0, as_stream(stream), d_weights, W, H, x, y, w, h, d_rect_w, scalar);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_region_noise_wrap(float* d_noise, int N, int C, int H, int W, const mdtile_region* regions, int num_regions, int wrap_x, int wrap_y,
                                        mdtile_stream_t stream) {
    const char* fn = "mdtile_region_noise_wrap";
    MDT_CHECK_ARG(d_noise, "%s: null noise", fn);
    MDT_CHECK_ARG(N > 0 && C > 0 && H > 0 && W > 0 && N * C <= 65535, "%s: bad shape N=%d C=%d H=%d W=%d", fn, N, C, H, W);
    MDT_CHECK_ARG(num_regions >= 0 && num_regions <= MDTILE_MAX_REGIONS, "%s: %d regions (max %d)", fn, num_regions, MDTILE_MAX_REGIONS);
    MDT_CHECK_ARG(num_regions == 0 || regions, "%s: null regions", fn);
    if (num_regions == 0) return MDTILE_OK;
    NoiseRegionsWrap R;
    memset(&R, 0, sizeof(R));
    R.n = num_regions;
    for (int i = 0; i < num_regions; ++i) {
        const mdtile_region& g = regions[i];
        char what[32];
        snprintf(what, sizeof(what), "region %d rect", i);
        if (int rc = rect_wrap_check(fn, what, W, H, g.x, g.y, g.w, g.h, wrap_x, wrap_y)) return rc;
        MDT_CHECK_ARG(g.out, "%s: region %d has no noise", fn, i);
        MDT_CHECK_ARG(g.mode == MDTILE_REGION_BG || g.mode == MDTILE_REGION_FG, "%s: region %d has mode %d", fn, i, g.mode);
        R.r[i] = g;
    }
    hipLaunchKernelGGL(k_region_noise_wrap, dim3(cdiv((long long)H * W, 256), N * C), dim3(256), 0, as_stream(stream), d_noise, C, H, W, R);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_blend_wrap_regions(const mdtile_plan* p, const mdtile_blend_args* a, const void* const* batch_out, int num_batches,
                                         const mdtile_wrap_regions* wr, mdtile_stream_t stream) {
    const char* fn = "mdtile_blend_wrap_regions";
    MDT_CHECK_ARG(p && a && wr, "%s: null plan / args / regions block", fn);
    if (int rc = shift_check(fn, p, wr->sx, wr->sy)) return rc;      // a sparse plan, a plain plan, the shift's range and its axes
    const char* kind = wrap_kind(p);
    MDT_CHECK_ARG(wr->num_regions >= 0 && wr->num_regions <= MDTILE_MAX_REGIONS, "%s: %d regions (max %d)", fn, wr->num_regions, MDTILE_MAX_REGIONS);
    MDT_CHECK_ARG(wr->num_regions == 0 || wr->regions, "%s: null regions", fn);
    MDT_CHECK_ARG(a->flags == 0, "%s: takes no MDTILE_BLEND_* flags (flags=%d): no partial sums, tile range or packed buffer on a %s plan", fn, a->flags, kind);
    MDT_CHECK_ARG(a->row_lo == 0 && a->row_hi == 0, "%s: takes no row band [%d,%d): wrap-around is not combined with the multi-GPU path", fn, a->row_lo,
                  a->row_hi);
    MDT_CHECK_ARG(!a->d_weights && !a->d_rescale, "%s: d_weights and d_rescale must be NULL: the kernel forms the weight sum and its reciprocal itself", fn);
    MDT_CHECK_ARG(a->N > 0 && a->C > 0 && a->N * a->C <= 65535, "%s: bad N=%d C=%d", fn, a->N, a->C);
    MDT_CHECK_ARG(a->method == MDTILE_METHOD_MD || a->method == MDTILE_METHOD_MOD, "%s: bad method %d", fn, a->method);
    MDT_CHECK_ARG(a->dtype >= 0 && a->dtype <= 2, "%s: bad dtype %d", fn, a->dtype);
    MDT_CHECK_ARG(a->d_x_out, "%s: null output", fn);
    MDT_CHECK_ARG(wr->d_region_w, "%s: null d_region_w: the background regions' weight sum is required (zeros when there is none)", fn);
    MDT_CHECK_ARG(num_batches == 0 || num_batches == p->num_batches, "%s: %d batches given, the %s plan has %d (0 = no grid is drawn)", fn, num_batches, kind,
                  p->num_batches);
    if (num_batches > MDTILE_MAX_BATCHES) {
        set_error("%s: %d batches > MDTILE_MAX_BATCHES=%d (a %s plan has no packed form: raise the tile batch size)", fn, num_batches, MDTILE_MAX_BATCHES, kind);
        return MDTILE_E_LIMIT;
    }
    MDT_CHECK_ARG((num_batches == 0) == (wr->d_grid_w == nullptr), "%s: d_grid_w must be NULL iff num_batches == 0 (%d batches given)", fn, num_batches);
    if (num_batches > 0) {
        MDT_CHECK_ARG(batch_out, "%s: null batch_out", fn);
        MDT_CHECK_ARG(a->method != MDTILE_METHOD_MOD || a->d_tile_w, "%s: Mixture of Diffusers needs d_tile_w", fn);
        for (int b = 0; b < num_batches; ++b) MDT_CHECK_ARG(batch_out[b], "%s: null batch pointer %d", fn, b);
    }
    int num_fg = 0;
    for (int k = 0; k < wr->num_regions; ++k) {
        const mdtile_region& R = wr->regions[k];
        char what[32];
        snprintf(what, sizeof(what), "region %d", k);
        if (int rc = rect_wrap_check(fn, what, p->w, p->h, R.x, R.y, R.w, R.h, p->wrap_x, p->wrap_y)) return rc;
        MDT_CHECK_ARG(R.out, "%s: region %d has no output", fn, k);
        MDT_CHECK_ARG(R.mode == MDTILE_REGION_BG || R.mode == MDTILE_REGION_FG, "%s: region %d bad mode %d", fn, k, R.mode);
        if (R.mode == MDTILE_REGION_FG || a->method == MDTILE_METHOD_MOD) MDT_CHECK_ARG(R.weight, "%s: region %d needs a weight / feather map", fn, k);
        num_fg += R.mode == MDTILE_REGION_FG;
    }
    if (int rc = plan_upload(p)) return rc;
    WrapRegionsParams P;
    memset(&P, 0, sizeof(P));
    P.W = p->w; P.H = p->h; P.tw = p->tw; P.th = p->th; P.cols = p->cols; P.rows = p->rows; P.tile_bs = p->tile_bs; P.N = a->N; P.C = a->C;
    P.num_batches = num_batches; P.num_regions = wr->num_regions; P.num_fg = num_fg; P.shift_x = wr->sx; P.shift_y = wr->sy;
    P.xs = p->d_xs; P.ys = p->d_ys; P.colquad = p->d_colquad; P.rowinfo = p->d_rowinfo;
    P.grid_w = wr->d_grid_w; P.region_w = wr->d_region_w; P.tile_w = a->d_tile_w; P.out = a->d_x_out;
    for (int k = 0; k < wr->num_regions; ++k) P.regions[k] = wr->regions[k];
    for (int b = 0; b < num_batches; ++b) P.batch[b] = batch_out[b];
    with_dtype(a->dtype, [&](auto* tag) { launch_wrap_regions<std::remove_pointer_t<decltype(tag)>>(P, a->method, as_stream(stream)); });
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}
