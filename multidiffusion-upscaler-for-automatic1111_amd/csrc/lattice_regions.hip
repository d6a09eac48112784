// Region prompt control under the per-step grid jitter: mdtile_blend_lattice_regions.  The grid is the step's lattice
// (lattice.h: a handful of integers, no table, no map); the regions are ordinary rectangles that stay where the user put them on the canvas.
//
// The weight sum of a pixel is another one every step -- the set of covering tiles moves, the regions do not -- so it is formed here, per pixel:
//     gw   = lat_wsum(...)                         exactly what mdtile_lattice_weight_map writes and k_lattice_blend divides by
//     wsum = region_w ? gw + region_w[y, x] : gw   region_w: the background regions' weight sum on the canvas, made once per job
//     Mixture of Diffusers: resc = 1.0f / wsum     IEEE division; the lattice covers every pixel, so wsum > 0
// Region weights arrive RAW and are multiplied by resc here -- mdtile_blend takes them premultiplied by its per-job reciprocal map, which cannot
// hold when the reciprocal changes every step (the same convention, for the same reason, as wrap_regions.hip).
//
// Order and arithmetic: grid tiles in ascending tile index from +0.0, each read at its PUSHED-IN coordinates where its LATTICE box lies
// (k_lattice_blend's walk), then the background regions in list order, the MultiDiffusion division, then the foreground composite over the
// foreground regions in list order (blend_tail's arithmetic, blend.hip); fp32 on scalars, -ffp-contract=off.  One thread writes each canvas
// pixel once; no LDS, no atomics.
#include "launchers.h"
#include "lattice.h"

using namespace mdt;

namespace {

// most blocks along grid.y, as in lattice.hip (which keeps its own definition: tests/test_gpu_lattice.py reads the number from that file's text);
// the kernel walks the planes (n * C + c) from blockIdx.y in steps of gridDim.y, so N * C may pass it
constexpr int kPlaneBlocks = 64;

struct LatticeRegionsParams : LatticeBlendParams {
    int num_regions, num_fg;
    const float* region_w;    // [H, W] on the canvas; null iff the list holds no background region
    mdtile_region regions[MDTILE_MAX_REGIONS];
};
static_assert(sizeof(LatticeRegionsParams) <= 4096, "kernel argument block must stay under 4 KiB");

// k_lattice_blend (lattice.hip) with a region tail behind the tile walk.  One thread owns one aligned quad (4 consecutive canvas columns of one
// row) for PP planes at a time and walks the planes from blockIdx.y * PP in steps of gridDim.y * PP.  The four grid weight sums come from
// lat_wsum with k_lattice_blend's candidates in its order; region_w is added and, for Mixture of Diffusers, the reciprocal taken, once, in
// front of the plane walk.  Per candidate tile the quad is either whole inside the tile's lattice box -- one element-aligned load4 per plane --
// or cut by a lattice border / the canvas edge: per-element loads of the covered pixels only, so the part of a pushed-in tile outside its lattice
// box is never read.  The region tail runs per element at plain canvas coordinates.
template <typename T, int METHOD, int PP>
__global__ __launch_bounds__(256) void k_lattice_blend_regions(const LatticeRegionsParams P) {
    using R4 = typename RawOf<T>::type;
    const int W = P.ax.extent, H = P.ay.extent, tw = P.ax.tile, th = P.ay.tile;
    const int W4 = (W + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W4 * H) return;
    const int y = idx / W4, x0 = (idx - y * W4) << 2;
    const int nvalid = W - x0 < 4 ? W - x0 : 4;
    const int planes = P.N * P.C;                              // the host guarantees planes % PP == 0
    const size_t tile_elems = (size_t)th * tw;

    const Cover rows = lat_cover(P.ay, y, y), cand = lat_cover(P.ax, x0, x0 + nvalid - 1);
    // pixels past the canvas (j >= nvalid) keep 0 and are never used
    float wsum[4] = {0.f, 0.f, 0.f, 0.f}, resc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= nvalid) continue;
        const float gw = lat_wsum<METHOD == MDTILE_METHOD_MOD>(P, y, x0 + j, rows, cand, P.tile_w);
        wsum[j] = P.region_w ? gw + P.region_w[(size_t)y * W + x0 + j] : gw;
        if (METHOD == MDTILE_METHOD_MOD) resc[j] = 1.0f / wsum[j];      // IEEE division, as mdtile_reciprocal
    }

    for (int p0 = blockIdx.y * PP; p0 < planes; p0 += gridDim.y * PP) {
        float acc[PP][4];
#pragma unroll
        for (int pp = 0; pp < PP; ++pp)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[pp][j] = 0.f;

        for (int r = rows.lo; r <= rows.hi; ++r) {             // ascending tile index: rows outer, columns inner
            const int wy = y - lat_origin(P.ay, r);            // row inside the lattice box (and inside the tile-weight map)
            const int ty = y - lat_pushed(P.ay, r);            // row inside the pushed-in box: where the tile's value lies
            for (int c = cand.lo; c <= cand.hi; ++c) {
                const int d0 = x0 - lat_origin(P.ax, c);       // lattice-relative column of the quad's first pixel
                const int tx = x0 - lat_pushed(P.ax, c);       // pushed-in-relative column of it
                const int t = r * P.cols + c;
                const int b = t / P.tile_bs, i = t - b * P.tile_bs;
                const T* row = reinterpret_cast<const T*>(P.batch[b]) + ((size_t)i * planes + p0) * tile_elems + (size_t)ty * tw;
                if (nvalid == 4 && d0 >= 0 && d0 + 3 < tw) {   // whole inside the lattice box: then 0 <= tx and tx + 3 < tw
                    float wg[4] = {1.f, 1.f, 1.f, 1.f};
                    if (METHOD == MDTILE_METHOD_MOD) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) wg[j] = P.tile_w[wy * tw + d0 + j] * resc[j];
                    }
#pragma unroll
                    for (int pp = 0; pp < PP; ++pp) {
                        float v[4];
                        load4<T>(row + (size_t)pp * tile_elems + tx, v);
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            if (METHOD == MDTILE_METHOD_MOD) acc[pp][j] += v[j] * wg[j];
                            else acc[pp][j] += v[j];
                        }
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int dj = d0 + j;
                        if (j >= nvalid || dj < 0 || dj >= tw) continue;       // outside the lattice box: the tile does not contribute
                        float wgt = 1.0f;
                        if (METHOD == MDTILE_METHOD_MOD) wgt = P.tile_w[wy * tw + dj] * resc[j];
#pragma unroll
                        for (int pp = 0; pp < PP; ++pp) {
                            const float v = to_f32<T>(row[(size_t)pp * tile_elems + tx + j]);
                            if (METHOD == MDTILE_METHOD_MOD) acc[pp][j] += v * wgt;
                            else acc[pp][j] += v;
                        }
                    }
                }
            }
        }

        // background regions, in list order, after every grid tile; Mixture of Diffusers: the region's RAW weight times this pixel's reciprocal
        for (int k = 0; k < P.num_regions; ++k) {
            const mdtile_region& R = P.regions[k];
            if (R.mode != MDTILE_REGION_BG) continue;
            const int ry = y - R.y;
            if (ry < 0 || ry >= R.h) continue;
            const size_t rplane = (size_t)R.h * R.w;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int rx = x0 + j - R.x;
                if (j >= nvalid || rx < 0 || rx >= R.w) continue;
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
                if (wsum[j] > 1.0f) {
#pragma unroll
                    for (int pp = 0; pp < PP; ++pp) acc[pp][j] = acc[pp][j] / wsum[j];
                }
            }
        }

        // foreground feather composite: blend_tail's (blend.hip)
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
                    const int ry = y - R.y, rx = x0 + j - R.x;
                    if (ry < 0 || ry >= R.h || rx < 0 || rx >= R.w) continue;
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

        // k_lattice_blend's store: one element-aligned group of four, or the row end's elements
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) {
            R4* dst = reinterpret_cast<R4*>(P.out) + ((size_t)(p0 + pp) * H + y) * W + x0;
            if (nvalid == 4) {
                raw4_u<R4> o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o.v[j] = raw_bits<T>(acc[pp][j]);
                *reinterpret_cast<raw4_u<R4>*>(dst) = o;
            } else {
                for (int j = 0; j < nvalid; ++j) dst[j] = raw_bits<T>(acc[pp][j]);
            }
        }
    }
}

using LatticeRegionsKernel = void (*)(const LatticeRegionsParams);
template <typename T, int PP>
LatticeRegionsKernel lattice_regions_kernel(int method) {
    return method == MDTILE_METHOD_MD ? k_lattice_blend_regions<T, MDTILE_METHOD_MD, PP> : k_lattice_blend_regions<T, MDTILE_METHOD_MOD, PP>;
}

// PP as lattice.hip sizes k_lattice_blend; whether another size pays with the region tail behind the walk is not measured
template <typename T>
void launch_lattice_regions(const LatticeRegionsParams& P, int method, hipStream_t s) {
    const int W = P.ax.extent, H = P.ay.extent, planes = P.N * P.C;
    const int pp = planes_per_thread(W, H, planes);
    const LatticeRegionsKernel k =
        pp == 4 ? lattice_regions_kernel<T, 4>(method) : pp == 2 ? lattice_regions_kernel<T, 2>(method) : lattice_regions_kernel<T, 1>(method);
    const int gy = planes / pp < kPlaneBlocks ? planes / pp : kPlaneBlocks;
    hipLaunchKernelGGL(k, dim3(cdiv((long long)H * ((W + 3) / 4), 256), gy), dim3(256), 0, s, P);
}

}  // namespace

extern "C" int mdtile_blend_lattice_regions(const mdtile_lattice* lat, const mdtile_blend_args* a, const void* const* batch_out, int num_batches,
                                            const mdtile_lattice_regions* r, mdtile_stream_t stream) {
    const char* fn = "mdtile_blend_lattice_regions";
    if (int rc = lattice_check(fn, lat)) return rc;
    MDT_CHECK_ARG(a && batch_out, "%s: null argument", fn);
    MDT_CHECK_ARG(r, "%s: null regions block (mdtile_blend_lattice is the call without regions)", fn);
    MDT_CHECK_ARG(a->flags == 0, "%s: the lattice takes no MDTILE_BLEND_* flags (flags=%d): no partial sums, tile range or packed buffer", fn, a->flags);
    MDT_CHECK_ARG(a->row_lo == 0 && a->row_hi == 0, "%s: the lattice takes no row band [%d,%d): it is not combined with the multi-GPU path", fn, a->row_lo,
                  a->row_hi);
    MDT_CHECK_ARG(!a->d_weights && !a->d_rescale, "%s: d_weights and d_rescale must be NULL: the kernel forms the weight sum of the step's grid itself", fn);
    MDT_CHECK_ARG(a->N > 0 && a->C > 0 && a->N * a->C <= 65535, "%s: bad N=%d C=%d", fn, a->N, a->C);
    MDT_CHECK_ARG(a->method == MDTILE_METHOD_MD || a->method == MDTILE_METHOD_MOD, "%s: bad method %d", fn, a->method);
    MDT_CHECK_ARG(a->dtype >= 0 && a->dtype <= 2, "%s: bad dtype %d", fn, a->dtype);
    MDT_CHECK_ARG(a->d_x_out, "%s: null output", fn);
    MDT_CHECK_ARG(a->method != MDTILE_METHOD_MOD || a->d_tile_w, "%s: Mixture of Diffusers needs d_tile_w", fn);
    if (int rc = batches_check(fn, lat, num_batches)) return rc;
    for (int b = 0; b < num_batches; ++b) MDT_CHECK_ARG(batch_out[b], "%s: null batch pointer %d", fn, b);
    MDT_CHECK_ARG(r->num_regions >= 0 && r->num_regions <= MDTILE_MAX_REGIONS, "%s: %d regions (max %d)", fn, r->num_regions, MDTILE_MAX_REGIONS);
    MDT_CHECK_ARG(r->num_regions == 0 || r->regions, "%s: null regions", fn);
    int num_fg = 0, num_bg = 0;
    for (int k = 0; k < r->num_regions; ++k) {
        const mdtile_region& R = r->regions[k];
        // the kernel reads R.out / R.weight at (y - R.y) * R.w + (x - R.x) for the canvas pixels inside the rectangle: it must lie on the canvas
        MDT_CHECK_ARG(R.w >= 1 && R.h >= 1 && R.x >= 0 && R.y >= 0 && R.w <= lat->w - R.x && R.h <= lat->h - R.y,
                      "%s: region %d (%d,%d,%d,%d) does not lie on the %dx%d canvas: w >= 1, h >= 1, x >= 0, y >= 0, x + w <= W, y + h <= H", fn, k, R.x, R.y,
                      R.w, R.h, lat->w, lat->h);
        MDT_CHECK_ARG(R.mode == MDTILE_REGION_BG || R.mode == MDTILE_REGION_FG, "%s: region %d bad mode %d", fn, k, R.mode);
        MDT_CHECK_ARG(R.out, "%s: region %d has no output", fn, k);
        if (R.mode == MDTILE_REGION_FG) MDT_CHECK_ARG(R.weight, "%s: region %d (foreground) needs its feather mask", fn, k);
        else if (a->method == MDTILE_METHOD_MOD) MDT_CHECK_ARG(R.weight, "%s: region %d (background, Mixture of Diffusers) needs its raw Gaussian weight", fn, k);
        num_fg += R.mode == MDTILE_REGION_FG;
        num_bg += R.mode == MDTILE_REGION_BG;
    }
    MDT_CHECK_ARG(num_bg == 0 || r->d_region_w, "%s: null d_region_w with %d background region(s): their weight sum on the canvas is required", fn, num_bg);
    LatticeRegionsParams P;
    memset(&P, 0, sizeof(P));
    fill_params(P, lat, a->N, a->C);
    P.tile_w = a->method == MDTILE_METHOD_MOD ? a->d_tile_w : nullptr;
    P.out = a->d_x_out;
    for (int b = 0; b < num_batches; ++b) P.batch[b] = batch_out[b];
    P.num_regions = r->num_regions; P.num_fg = num_fg; P.region_w = r->d_region_w;
    for (int k = 0; k < r->num_regions; ++k) P.regions[k] = r->regions[k];
    with_dtype(a->dtype, [&](auto* tag) { launch_lattice_regions<std::remove_pointer_t<decltype(tag)>>(P, a->method, as_stream(stream)); });
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}
