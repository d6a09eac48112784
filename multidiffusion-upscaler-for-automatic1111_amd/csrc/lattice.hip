// The jittered tile grid on a plain (bounded) canvas: mdtile_lattice_* , mdtile_gather_all_lattice, mdtile_blend_lattice,
// region prompt control under it: mdtile_blend_lattice_regions, and inpaint tile skipping under it: mdtile_lattice_activity,
// mdtile_lattice_subset_*, mdtile_gather_all_lattice_sparse, mdtile_blend_lattice_sparse.
//
// Per axis (x shown; y likewise with th, H, sy): stride st = tw - ov, shift s in [1, st], off = s - st in (-st, 0].
//     u_k  = off + k st,  k = 0 .. K          the LATTICE origins (u_0 <= 0);  K = max(0, ceil((W - tw - off) / st)) = first k with u_k + tw >= W
//     x'_k = min(max(u_k, 0), W - tw)         the PUSHED-IN box the model is run on: inside the canvas, full size
// An axis whose tile is as large as the canvas has one tile at 0 and does not move (here: stride 1, off 0, K 0).
// A tile is EVALUATED at its pushed-in box but CONTRIBUTES only where its lattice box lies: tile k covers x iff u_k <= x < u_k + tw, so every tile
// border sits at some u_k or u_k + tw and moves with s.  The covering tiles of x are the contiguous range
//     max(0, floor((x - tw - off) / st) + 1) .. min(K, floor((x - off) / st))
// (a FLOOR division: the numerators are negative near the left edge), and 0 <= x - x'_k < tw for each of them.
//
// Nothing here has a table or a map: the grid of a step is the handful of integers of mdtile_lattice, the kernels take them by value and derive
// the covering tiles AND the weight sum of a pixel from them.  So a new grid every sampler step costs no allocation, no upload and no extra launch.
//
// Arithmetic (what the sequential `+=` loop over the tile list gives, bit for bit; -ffp-contract=off):
//     wsum[y, x] = sum of w_t over the covering tiles in ascending t = r cols + c (rows outer), fp32 from +0.0;  MultiDiffusion w_t = 1.0f, Mixture of
//                  Diffusers w_t = tile_w[y - v_r, x - u_c], read in LATTICE coordinates (the Gaussian tapers at the moving borders)
//     MD : buf += v;                                          out = wsum > 1 ? buf / wsum : buf
//     MoD: buf += v * (tile_w[y - v_r, x - u_c] * (1.0f / wsum))
// with v the tile's value at the PUSHED-IN coordinates (y - y'_r, x - x'_c).  All fp32 arithmetic is written on scalars.
//
// WITH REGIONS (k_lattice_blend<..., REGIONS = true>; the other instantiations hold none of it) the regions are ordinary rectangles that stay where
// the user put them on the canvas.  The weight sum of a pixel is another one every step -- the set of covering tiles moves, the regions do not --
// so it is formed per pixel:
//     gw   = lat_wsum(...)                         exactly what mdtile_lattice_weight_map writes and the kernel without regions divides by
//     wsum = region_w ? gw + region_w[y, x] : gw   region_w: the background regions' weight sum on the canvas, made once per job
//     Mixture of Diffusers: rinv = 1.0f / wsum     IEEE division; the lattice covers every pixel, so wsum > 0
// Region weights arrive RAW and are multiplied by rinv here -- mdtile_blend takes them premultiplied by its per-job reciprocal map, which cannot
// hold when the reciprocal changes every step (the same convention, for the same reason, as mdtile_blend_wrap_regions, wrap.hip).
// Order: the grid tiles as above, then the background regions in list order, the MultiDiffusion division, then the foreground composite over the
// foreground regions in list order (blend_tail's arithmetic, blend.hip).  One thread writes each canvas pixel once; no LDS, no atomics.
//
// WITH TILE SKIPPING (k_lattice_blend<..., SPARSE = true>, k_lattice_gather<T, SPARSE = true>; the other instantiations hold none of it; never
// together with REGIONS) a tile is ACTIVE iff the mask is not zero somewhere in its CONTRIBUTING box (the lattice box clipped to the canvas), only
// the active tiles have an output, in compact batches indexed by slot[t], and a pixel is LIVE iff every lattice tile that covers it is active.  A
// live pixel gets the sum above over the same terms in the same order (the weight sum runs over ALL covering tiles: they are all active there);
// any other pixel gets the bit pattern of fill[n, c, y, x], and no tile output is read for it: liveness is decided from the slot table in front of
// the plane walk.  A slot outside [0, num_active) counts as "not active", so no table can make a kernel read or write outside a batch.
#include "launchers.h"
#include "lattice.h"

using namespace mdt;

namespace {

// most blocks along grid.y: kernels walk the planes (n * C + c) from blockIdx.y in steps of gridDim.y, so N * C may pass it
constexpr int kPlaneBlocks = 64;

struct LatticeGatherParams : LatticeParams {
    const void* x_in;
    void* batch[MDTILE_MAX_BATCHES];
};
static_assert(sizeof(LatticeGatherParams) <= 4096, "kernel argument block must stay under 4 KiB");
struct LatticeSparseGatherParams : LatticeGatherParams {      // tile_bs: the compact batches'
    const int* slot;
    int num_active;
};
static_assert(sizeof(LatticeSparseGatherParams) <= 4096, "kernel argument block must stay under 4 KiB");
// weights[y, x] = wsum (written, not added)
__global__ __launch_bounds__(256) void k_lattice_weight(const LatticeParams P, const float* __restrict__ tile_w, float* __restrict__ weights) {
    const int W = P.ax.extent, H = P.ay.extent;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W * H) return;
    const int y = idx / W, x = idx - y * W;
    const Cover rows = lat_cover(P.ay, y, y), cols = lat_cover(P.ax, x, x);
    weights[idx] = tile_w ? lat_wsum<true>(P, y, x, rows, cols, tile_w) : lat_wsum<false>(P, y, x, rows, cols, tile_w);
}

// tile t = r cols + c, tile-major compact batches: x_tile[(t mod tile_bs) N + n, ch, ty, tx] of batch t / tile_bs = x_in[n, ch, y'_r + ty, x'_c + tx].
// A pushed-in box lies on the canvas, so the copy has no edge case but the last quad of a tile row; the elements move as integers.
// grid: x = quads over (th rows x ceil(tw / 4)), y = planes (walked in steps of gridDim.y), z = tile
// SPARSE: blockIdx.z still walks every lattice tile, and a block whose tile has no slot returns after that one load of slot[t], before any other
// access; an active tile goes to its slot's place in the compact batches
template <typename T, bool SPARSE = false>
__global__ __launch_bounds__(256) void k_lattice_gather(const std::conditional_t<SPARSE, LatticeSparseGatherParams, LatticeGatherParams> P) {
    using R = typename RawOf<T>::type;
    const int W = P.ax.extent, H = P.ay.extent, tw = P.ax.tile, th = P.ay.tile;
    const int tw4 = (tw + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= tw4 * th) return;
    const int ty = idx / tw4, tx0 = (idx - ty * tw4) << 2;
    int t = blockIdx.z;
    const int r = t / P.cols, c = t - r * P.cols;
    const int sy = lat_pushed(P.ay, r) + ty, sx = lat_pushed(P.ax, c) + tx0;      // sy < H; sx + nvalid <= W
    if constexpr (SPARSE) {
        t = P.slot[t];
        if (t < 0 || t >= P.num_active) return;
    }
    const int b = t / P.tile_bs, i = t - b * P.tile_bs;
    const int planes = P.N * P.C;
    const int nvalid = tw - tx0 < 4 ? tw - tx0 : 4;
    for (int plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const R* src = reinterpret_cast<const R*>(P.x_in) + ((size_t)plane * H + sy) * W + sx;
        R* dst = reinterpret_cast<R*>(P.batch[b]) + (((size_t)i * planes + plane) * th + ty) * tw + tx0;
        if (nvalid == 4) {
            *reinterpret_cast<raw4_u<R>*>(dst) = *reinterpret_cast<const raw4_u<R>*>(src);
        } else {
            for (int j = 0; j < nvalid; ++j) dst[j] = src[j];
        }
    }
}

// active[t] = some element of mask[:, contributing box of t] is not equal to zero.  k_tile_activity's scheme (sparse.hip) on the lattice box
// clipped to the canvas: one block per tile, a lane ORs `!(v == 0.0f)` over its quads of the box's row segments (16-byte loads at whatever
// alignment the shift leaves; the last quad of a segment per element), a wave reduces by ballot, the four waves meet in LDS and one lane stores
// the flag: every entry is written by exactly one plain store.
__global__ __launch_bounds__(256) void k_lattice_activity(const LatticeParams P, int planes, const float* __restrict__ mask, int* __restrict__ active) {
    __shared__ int s_any[4];
    const int W = P.ax.extent, H = P.ay.extent;
    const int t = blockIdx.x;
    const int r = t / P.cols, c = t - r * P.cols;
    const int u = lat_origin(P.ax, c), v = lat_origin(P.ay, r);
    const int x0 = u < 0 ? 0 : u, x1 = u + P.ax.tile < W ? u + P.ax.tile : W;      // never empty: every lattice tile meets the canvas
    const int y0 = v < 0 ? 0 : v, y1 = v + P.ay.tile < H ? v + P.ay.tile : H;
    const int cw = x1 - x0, ch = y1 - y0;
    const int cw4 = (cw + 3) >> 2;
    const int per_plane = cw4 * ch;
    const long long total = (long long)per_plane * planes;
    bool any = false;
    for (long long q = threadIdx.x; q < total; q += 256) {
        const int plane = (int)(q / per_plane), rem = (int)(q - (long long)plane * per_plane);
        const int ty = rem / cw4, tx = (rem - ty * cw4) << 2;
        const float* src = mask + ((size_t)plane * H + y0 + ty) * W + x0 + tx;
        if (tx + 3 < cw) {
            float m[4];
            load4<float>(src, m);
            any = any || !(m[0] == 0.0f) || !(m[1] == 0.0f) || !(m[2] == 0.0f) || !(m[3] == 0.0f);
        } else {
            for (int j = 0; tx + j < cw; ++j) any = any || !(src[j] == 0.0f);
        }
    }
    const bool wave_any = __ballot(any) != 0;
    if ((threadIdx.x & 63) == 0) s_any[threadIdx.x >> 6] = wave_any ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) active[t] = (s_any[0] | s_any[1] | s_any[2] | s_any[3]) ? 1 : 0;
}

// slot[t] = number of active t' < t where t is active, else -1.  One block: thread i owns the tiles [i chunk, (i + 1) chunk), counts its active
// ones, the 256 counts are summed in order through LDS, and the thread numbers its tiles from the sum of the counts in front of it.  chunk <= 256
// (at most 65535 tiles), every entry written once.
__global__ __launch_bounds__(256) void k_lattice_slots(int T, const int* __restrict__ active, int* __restrict__ slot) {
    __shared__ int s_count[256];
    const int chunk = (T + 255) / 256;
    const int lo = threadIdx.x * chunk, hi = lo + chunk < T ? lo + chunk : T;
    int n = 0;
    for (int t = lo; t < hi; ++t) n += active[t] != 0;
    s_count[threadIdx.x] = n;
    __syncthreads();
    int rank = 0;
    for (int i = 0; i < (int)threadIdx.x; ++i) rank += s_count[i];
    for (int t = lo; t < hi; ++t) slot[t] = active[t] != 0 ? rank++ : -1;
}

// One thread owns one aligned quad (4 consecutive canvas columns of one row) for PP planes at a time, and walks the planes from blockIdx.y * PP
// in steps of gridDim.y * PP.  The tile rows that cover y and the tile columns that cover ANY pixel of the quad come from the lattice integers;
// the weight sums of the four pixels are formed once, in front of the plane walk.  Per candidate tile the quad is either one whole piece of the
// tile's CONTRIBUTING row segment (lattice-relative columns d0 .. d0 + 3 all in [0, tw)) -- one element-aligned vector load per plane (load4:
// 16 bytes of fp32, 8 of a 16-bit type, at any alignment) -- or it is cut by a lattice border / the canvas edge: per-element loads of the covered
// pixels only.  The part of a pushed-in tile outside its lattice box is never read.
// REGIONS: region_w is added to the four weight sums in front of the plane walk, and the region tail runs behind the tile walk, per element at
// plain canvas coordinates.
// SPARSE: a pass over the slots of the candidate tiles in front of everything else gives each pixel of the quad its live bit.  The walk skips the
// tiles that are not active, finds an active tile's rows by its slot and adds the pixels that are covered AND live; the one-load piece needs all
// four live.  A quad with no live pixel reads no tile and no weight and moves fill's four elements as one vector; a mixed quad selects per element.
template <bool REGIONS, bool SPARSE>
using LatticeBlendArgs = std::conditional_t<REGIONS, LatticeRegionsParams, std::conditional_t<SPARSE, LatticeSparseParams, LatticeBlendParams>>;

template <typename T, int METHOD, int PP, bool REGIONS = false, bool SPARSE = false>
__global__ __launch_bounds__(256) void k_lattice_blend(const LatticeBlendArgs<REGIONS, SPARSE> P) {
    static_assert(!(REGIONS && SPARSE), "tile skipping is never combined with regions");
    using Raw = typename RawOf<T>::type;
    const int W = P.ax.extent, H = P.ay.extent, tw = P.ax.tile, th = P.ay.tile;
    const int W4 = (W + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W4 * H) return;
    const int y = idx / W4, x0 = (idx - y * W4) << 2;
    const int nvalid = W - x0 < 4 ? W - x0 : 4;
    const int planes = P.N * P.C;                              // the host guarantees planes % PP == 0
    const size_t tile_elems = (size_t)th * tw;

    const Cover rows = lat_cover(P.ay, y, y), cand = lat_cover(P.ax, x0, x0 + nvalid - 1);
    [[maybe_unused]] bool live[4];
    [[maybe_unused]] bool all_live = true, any_live = true;    // of the pixels on the canvas; not sparse: every tile has an output
    if constexpr (SPARSE) {
#pragma unroll
        for (int j = 0; j < 4; ++j) live[j] = j < nvalid;
        for (int r = rows.lo; r <= rows.hi; ++r) {
            for (int c = cand.lo; c <= cand.hi; ++c) {
                const int s = P.slot[r * P.cols + c];
                if (s >= 0 && s < P.num_active) continue;
                const int d0 = x0 - lat_origin(P.ax, c);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (d0 + j >= 0 && d0 + j < tw) live[j] = false;
            }
        }
        all_live = live[0] && live[1] && live[2] && live[3];   // then nvalid == 4
        any_live = live[0] || live[1] || live[2] || live[3];
    }
    float wsum[4] = {0.f, 0.f, 0.f, 0.f}, rinv[4] = {0.f, 0.f, 0.f, 0.f};      // pixels past the canvas (j >= nvalid) keep 0 and are never used
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (j >= nvalid) continue;
        if constexpr (SPARSE) {
            if (!live[j]) continue;                            // never used: the pixel takes fill
        }
        wsum[j] = lat_wsum<METHOD == MDTILE_METHOD_MOD>(P, y, x0 + j, rows, cand, P.tile_w);
        if constexpr (REGIONS) {
            if (P.region_w) wsum[j] = wsum[j] + P.region_w[(size_t)y * W + x0 + j];
        }
        if (METHOD == MDTILE_METHOD_MOD) rinv[j] = 1.0f / wsum[j];      // IEEE division, as mdtile_reciprocal
    }

    for (int p0 = blockIdx.y * PP; p0 < planes; p0 += gridDim.y * PP) {
        float acc[PP][4];
#pragma unroll
        for (int pp = 0; pp < PP; ++pp)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[pp][j] = 0.f;

        if constexpr (SPARSE) {
            if (!any_live) {                                   // fill alone: one load and one store per plane, or the row end's elements
#pragma unroll
                for (int pp = 0; pp < PP; ++pp) {
                    const size_t off = ((size_t)(p0 + pp) * H + y) * W + x0;
                    const Raw* fill = reinterpret_cast<const Raw*>(P.fill) + off;
                    Raw* dst = reinterpret_cast<Raw*>(P.out) + off;
                    if (nvalid == 4) {
                        *reinterpret_cast<raw4_u<Raw>*>(dst) = *reinterpret_cast<const raw4_u<Raw>*>(fill);
                    } else {
                        for (int j = 0; j < nvalid; ++j) dst[j] = fill[j];
                    }
                }
                continue;
            }
        }

        for (int r = rows.lo; r <= rows.hi; ++r) {             // ascending tile index: rows outer, columns inner
            const int wy = y - lat_origin(P.ay, r);            // row inside the lattice box (and inside the tile-weight map)
            const int ty = y - lat_pushed(P.ay, r);            // row inside the pushed-in box: where the tile's value lies
            for (int c = cand.lo; c <= cand.hi; ++c) {
                const int d0 = x0 - lat_origin(P.ax, c);       // lattice-relative column of the quad's first pixel
                const int tx = x0 - lat_pushed(P.ax, c);       // pushed-in-relative column of it
                int t = r * P.cols + c;                        // the tile's place in the batches: its index, with tile skipping its slot
                if constexpr (SPARSE) {
                    t = P.slot[t];
                    if (t < 0 || t >= P.num_active) continue;  // no pixel it covers is live
                }
                const int b = t / P.tile_bs, i = t - b * P.tile_bs;
                const T* row = reinterpret_cast<const T*>(P.batch[b]) + ((size_t)i * planes + p0) * tile_elems + (size_t)ty * tw;
                // the four values are consecutive in memory (then 0 <= tx and tx + 3 < tw): one load per plane at whatever alignment the shift and
                // the batch pointer leave -- an odd shift puts EVERY tile row off its 16-byte boundary, so this is the common case, not the edge
                bool whole = nvalid == 4 && d0 >= 0 && d0 + 3 < tw;
                if constexpr (SPARSE) whole = whole && all_live;
                if (whole) {
                    float wg[4] = {1.f, 1.f, 1.f, 1.f};
                    if (METHOD == MDTILE_METHOD_MOD) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) wg[j] = P.tile_w[wy * tw + d0 + j] * rinv[j];
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
                        if constexpr (SPARSE) {
                            if (!live[j]) continue;
                        }
                        float wgt = 1.0f;
                        if (METHOD == MDTILE_METHOD_MOD) wgt = P.tile_w[wy * tw + dj] * rinv[j];
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
        if constexpr (REGIONS) {
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
                    if (METHOD == MDTILE_METHOD_MOD) wgt = R.weight[off] * rinv[j];
#pragma unroll
                    for (int pp = 0; pp < PP; ++pp) {
                        const float v = to_f32<T>(src[(size_t)pp * rplane]);
                        if (METHOD == MDTILE_METHOD_MOD) acc[pp][j] += v * wgt;
                        else acc[pp][j] += v;
                    }
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
        if constexpr (REGIONS) {
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
        }

        // one element-aligned group of four, or the row end's elements
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) {
            Raw* dst = reinterpret_cast<Raw*>(P.out) + ((size_t)(p0 + pp) * H + y) * W + x0;
            if constexpr (SPARSE) {
                if (!all_live) {                               // a mixed quad (or a row end): per element, fill's bits where the pixel is not live
                    const Raw* fill = reinterpret_cast<const Raw*>(P.fill) + ((size_t)(p0 + pp) * H + y) * W + x0;
                    for (int j = 0; j < nvalid; ++j) dst[j] = live[j] ? raw_bits<T>(acc[pp][j]) : fill[j];
                    continue;
                }
            }
            if (nvalid == 4) {
                raw4_u<Raw> o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o.v[j] = raw_bits<T>(acc[pp][j]);
                *reinterpret_cast<raw4_u<Raw>*>(dst) = o;
            } else {
                for (int j = 0; j < nvalid; ++j) dst[j] = raw_bits<T>(acc[pp][j]);
            }
        }
    }
}

template <typename T, int PP, bool REGIONS, bool SPARSE>
auto lattice_blend_kernel(int method) {
    return method == MDTILE_METHOD_MD ? k_lattice_blend<T, MDTILE_METHOD_MD, PP, REGIONS, SPARSE> : k_lattice_blend<T, MDTILE_METHOD_MOD, PP, REGIONS, SPARSE>;
}

// PP is sized for the walk alone; whether another size pays with the region tail behind it is not measured
template <typename T, bool REGIONS, bool SPARSE = false>
void launch_lattice_blend(const LatticeBlendArgs<REGIONS, SPARSE>& P, int method, hipStream_t s) {
    const int W = P.ax.extent, H = P.ay.extent, planes = P.N * P.C;
    const int pp = planes_per_thread(W, H, planes);
    const auto k = pp == 4   ? lattice_blend_kernel<T, 4, REGIONS, SPARSE>(method)
                   : pp == 2 ? lattice_blend_kernel<T, 2, REGIONS, SPARSE>(method)
                             : lattice_blend_kernel<T, 1, REGIONS, SPARSE>(method);
    const int gy = planes / pp < kPlaneBlocks ? planes / pp : kPlaneBlocks;
    hipLaunchKernelGGL(k, dim3(cdiv((long long)H * ((W + 3) / 4), 256), gy), dim3(256), 0, s, P);
}

// What mdtile_blend_lattice and mdtile_blend_lattice_regions ask of the arguments they share, and the (zeroed) argument block filled from them;
// errors name `fn`
int lattice_blend_args(const char* fn, const mdtile_lattice* lat, const mdtile_blend_args* a, const void* const* batch_out, int num_batches,
                       LatticeBlendParams& P, const mdtile_lattice_subset* sub = nullptr) {
    if (int rc = lattice_check(fn, lat)) return rc;
    MDT_CHECK_ARG(a && batch_out, "%s: null argument", fn);
    // what this form does not do, by name
    MDT_CHECK_ARG(a->flags == 0, "%s: the lattice takes no MDTILE_BLEND_* flags (flags=%d): no partial sums, tile range or packed buffer", fn, a->flags);
    MDT_CHECK_ARG(a->row_lo == 0 && a->row_hi == 0, "%s: the lattice takes no row band [%d,%d): it is not combined with the multi-GPU path", fn, a->row_lo,
                  a->row_hi);
    MDT_CHECK_ARG(!a->d_weights && !a->d_rescale, "%s: d_weights and d_rescale must be NULL: the kernel forms the weight sum of the step's grid itself", fn);
    MDT_CHECK_ARG(a->N > 0 && a->C > 0 && a->N * a->C <= 65535, "%s: bad N=%d C=%d", fn, a->N, a->C);
    MDT_CHECK_ARG(a->method == MDTILE_METHOD_MD || a->method == MDTILE_METHOD_MOD, "%s: bad method %d", fn, a->method);
    MDT_CHECK_ARG(a->dtype >= 0 && a->dtype <= 2, "%s: bad dtype %d", fn, a->dtype);
    MDT_CHECK_ARG(a->d_x_out, "%s: null output", fn);
    MDT_CHECK_ARG(a->method != MDTILE_METHOD_MOD || a->d_tile_w, "%s: Mixture of Diffusers needs d_tile_w", fn);
    if (int rc = sub ? subset_batches_check(fn, sub, num_batches) : batches_check(fn, lat, num_batches)) return rc;
    for (int b = 0; b < num_batches; ++b) MDT_CHECK_ARG(batch_out[b], "%s: null batch pointer %d", fn, b);
    fill_params(P, lat, a->N, a->C);
    P.tile_w = a->method == MDTILE_METHOD_MOD ? a->d_tile_w : nullptr;
    P.out = a->d_x_out;
    for (int b = 0; b < num_batches; ++b) P.batch[b] = batch_out[b];
    return MDTILE_OK;
}

}  // namespace

extern "C" int mdtile_lattice_make(int w, int h, int tile_w, int tile_h, int overlap, int tile_bs, int sx, int sy, mdtile_lattice* lat) {
    const char* fn = "mdtile_lattice_make";
    MDT_CHECK_ARG(lat, "%s: null lattice", fn);
    MDT_CHECK_ARG(w > 0 && h > 0 && tile_w > 0 && tile_h > 0 && tile_bs > 0 && w <= 65535 && h <= 65535, "%s: bad arguments w=%d h=%d tile=%dx%d bs=%d", fn, w, h,
                  tile_w, tile_h, tile_bs);
    // the clamp of mdtile_plan_create(clamp = 1)
    const int tw = tile_w < w ? tile_w : w, th = tile_h < h ? tile_h : h;
    const int mn = tile_w < tile_h ? tile_w : tile_h;     // requested, not clamped, sizes
    int ov = overlap < mn - 4 ? overlap : mn - 4;
    if (ov < 0) ov = 0;
    MDT_CHECK_ARG(tw - ov != 0 && th - ov != 0, "%s: overlap %d equals the canvas-clamped tile %dx%d (mdtile_plan_create refuses it too)", fn, ov, tw, th);
    mdtile_lattice l;
    l.w = w; l.h = h; l.tile_w = tw; l.tile_h = th; l.overlap = ov;
    l.stride_x = tw - ov; l.stride_y = th - ov;
    const bool move_x = tw < w, move_y = th < h;          // a moving axis has tile == requested tile, so its stride is >= 4
    MDT_CHECK_ARG(!move_x || (sx >= 1 && sx <= l.stride_x), "%s: shift sx = %d outside [1, %d] (the stride) on an axis that moves", fn, sx, l.stride_x);
    MDT_CHECK_ARG(!move_y || (sy >= 1 && sy <= l.stride_y), "%s: shift sy = %d outside [1, %d] (the stride) on an axis that moves", fn, sy, l.stride_y);
    l.sx = move_x ? sx : 0;
    l.sy = move_y ? sy : 0;
    l.cols = move_x ? axis_tiles(w, tw, l.stride_x, sx) : 1;
    l.rows = move_y ? axis_tiles(h, th, l.stride_y, sy) : 1;
    MDT_CHECK_ARG(l.cols <= 32767 && l.rows <= 32767, "%s: too many tiles (%d x %d)", fn, l.cols, l.rows);
    l.num_tiles = l.cols * l.rows;
    l.num_batches = (l.num_tiles + tile_bs - 1) / tile_bs;
    l.tile_bs = (l.num_tiles + l.num_batches - 1) / l.num_batches;
    *lat = l;
    return MDTILE_OK;
}

extern "C" int mdtile_lattice_bboxes(const mdtile_lattice* lat, int* xywh) {
    if (int rc = lattice_check("mdtile_lattice_bboxes", lat)) return rc;
    MDT_CHECK_ARG(xywh, "mdtile_lattice_bboxes: null argument");
    LatticeParams P;
    fill_params(P, lat, 1, 1);
    for (int r = 0; r < lat->rows; ++r)
        for (int c = 0; c < lat->cols; ++c) {
            int* o = xywh + 4 * (r * lat->cols + c);
            o[0] = lat_pushed(P.ax, c); o[1] = lat_pushed(P.ay, r); o[2] = lat->tile_w; o[3] = lat->tile_h;
        }
    return MDTILE_OK;
}

extern "C" int mdtile_lattice_weight_map(const mdtile_lattice* lat, const float* d_tile_w, float* d_weights, mdtile_stream_t stream) {
    if (int rc = lattice_check("mdtile_lattice_weight_map", lat)) return rc;
    MDT_CHECK_ARG(d_weights, "mdtile_lattice_weight_map: null output");
    LatticeParams P;
    fill_params(P, lat, 1, 1);
    hipLaunchKernelGGL(k_lattice_weight, dim3(cdiv((long long)lat->w * lat->h, 256)), dim3(256), 0, as_stream(stream), P, d_tile_w, d_weights);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_gather_all_lattice(const mdtile_lattice* lat, int dtype, int N, int C, const void* d_x_in, void* const* batch_ptrs, int num_batches,
                                         mdtile_stream_t stream) {
    const char* fn = "mdtile_gather_all_lattice";
    if (int rc = lattice_check(fn, lat)) return rc;
    MDT_CHECK_ARG(d_x_in && batch_ptrs, "%s: null argument", fn);
    MDT_CHECK_ARG(N > 0 && C > 0 && N * C <= 65535, "%s: bad N=%d C=%d", fn, N, C);
    MDT_CHECK_ARG(dtype >= 0 && dtype <= 2, "%s: bad dtype %d", fn, dtype);
    if (int rc = batches_check(fn, lat, num_batches)) return rc;
    MDT_CHECK_ARG(lat->num_tiles <= 65535, "%s: %d tiles in one launch (at most 65535)", fn, lat->num_tiles);
    for (int b = 0; b < num_batches; ++b) MDT_CHECK_ARG(batch_ptrs[b], "%s: null batch pointer %d", fn, b);
    LatticeGatherParams P;
    memset(&P, 0, sizeof(P));
    fill_params(P, lat, N, C);
    P.x_in = d_x_in;
    for (int b = 0; b < num_batches; ++b) P.batch[b] = batch_ptrs[b];
    const int planes = N * C;
    dim3 grid(cdiv((long long)lat->tile_h * ((lat->tile_w + 3) / 4), 256), planes < kPlaneBlocks ? planes : kPlaneBlocks, lat->num_tiles), block(256);
    with_dtype(dtype, [&](auto* tag) { hipLaunchKernelGGL((k_lattice_gather<std::remove_pointer_t<decltype(tag)>>), grid, block, 0, as_stream(stream), P); });
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_blend_lattice(const mdtile_lattice* lat, const mdtile_blend_args* a, const void* const* batch_out, int num_batches,
                                    mdtile_stream_t stream) {
    LatticeBlendParams P;
    memset(&P, 0, sizeof(P));
    if (int rc = lattice_blend_args("mdtile_blend_lattice", lat, a, batch_out, num_batches, P)) return rc;
    with_dtype(a->dtype, [&](auto* tag) { launch_lattice_blend<std::remove_pointer_t<decltype(tag)>, false>(P, a->method, as_stream(stream)); });
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_blend_lattice_regions(const mdtile_lattice* lat, const mdtile_blend_args* a, const void* const* batch_out, int num_batches,
                                            const mdtile_lattice_regions* r, mdtile_stream_t stream) {
    const char* fn = "mdtile_blend_lattice_regions";
    LatticeRegionsParams P;
    memset(&P, 0, sizeof(P));
    if (int rc = lattice_blend_args(fn, lat, a, batch_out, num_batches, P)) return rc;
    MDT_CHECK_ARG(r, "%s: null regions block (mdtile_blend_lattice is the call without regions)", fn);
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
    P.num_regions = r->num_regions; P.num_fg = num_fg; P.region_w = r->d_region_w;
    for (int k = 0; k < r->num_regions; ++k) P.regions[k] = r->regions[k];
    with_dtype(a->dtype, [&](auto* tag) { launch_lattice_blend<std::remove_pointer_t<decltype(tag)>, true>(P, a->method, as_stream(stream)); });
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

// ---- inpaint tile skipping under the jittered grid ------------------------------------------------------------------------
extern "C" int mdtile_lattice_activity(const mdtile_lattice* lat, const float* d_mask, int planes, int* d_active, int* d_slot, mdtile_stream_t stream) {
    const char* fn = "mdtile_lattice_activity";
    if (int rc = lattice_check(fn, lat)) return rc;
    MDT_CHECK_ARG(d_mask && d_active && d_slot, "%s: null argument", fn);
    MDT_CHECK_ARG(planes >= 1 && planes <= 65535, "%s: bad planes=%d", fn, planes);
    MDT_CHECK_ARG(lat->num_tiles <= 65535, "%s: %d tiles (at most 65535: the ranks are written by one block)", fn, lat->num_tiles);
    LatticeParams P;
    fill_params(P, lat, 1, 1);
    hipLaunchKernelGGL(k_lattice_activity, dim3(lat->num_tiles), dim3(256), 0, as_stream(stream), P, planes, d_mask, d_active);
    hipLaunchKernelGGL(k_lattice_slots, dim3(1), dim3(256), 0, as_stream(stream), lat->num_tiles, d_active, d_slot);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_lattice_subset_make(const mdtile_lattice* lat, const int* h_active, int tile_bs, const int* d_slot, mdtile_lattice_subset* sub) {
    const char* fn = "mdtile_lattice_subset_make";
    if (int rc = lattice_check(fn, lat)) return rc;
    MDT_CHECK_ARG(h_active && sub, "%s: null argument", fn);
    MDT_CHECK_ARG(d_slot, "%s: null d_slot: the blend and the gather find an active tile's place in the compact batches there", fn);
    MDT_CHECK_ARG(tile_bs > 0, "%s: bad tile_bs=%d", fn, tile_bs);
    int Ta = 0;
    for (int t = 0; t < lat->num_tiles; ++t) Ta += h_active[t] != 0;
    MDT_CHECK_ARG(Ta >= 1, "%s: no active tile: num_active = 0 outside [1, %d] (there is nothing to run)", fn, lat->num_tiles);
    const int nb = (Ta - 1) / tile_bs + 1;                // ceil(Ta / tile_bs), Ta >= 1, for any tile_bs up to INT_MAX
    MDT_CHECK_ARG(nb <= MDTILE_MAX_BATCHES, "%s: %d active tiles make %d batches > MDTILE_MAX_BATCHES=%d (raise the tile batch size, or run the full lattice)", fn,
                  Ta, nb, MDTILE_MAX_BATCHES);
    mdtile_lattice_subset s;
    s.lat = *lat;
    s.num_active = Ta;
    s.num_batches = nb;
    s.tile_bs = (Ta - 1) / nb + 1;
    s.d_slot = d_slot;
    *sub = s;
    return MDTILE_OK;
}

extern "C" int mdtile_lattice_subset_bboxes(const mdtile_lattice_subset* sub, const int* h_active, int* xywh, int* ids) {
    const char* fn = "mdtile_lattice_subset_bboxes";
    if (int rc = subset_check(fn, sub)) return rc;
    MDT_CHECK_ARG(h_active && xywh, "%s: null argument", fn);
    const mdtile_lattice* lat = &sub->lat;
    int Ta = 0;
    for (int t = 0; t < lat->num_tiles; ++t) Ta += h_active[t] != 0;
    MDT_CHECK_ARG(Ta == sub->num_active, "%s: %d flags are set, the subset has %d active tiles (not the flags it was made from)", fn, Ta, sub->num_active);
    LatticeParams P;
    fill_params(P, lat, 1, 1);
    int s = 0;
    for (int t = 0; t < lat->num_tiles; ++t) {
        if (!h_active[t]) continue;
        const int r = t / lat->cols, c = t - r * lat->cols;
        int* o = xywh + 4 * s;
        o[0] = lat_pushed(P.ax, c); o[1] = lat_pushed(P.ay, r); o[2] = lat->tile_w; o[3] = lat->tile_h;
        if (ids) ids[s] = t;
        ++s;
    }
    return MDTILE_OK;
}

extern "C" int mdtile_gather_all_lattice_sparse(const mdtile_lattice_subset* sub, int dtype, int N, int C, const void* d_x_in, void* const* batch_ptrs,
                                                int num_batches, mdtile_stream_t stream) {
    const char* fn = "mdtile_gather_all_lattice_sparse";
    if (int rc = subset_check(fn, sub)) return rc;
    const mdtile_lattice* lat = &sub->lat;
    MDT_CHECK_ARG(d_x_in && batch_ptrs, "%s: null argument", fn);
    MDT_CHECK_ARG(N > 0 && C > 0 && N * C <= 65535, "%s: bad N=%d C=%d", fn, N, C);
    MDT_CHECK_ARG(dtype >= 0 && dtype <= 2, "%s: bad dtype %d", fn, dtype);
    if (int rc = subset_batches_check(fn, sub, num_batches)) return rc;
    MDT_CHECK_ARG(lat->num_tiles <= 65535, "%s: %d tiles in one launch (at most 65535)", fn, lat->num_tiles);
    for (int b = 0; b < num_batches; ++b) MDT_CHECK_ARG(batch_ptrs[b], "%s: null batch pointer %d", fn, b);
    LatticeSparseGatherParams P;
    memset(&P, 0, sizeof(P));
    fill_params(P, lat, N, C);
    P.tile_bs = sub->tile_bs;
    P.x_in = d_x_in;
    P.slot = sub->d_slot;
    P.num_active = sub->num_active;
    for (int b = 0; b < num_batches; ++b) P.batch[b] = batch_ptrs[b];
    const int planes = N * C;
    dim3 grid(cdiv((long long)lat->tile_h * ((lat->tile_w + 3) / 4), 256), planes < kPlaneBlocks ? planes : kPlaneBlocks, lat->num_tiles), block(256);
    with_dtype(dtype, [&](auto* tag) { hipLaunchKernelGGL((k_lattice_gather<std::remove_pointer_t<decltype(tag)>, true>), grid, block, 0, as_stream(stream), P); });
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_blend_lattice_sparse(const mdtile_lattice_subset* sub, const mdtile_blend_args* a, const void* const* batch_out, int num_batches,
                                           const void* d_fill, mdtile_stream_t stream) {
    const char* fn = "mdtile_blend_lattice_sparse";
    if (int rc = subset_check(fn, sub)) return rc;
    LatticeSparseParams P;
    memset(&P, 0, sizeof(P));
    if (int rc = lattice_blend_args(fn, &sub->lat, a, batch_out, num_batches, P, sub)) return rc;
    MDT_CHECK_ARG(d_fill, "%s: null fill: the pixels that are not live need a value", fn);
    P.tile_bs = sub->tile_bs;
    P.slot = sub->d_slot;
    P.fill = d_fill;
    P.num_active = sub->num_active;
    with_dtype(a->dtype, [&](auto* tag) { launch_lattice_blend<std::remove_pointer_t<decltype(tag)>, false, true>(P, a->method, as_stream(stream)); });
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}
