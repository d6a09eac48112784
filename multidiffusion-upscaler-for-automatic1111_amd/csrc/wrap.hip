// Wrap-around (panoramas, vertical strips, seamless textures): weight map, tile gather and overlap blend for a plan whose canvas is closed in x,
// in y or in both (mdtile_plan_create_wrap).  Each axis is on a circle: tile column c covers the canvas columns
// (xs[c] + i) mod W, i in [0, tw), tile row r the canvas rows (ys[r] + i) mod H, i in [0, th).  The formulation is the gather of blend.hip -- one
// thread owns its output pixels and walks the tiles that cover them -- so closing the canvas only changes WHICH tile columns / rows cover a
// canvas column / row: a cyclic run of the plan's column / row list instead of a plain range.  Nothing scatters across a seam.
//
// An axis that does not wrap (wrap_x = 0 or wrap_y = 0; the x-only panorama is the case wrap_y = 0) is the specialisation that needs no code of
// its own: a plain run never passes the end of its list and a plain tile never passes the edge, so the same arithmetic on the circle serves it.
//
// Order: the covering tiles are summed in ASCENDING tile index (rows outer, columns inner; a cyclic run is walked as [0, head) then
// [first, ...)), which is the order of the sequential `+=` loop over the tile list; at a seam pixel tile column 0 therefore comes before column
// cols - 1, and tile row 0 before row rows - 1.  Per-term operations and epilogues are those of k_blend's generic walk (blend.hip): Mixture of
// Diffusers w = tile_w * rescale[y, x], term out * w; MultiDiffusion weights > 1 ? buf / weights : buf.  fp32 accumulation from +0.0,
// -ffp-contract=off: results equal the sequential loop bit for bit.
//
// SPARSE plans (mdtile_plan_create_subset; sparse.hip has the entry point and the activity kernel) are gathered and blended by
// the same two kernels: their parent is always a plain plan, so the arithmetic on the circle serves it as it serves an axis that does not
// wrap.  What they add -- the gather's `active` table, the blend's liveness pass over `slot`, the skip of tiles that are not active and the
// `fill` pass-through -- is compiled into k_walk_blend<..., SPARSE = true> only; the wrap-around instantiations hold none of it.
//
// The SHIFTED grid (mdtile_gather_all_shift / mdtile_blend_shift; wrap-around plans only) displaces every tile origin by (sx, sy)
// on the circle.  That changes neither which tile indices cover a pixel nor their order, it moves the pixel: the gather adds the shift to the
// source coordinate, the blend keeps its threads on PLAN coordinates and adds it to the store address.  Both are compiled under
// `if constexpr (SHIFT)` into instantiations of their own, with an argument block of their own; the others hold none of it.
//
// CUSTOM REGIONS on a wrap-around plan (mdtile_blend_wrap_regions; wrap_regions.hip has the entry point and the three rect calls)
// are k_walk_blend<..., REGIONS = true>: the walk of the shifted grid on the thread's quad of PLAN coordinates, then the region tail of blend_tail
// (blend.hip) at the quad's CANVAS coordinates.  The other instantiations hold none of it, and mdtile_blend / mdtile_blend_shift still refuse
// regions on such a plan.  A region R covers canvas pixel (yc, xc) iff ry = rel(yc, R.y, H) < R.h and rx = rel(xc, R.x, W) < R.w; its value and
// weight are read at ry * R.w + rx.  The host has checked 0 <= R.x < W, 0 < R.w <= W (likewise y) and that a region passes an edge only on an axis
// that wraps, so on an axis that does not wrap rel() of a pixel in front of the region is >= extent - R.x >= R.w: not covered, with the same
// arithmetic.  The weight sum is formed in the kernel, per pixel: the grid's map travels with the shift (plan coordinates), the background
// regions' map stays on the canvas, so their sum is another one every step and nothing made once per job holds it:
//     wsum = grid_w[yp, xp] + region_w[yc, xc];   Mixture of Diffusers: resc = 1.0f / wsum   (IEEE division, as mdtile_reciprocal and k_lattice_blend)
// Region weights arrive RAW and are multiplied by resc here -- mdtile_blend takes them premultiplied by its per-job reciprocal map.  Order: the
// grid tiles as above, then the background regions in list order, the MultiDiffusion division, then the foreground composite over the foreground
// regions in list order.  One thread writes each canvas pixel once; no LDS, no atomics.
//
// Not here (refused with an error that names the reason): custom regions through mdtile_blend / mdtile_blend_shift, MDTILE_BLEND_* flags, row
// bands, mdtile_gather_range, mdtile_blend_finalize -- tile skipping is not combined with regions, and neither wrap-around nor tile skipping
// with the multi-GPU partial path.
#include "launchers.h"
#include "walk.h"

using namespace mdt;

namespace {

// weights[p] += sum over the covering tiles, ascending tile index (rows outer, columns inner), of tile_w[...] (or 1.0)
__global__ __launch_bounds__(256) void k_wrap_weight_grid(int W, int H, int tw, int cols, int rows, const int* __restrict__ xs,
                                                          const int* __restrict__ ys, const int* __restrict__ colrange,
                                                          const int* __restrict__ rowrange, const float* __restrict__ tile_w,
                                                          float* __restrict__ weights) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W * H) return;
    const int y = idx / W, x = idx - y * W;
    const CyclicRun run(colrange[x], cols), rrun(rowrange[y], rows);
    float s = 0.0f;
    for (int kr = 0; kr < rrun.count; ++kr) {
        const int ty = rel(y, ys[rrun.at(kr)], H);
        for (int k = 0; k < run.count; ++k) {
            const int tx = rel(x, xs[run.at(k)], W);
            s += tile_w ? tile_w[ty * tw + tx] : 1.0f;
        }
    }
    weights[idx] += s;
}

struct WrapGatherParams {
    int W, H, tw, th, cols, tile_bs, N, C;
    int s_lo, _pad;
    const int *xs, *ys;
    const int* active;        // a sparse plan's active tile indices (position s holds tile active[s]); null: position s is tile s
    const void* x_in;
    void* batch[MDTILE_MAX_BATCHES];
};
static_assert(sizeof(WrapGatherParams) <= 4096, "kernel argument block must stay under 4 KiB");
// the shifted grid (mdtile_gather_all_shift): every tile origin displaced by (shift_x, shift_y) on the circle.  The kernels that
// are not shifted keep the argument block above.
struct WrapGatherShiftParams : WrapGatherParams {
    int shift_x, shift_y;     // 0 <= shift_x < W, 0 <= shift_y < H; 0 on an axis that does not wrap
};
static_assert(sizeof(WrapGatherShiftParams) <= 4096, "kernel argument block must stay under 4 KiB");

// position s (a tile of the list, or a slot of a sparse plan) holds tile t: x_tile[(s mod tile_bs) * N + n, c, ty, tx] of batch s / tile_bs =
// x_in[n, c, (y_t + ty) mod H, (x_t + tx) mod W].  grid: x = quads over (th rows x tw4), y = plane (n*C + c), z = position
// SHIFT: the origin is ((x_t + shift_x) mod W, (y_t + shift_y) mod H).  The reduced source coordinate is < extent and the shift is < extent, so
// their sum is < 2 * extent: one more subtraction, after the first (x_t + shift_x + tx itself may pass 2 W: it is never formed).
template <typename T, bool SHIFT>
__global__ __launch_bounds__(256) void k_wrap_gather(const std::conditional_t<SHIFT, WrapGatherShiftParams, WrapGatherParams> P) {
    const int tw4 = (P.tw + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= tw4 * P.th) return;
    const int ty = idx / tw4, tx0 = (idx - ty * tw4) << 2;
    const int plane = blockIdx.y, n = plane / P.C, c = plane - n * P.C;
    const int s = P.s_lo + blockIdx.z;
    const int t = P.active ? P.active[s] : s;
    const int r = t / P.cols, cc = t - r * P.cols;
    int sy = P.ys[r] + ty;                // ys < H and ty < th <= H (th == H only on plain rows, ys = 0): one subtraction brings it back onto the canvas
    if (sy >= P.H) sy -= P.H;
    if constexpr (SHIFT) {
        sy += P.shift_y;
        if (sy >= P.H) sy -= P.H;
    }
    const T* srow = reinterpret_cast<const T*>(P.x_in) + (((size_t)n * P.C + c) * P.H + sy) * P.W;
    const int b = s / P.tile_bs, i = s - b * P.tile_bs;
    T* dst = reinterpret_cast<T*>(P.batch[b]) + (((size_t)i * P.N + n) * P.C + c) * ((size_t)P.th * P.tw) + (size_t)ty * P.tw + tx0;
    int sx = P.xs[cc] + tx0;              // xs < W and tx0 < tw <= W (tw == W only on plain columns, xs = 0): likewise
    if (sx >= P.W) sx -= P.W;
    if constexpr (SHIFT) {
        sx += P.shift_x;
        if (sx >= P.W) sx -= P.W;
    }
    const int nvalid = P.tw - tx0 < 4 ? P.tw - tx0 : 4;
    if (nvalid == 4 && sx + 3 < P.W) {    // the four source columns are consecutive in memory
        float v[4];
        load4<T>(srow + sx, v);
        store4<T>(dst, v);
    } else {
        for (int j = 0; j < nvalid; ++j) {
            const int x = sx + j < P.W ? sx + j : sx + j - P.W;
            dst[j] = srow[x];
        }
    }
}

struct WalkBlendParams {
    int W, H, tw, th, cols, tile_bs, N, C;
    const int *xs, *ys;
    const int4 *colquad, *rowinfo;
    const float *weights, *tile_w, *rescale;
    void* out;
    const void* batch[MDTILE_MAX_BATCHES];
    int rows;                 // behind the pointers: the argument layout the per-axis kernel was measured with (docs/history/results_log.md)
    // a sparse plan only (SPARSE kernels; null otherwise)
    const int* slot;          // slot[t] = rank of tile t among the active ones = its place in the compact batches, or -1
    const void* fill;         // [N, C, H, W] in the storage type: the value of every pixel that is not live
};
static_assert(sizeof(WalkBlendParams) <= 4096, "kernel argument block must stay under 4 KiB");
// the shifted grid (mdtile_blend_shift): the value of plan coordinate (y, x) is stored at ((y + shift_y) mod H, (x + shift_x) mod W).
// The kernels that are not shifted keep the argument block above.
struct WalkBlendShiftParams : WalkBlendParams {
    int shift_x, shift_y;     // 0 <= shift_x < W, 0 <= shift_y < H; 0 on an axis that does not wrap
};
static_assert(sizeof(WalkBlendShiftParams) <= 4096, "kernel argument block must stay under 4 KiB");
// the shifted grid with custom regions (mdtile_blend_wrap_regions): an argument block of its own
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
template <bool SHIFT, bool REGIONS>
using WalkBlendArgs = std::conditional_t<REGIONS, WrapRegionsParams, std::conditional_t<SHIFT, WalkBlendShiftParams, WalkBlendParams>>;

// One thread owns one quad (4 consecutive canvas columns of one row; rows start at x = 0, so a quad never straddles the seam) for PP planes.
// The tile rows that cover the canvas row come from rowinfo[y].x and the tile columns that cover ANY pixel of the quad from colquad[xq].x, both
// as cyclic runs; a canvas row is one row of every tile that covers it (tile-relative row rel(y, ys[r], H)).  A TILE's row segment may straddle
// the seam: per candidate tile the quad is either one contiguous piece of the tile row (tile-relative x0 .. x0 + 3 all below tw) -- vector
// loads when that piece is also aligned in memory -- or it is cut by a tile edge / the seam: per-element loads of the covered pixels only.
//
// SPARSE (the plan of the active tiles of a plain parent): a tile that is not active has no output, and a pixel is LIVE iff every tile that
// covers it is active.  A pass over the slot table in front of the walk decides that, before the first tile value is loaded; the walk then
// skips the tiles that are not active, finds an active tile's rows in the compact batches by its slot and adds the pixels that are covered
// AND live; a pixel that is not live gets the bit pattern of `fill` (copied as integers: NaN payloads and -0.0 survive in every dtype).
// A plain tile column that starts 1 - 3 px to the right of x0 has no test of its own: xs[c] + tw <= W there, so rel() gives
// tx = W + (x0 - xs[c]) >= W - 3, hence tx + 3 >= W >= tw (never `whole`), and each tx + j either passes W and comes back as the true offset
// x0 + j - xs[c] >= 0 or stays >= x0 + tw + j >= tw, which is not covered.
//
// SHIFT (wrap-around plans only, never SPARSE): the thread still owns the quad of PLAN coordinates (y, x0 .. x0 + 3) -- the walk, the weight /
// rescale loads and the tile loads are those above -- and only its store moves: to row (y + shift_y) mod H, columns (x0 + shift_x + j) mod W.
// The displaced quad is in general not aligned and, on a wrapped x, may be cut by the seam: one element-aligned group of four when it is not
// cut, per element with the column taken mod W when it is.
//
// REGIONS (always SHIFT, at rest with shift 0): both weight maps are loaded, and for Mixture of Diffusers divided, in front of the walk, which is
// skipped when no grid is drawn (num_batches == 0); the region tail runs per element at the canvas columns xc[j], so a region that crosses a seam
// and a quad that the shift cut take the same path.
template <typename T, int METHOD, int PP, bool SPARSE, bool SHIFT, bool REGIONS = false>
__global__ __launch_bounds__(256) void k_walk_blend(const WalkBlendArgs<SHIFT, REGIONS> P) {
    static_assert(!(SPARSE && SHIFT), "a sparse plan is never shifted");
    static_assert(!REGIONS || (SHIFT && !SPARSE), "regions come with the shifted grid's store, never on a sparse plan");
    const int W4 = (P.W + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W4 * P.H) return;
    const int y = idx / W4, xq = idx - y * W4;
    const int x0 = xq << 2;
    const int p0 = blockIdx.y * PP;                        // the host guarantees N*C % PP == 0
    const int nvalid = P.W - x0 < 4 ? P.W - x0 : 4;
    const size_t tile_elems = (size_t)P.th * P.tw;

    // SHIFT: the quad's canvas pixels are row yc, columns xc[j] = (xd + j) mod W -- consecutive in memory unless the seam cuts the displaced quad
    // (`uncut`).  REGIONS place the quad here; SHIFT alone does in front of its store (here it changes hipcc's schedule of those kernels).
    [[maybe_unused]] int yc, xd, xc[4];
    [[maybe_unused]] bool uncut;
    // the weight sum and, for Mixture of Diffusers, its reciprocal; pixels past the canvas (j >= nvalid) keep 0 and are never used
    [[maybe_unused]] float wsum[4] = {0.f, 0.f, 0.f, 0.f};
    float resc[4] = {0.f, 0.f, 0.f, 0.f};
    if constexpr (REGIONS) {
        yc = onto(y + P.shift_y, P.H);                     // y < H, shift_y < H
        xd = onto(x0 + P.shift_x, P.W);                    // x0 < W, shift_x < W
        uncut = nvalid == 4 && xd + 3 < P.W;
#pragma unroll
        for (int j = 0; j < 4; ++j) xc[j] = onto(xd + j, P.W);

        // wsum = grid_w[yp, xp] + region_w[yc, xc]
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

    // which pixels of the quad get a blended value (`SPARSE ? live[j] : j < nvalid` below): those on the canvas, and of them, on a sparse plan,
    // the live ones
    [[maybe_unused]] bool live[4];
    bool all_live = true, any_live = true;                 // of the pixels on the canvas; not sparse: every tile has an output
    if constexpr (SPARSE) {
        const CyclicRun run(P.colquad[xq].x, P.cols), rrun(P.rowinfo[y].x, P.rows);
#pragma unroll
        for (int j = 0; j < 4; ++j) live[j] = j < nvalid;
        for (int kr = 0; kr < rrun.count; ++kr) {
            const int r = rrun.at(kr);
            for (int k = 0; k < run.count; ++k) {
                const int c = run.at(k);
                if (P.slot[r * P.cols + c] >= 0) continue;
                const int tx = rel(x0, P.xs[c], P.W);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    int txj = tx + j;                      // tx < W, j < 4: one subtraction
                    if (txj >= P.W) txj -= P.W;
                    if (txj < P.tw) live[j] = false;
                }
            }
        }
        all_live = live[0] && live[1] && live[2] && live[3];   // then nvalid == 4
        any_live = live[0] || live[1] || live[2] || live[3];
    }
    bool walk = any_live;
    if constexpr (REGIONS) walk = P.num_batches > 0;       // 0: no grid is drawn, and the plan's tables are not read
    if (walk) {
        const CyclicRun run(P.colquad[xq].x, P.cols), rrun(P.rowinfo[y].x, P.rows);      // (SPARSE: the liveness pass's, loaded once)
        if constexpr (!REGIONS) {
            if (METHOD == MDTILE_METHOD_MOD) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (SPARSE ? live[j] : j < nvalid) resc[j] = P.rescale[(size_t)y * P.W + x0 + j];
            }
        }

        for (int kr = 0; kr < rrun.count; ++kr) {          // ascending tile index: rows outer, columns inner
            const int r = rrun.at(kr);
            const int ty = rel(y, P.ys[r], P.H);           // < th: rowinfo holds exactly the rows that cover y
            const size_t roff = (size_t)ty * P.tw;         // the tile row inside a [th, tw] plane (and inside the tile-weight map)
            for (int k = 0; k < run.count; ++k) {
                const int c = run.at(k);
                int t = r * P.cols + c;                    // the tile's place in the batches: its index, on a sparse plan its slot
                if constexpr (SPARSE) {
                    t = P.slot[t];
                    if (t < 0) continue;                   // no pixel it covers is live
                }
                const int b = t / P.tile_bs, i = t - b * P.tile_bs;
                const int tx = rel(x0, P.xs[c], P.W);
                const T* row = reinterpret_cast<const T*>(P.batch[b]) + ((size_t)i * P.N * P.C + p0) * tile_elems + roff;
                // one contiguous piece of the tile row, every pixel live, at an address aligned for the vector load in this plane and
                // (tile_elems % 4 == 0) in the others
                // (`nvalid == 4` is tested here, not once in front of the walk: hoisted by hand it changes hipcc's schedule of the kernels that are
                // not sparse, docs/history/results_log.md)
                const bool whole = nvalid == 4 && all_live && tx + 3 < P.tw;
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
                        if (!(SPARSE ? live[j] : j < nvalid) || txj >= P.tw) continue;
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

        // MD normalisation: x = where(weights > 1, buf / weights, buf) (a sparse plan: the parent's full weight map)
        if constexpr (!REGIONS) {
            if (METHOD == MDTILE_METHOD_MD) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (!(SPARSE ? live[j] : j < nvalid)) continue;
                    const float w = P.weights[(size_t)y * P.W + x0 + j];
                    if (w > 1.0f) {
#pragma unroll
                        for (int pp = 0; pp < PP; ++pp) acc[pp][j] = acc[pp][j] / w;
                    }
                }
            }
        }
    }

    if constexpr (REGIONS) {
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
    }

    if constexpr (SHIFT) {
        using Raw = typename RawOf<T>::type;
        if constexpr (!REGIONS) {
            yc = onto(y + P.shift_y, P.H);
            xd = onto(x0 + P.shift_x, P.W);
            uncut = nvalid == 4 && xd + 3 < P.W;
        }
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) {
            Raw* drow = reinterpret_cast<Raw*>(P.out) + ((size_t)(p0 + pp) * P.H + yc) * P.W;
            if (uncut) {
                raw4_u<Raw> o;
#pragma unroll
                for (int j = 0; j < 4; ++j) o.v[j] = raw_bits<T>(acc[pp][j]);
                *reinterpret_cast<raw4_u<Raw>*>(drow + xd) = o;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (j >= nvalid) continue;
                    const int xj = REGIONS ? xc[j] : onto(xd + j, P.W);       // SHIFT alone forms the columns here, where the seam cut the quad
                    drow[xj] = raw_bits<T>(acc[pp][j]);
                }
            }
        }
        return;
    }

#pragma unroll
    for (int pp = 0; pp < PP; ++pp) {
        const size_t off = ((size_t)(p0 + pp) * P.H + y) * P.W + x0;
        if constexpr (SPARSE) {
            using R = typename RawOf<T>::type;
            R* dst = reinterpret_cast<R*>(P.out) + off;
            const R* fill = reinterpret_cast<const R*>(P.fill) + off;
            if (nvalid == 4 && (all_live || !any_live)) {      // four elements, one source: one load (fill only) and one store
                raw4_u<R> o;
                if (all_live) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) o.v[j] = raw_bits<T>(acc[pp][j]);
                } else {
                    o = *reinterpret_cast<const raw4_u<R>*>(fill);
                }
                *reinterpret_cast<raw4_u<R>*>(dst) = o;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nvalid) dst[j] = live[j] ? raw_bits<T>(acc[pp][j]) : fill[j];
            }
        } else {
            T* dst = reinterpret_cast<T*>(P.out) + off;
            if (nvalid == 4) store4<T>(dst, acc[pp]);
            else {
                dst[0] = from_f32<T>(acc[pp][0]);
                if (nvalid > 1) dst[1] = from_f32<T>(acc[pp][1]);
                if (nvalid > 2) dst[2] = from_f32<T>(acc[pp][2]);
            }
        }
    }
}

template <typename T, int PP, bool SPARSE, bool SHIFT, bool REGIONS>
auto walk_blend_kernel(int method) {
    return method == MDTILE_METHOD_MD ? k_walk_blend<T, MDTILE_METHOD_MD, PP, SPARSE, SHIFT, REGIONS> : k_walk_blend<T, MDTILE_METHOD_MOD, PP, SPARSE, SHIFT, REGIONS>;
}

// one launch shape for every form; with REGIONS PP is sized as without: whether another size pays with the region tail behind the walk is not
// measured
template <typename T, bool SPARSE, bool SHIFT, bool REGIONS = false>
void launch_walk_blend(const WalkBlendArgs<SHIFT, REGIONS>& P, int method, hipStream_t s) {
    const int planes = P.N * P.C, pp = planes_per_thread(P.W, P.H, planes);
    const auto k = pp == 4 ? walk_blend_kernel<T, 4, SPARSE, SHIFT, REGIONS>(method) : pp == 2 ? walk_blend_kernel<T, 2, SPARSE, SHIFT, REGIONS>(method)
                                                                                       : walk_blend_kernel<T, 1, SPARSE, SHIFT, REGIONS>(method);
    hipLaunchKernelGGL(k, dim3(cdiv((long long)P.H * ((P.W + 3) / 4), 256), planes / pp), dim3(256), 0, s, P);
}

}  // namespace

int mdt::wrap_weight_map(const mdtile_plan* p, const float* d_tile_w, float* d_weights, hipStream_t s) {
    if (int rc = plan_upload(p)) return rc;
    const int n = p->w * p->h;
    hipLaunchKernelGGL(k_wrap_weight_grid, dim3(cdiv(n, 256)), dim3(256), 0, s, p->w, p->h, p->tw, p->cols, p->rows, p->d_xs, p->d_ys, p->d_colrange,
                       p->d_rowrange, d_tile_w, d_weights);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

int mdt::gather_check(const mdtile_plan* p, int dtype, int N, int C, const void* d_x_in, void* const* ptrs) {
    MDT_CHECK_ARG(p && d_x_in && ptrs, "mdtile_gather: null argument");
    MDT_CHECK_ARG(N > 0 && C > 0 && N * C <= 65535, "mdtile_gather: bad N=%d C=%d", N, C);
    MDT_CHECK_ARG(dtype >= 0 && dtype <= 2, "mdtile_gather: bad dtype %d", dtype);
    return MDTILE_OK;
}

// positions [s_lo, s_hi) -- tiles of a wrap-around plan, active slots of a sparse one -- into the plan's batch buffers ptrs[0 .. nptrs) (holes
// are fine: only the batches of those positions are touched)
// shift: null, or {shift_x, shift_y} of mdtile_gather_all_shift (checked there) -> the SHIFT kernels
int mdt::walk_gather(const mdtile_plan* p, int dtype, int N, int C, const void* d_x_in, void* const* ptrs, int nptrs, int s_lo, int s_hi, hipStream_t s,
                     const int* shift) {
    if (int rc = gather_check(p, dtype, N, C, d_x_in, ptrs)) return rc;
    const bool sparse = plan_sparse(p);
    const char* kind = sparse ? "sparse" : wrap_kind(p);
    MDT_CHECK_ARG(s_lo >= 0 && s_hi <= plan_tiles(p) && s_lo < s_hi && s_hi - s_lo <= 65535,
                  sparse ? "mdtile_gather: bad range [%d,%d) of %d active tiles" : "mdtile_gather: bad tile range [%d,%d) of %d", s_lo, s_hi, plan_tiles(p));
    MDT_CHECK_ARG(nptrs == p->num_batches, "mdtile_gather: %d batches given, the %s plan has %d", nptrs, kind, p->num_batches);
    if (nptrs > MDTILE_MAX_BATCHES) {      // a wrap-around plan only: mdtile_plan_create_subset makes no sparse plan of that many batches
        set_error("mdtile_gather: %d batches > MDTILE_MAX_BATCHES=%d (a %s plan has no packed form)", nptrs, MDTILE_MAX_BATCHES, kind);
        return MDTILE_E_LIMIT;
    }
    for (int q = s_lo; q < s_hi; ++q) MDT_CHECK_ARG(ptrs[q / p->tile_bs], "mdtile_gather: null batch pointer %d", q / p->tile_bs);
    if (int rc = plan_upload(p)) return rc;
    WrapGatherShiftParams P;
    memset(&P, 0, sizeof(P));
    P.W = p->w; P.H = p->h; P.tw = p->tw; P.th = p->th; P.cols = p->cols; P.tile_bs = p->tile_bs; P.N = N; P.C = C;
    P.s_lo = s_lo; P.xs = p->d_xs; P.ys = p->d_ys; P.active = sparse ? p->d_active : nullptr; P.x_in = d_x_in;
    for (int b = 0; b < nptrs; ++b) P.batch[b] = ptrs[b];
    dim3 grid(cdiv((long long)p->th * ((p->tw + 3) / 4), 256), N * C, s_hi - s_lo), block(256);
    if (shift) {
        P.shift_x = shift[0]; P.shift_y = shift[1];
        with_dtype(dtype, [&](auto* tag) { hipLaunchKernelGGL((k_wrap_gather<std::remove_pointer_t<decltype(tag)>, true>), grid, block, 0, s, P); });
    } else {
        const WrapGatherParams& P0 = P;
        with_dtype(dtype, [&](auto* tag) { hipLaunchKernelGGL((k_wrap_gather<std::remove_pointer_t<decltype(tag)>, false>), grid, block, 0, s, P0); });
    }
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

// The grid blend that takes no regions, flags or row bands: mdtile_blend on a wrap-around plan (d_fill null) and mdtile_blend_sparse (the caller
// has checked that the plan is sparse).  The texts name the entry point and the kind of plan.
// shift: null, or {shift_x, shift_y} of mdtile_blend_shift (checked there; never a sparse plan) -> the SHIFT kernels
int mdt::walk_blend(const mdtile_plan* p, const mdtile_blend_args* a, const void* const* batch_out, int num_batches, int num_regions, const void* d_fill,
                    hipStream_t s, const int* shift) {
    const bool sparse = plan_sparse(p);
    const char* fn = sparse ? "mdtile_blend_sparse" : shift ? "mdtile_blend_shift" : "mdtile_blend";
    const char* kind = sparse ? "sparse" : wrap_kind(p);
    const char* what = sparse ? "tile skipping" : "wrap-around";
    const char* whose = sparse ? " (the parent's map)" : "";
    MDT_CHECK_ARG(a, "%s: null plan/args", fn);
    // what this form does not do, by name
    MDT_CHECK_ARG(num_regions == 0, "%s: a %s plan takes no custom regions (%d given): %s is not combined with regions", fn, kind, num_regions, what);
    MDT_CHECK_ARG(a->flags == 0, "%s: a %s plan takes no MDTILE_BLEND_* flags (flags=%d): no partial sums, tile range or packed buffer", fn, kind, a->flags);
    MDT_CHECK_ARG(a->row_lo == 0 && a->row_hi == 0, "%s: a %s plan takes no row band [%d,%d): %s is not combined with the multi-GPU path", fn, kind, a->row_lo,
                  a->row_hi, what);
    MDT_CHECK_ARG(a->N > 0 && a->C > 0 && a->N * a->C <= 65535, "%s: bad N=%d C=%d", fn, a->N, a->C);
    MDT_CHECK_ARG(a->method == MDTILE_METHOD_MD || a->method == MDTILE_METHOD_MOD, "%s: bad method %d", fn, a->method);
    MDT_CHECK_ARG(a->dtype >= 0 && a->dtype <= 2, "%s: bad dtype %d", fn, a->dtype);
    MDT_CHECK_ARG(a->d_x_out, "%s: null output", fn);
    MDT_CHECK_ARG(!sparse || d_fill, "%s: null fill: the pixels no active tile decides need a value", fn);
    MDT_CHECK_ARG(batch_out && num_batches == p->num_batches, "%s: %d batches given, the %s plan has %d", fn, num_batches, kind, p->num_batches);
    if (num_batches > MDTILE_MAX_BATCHES) {      // a wrap-around plan only: mdtile_plan_create_subset makes no sparse plan of that many batches
        set_error("%s: %d batches > MDTILE_MAX_BATCHES=%d (a %s plan has no packed form: raise the tile batch size)", fn, num_batches, MDTILE_MAX_BATCHES, kind);
        return MDTILE_E_LIMIT;
    }
    if (a->method == MDTILE_METHOD_MD) MDT_CHECK_ARG(a->d_weights, "%s: MultiDiffusion needs d_weights%s", fn, whose);
    else MDT_CHECK_ARG(a->d_tile_w && a->d_rescale, "%s: Mixture of Diffusers needs d_tile_w and d_rescale%s", fn, whose);
    for (int b = 0; b < num_batches; ++b) MDT_CHECK_ARG(batch_out[b], "%s: null batch pointer %d", fn, b);
    if (int rc = plan_upload(p)) return rc;
    WalkBlendShiftParams P;
    memset(&P, 0, sizeof(P));
    P.W = p->w; P.H = p->h; P.tw = p->tw; P.th = p->th; P.cols = p->cols; P.rows = p->rows; P.tile_bs = p->tile_bs; P.N = a->N; P.C = a->C;
    P.xs = p->d_xs; P.ys = p->d_ys; P.colquad = p->d_colquad; P.rowinfo = p->d_rowinfo;
    P.weights = a->d_weights; P.tile_w = a->d_tile_w; P.rescale = a->d_rescale; P.out = a->d_x_out;
    if (sparse) { P.slot = p->d_slot; P.fill = d_fill; }
    for (int b = 0; b < num_batches; ++b) P.batch[b] = batch_out[b];
    with_dtype(a->dtype, [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        if (shift) {
            P.shift_x = shift[0]; P.shift_y = shift[1];
            launch_walk_blend<T, false, true>(P, a->method, s);
        } else if (sparse) {
            launch_walk_blend<T, true, false>(P, a->method, s);
        } else {
            launch_walk_blend<T, false, false>(P, a->method, s);
        }
    });
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

// mdtile_blend_wrap_regions (wrap_regions.hip, which has checked every argument and counted the foreground regions) -> the REGIONS kernels
int mdt::walk_blend_regions(const mdtile_plan* p, const mdtile_blend_args* a, const void* const* batch_out, int num_batches, const mdtile_wrap_regions* wr,
                            int num_fg, hipStream_t s) {
    if (int rc = plan_upload(p)) return rc;
    WrapRegionsParams P;
    memset(&P, 0, sizeof(P));
    P.W = p->w; P.H = p->h; P.tw = p->tw; P.th = p->th; P.cols = p->cols; P.rows = p->rows; P.tile_bs = p->tile_bs; P.N = a->N; P.C = a->C;
    P.num_batches = num_batches; P.num_regions = wr->num_regions; P.num_fg = num_fg; P.shift_x = wr->sx; P.shift_y = wr->sy;
    P.xs = p->d_xs; P.ys = p->d_ys; P.colquad = p->d_colquad; P.rowinfo = p->d_rowinfo;
    P.grid_w = wr->d_grid_w; P.region_w = wr->d_region_w; P.tile_w = a->d_tile_w; P.out = a->d_x_out;
    for (int k = 0; k < wr->num_regions; ++k) P.regions[k] = wr->regions[k];
    for (int b = 0; b < num_batches; ++b) P.batch[b] = batch_out[b];
    with_dtype(a->dtype, [&](auto* tag) { launch_walk_blend<std::remove_pointer_t<decltype(tag)>, false, true, true>(P, a->method, s); });
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

// what both shifted entry points ask of the plan and the shift before anything else is looked at
int mdt::shift_check(const char* fn, const mdtile_plan* p, int sx, int sy) {
    MDT_CHECK_ARG(p, "%s: null plan", fn);
    MDT_CHECK_ARG(!plan_sparse(p), "%s: refused on a sparse plan: the grid shift is not combined with tile skipping", fn);
    MDT_CHECK_ARG(plan_wraps(p), "%s: refused on a plain plan: only a wrap-around plan (mdtile_plan_create_wrap) has a circle to shift the grid on", fn);
    MDT_CHECK_ARG(sx >= 0 && sx < p->w && sy >= 0 && sy < p->h, "%s: shift (%d, %d) out of range: 0 <= sx < %d and 0 <= sy < %d", fn, sx, sy, p->w, p->h);
    MDT_CHECK_ARG(sx == 0 || p->wrap_x, "%s: sx = %d on a %s plan: the x axis does not wrap", fn, sx, wrap_kind(p));
    MDT_CHECK_ARG(sy == 0 || p->wrap_y, "%s: sy = %d on a %s plan: the y axis does not wrap", fn, sy, wrap_kind(p));
    return MDTILE_OK;
}

extern "C" int mdtile_gather_all_shift(const mdtile_plan* p, int dtype, int N, int C, const void* d_x_in, void* const* batch_ptrs, int num_batches, int sx,
                                       int sy, mdtile_stream_t stream) {
    if (int rc = shift_check("mdtile_gather_all_shift", p, sx, sy)) return rc;
    MDT_CHECK_ARG(batch_ptrs, "mdtile_gather_all_shift: null argument");
    MDT_CHECK_ARG(num_batches == p->num_batches, "mdtile_gather_all_shift: %d batches given, the %s plan has %d (it has no packed form)", num_batches,
                  wrap_kind(p), p->num_batches);
    const int shift[2] = {sx, sy};
    return walk_gather(p, dtype, N, C, d_x_in, batch_ptrs, num_batches, 0, plan_tiles(p), as_stream(stream), shift);
}

extern "C" int mdtile_blend_shift(const mdtile_plan* p, const mdtile_blend_args* args, const void* const* batch_out, int num_batches, int sx, int sy,
                                  mdtile_stream_t stream) {
    if (int rc = shift_check("mdtile_blend_shift", p, sx, sy)) return rc;
    const int shift[2] = {sx, sy};
    return walk_blend(p, args, batch_out, num_batches, 0, nullptr, as_stream(stream), shift);
}
