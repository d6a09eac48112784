// What the kernels of the jittered grid (lattice.hip: k_lattice_weight, k_lattice_gather, k_lattice_blend) are written on: the axis as the kernels
// see it, their argument blocks, the covering range and the weight sum of a pixel from the lattice integers, and the host checks of a caller's
// mdtile_lattice.  The raw 4-element store and the planes-per-thread rule are walk.h's.
#pragma once
#include "launchers.h"
#include "walk.h"

namespace {

using namespace mdt;

// one axis as the kernels see it
struct LatAxis {
    int extent, tile;
    int stride, off, K;       // off = s - stride in (-stride, 0]; an axis that does not move: stride 1, off 0, K 0
};

struct LatticeParams {
    LatAxis ax, ay;
    int cols, tile_bs, N, C;
};
struct LatticeBlendParams : LatticeParams {
    const float* tile_w;      // Mixture of Diffusers: the [th, tw] Gaussian; null for MultiDiffusion
    void* out;
    const void* batch[MDTILE_MAX_BATCHES];
};
static_assert(sizeof(LatticeBlendParams) <= 4096, "kernel argument block must stay under 4 KiB");
// with custom regions (mdtile_blend_lattice_regions)
struct LatticeRegionsParams : LatticeBlendParams {
    int num_regions, num_fg;
    const float* region_w;    // [H, W] on the canvas; null iff the list holds no background region
    mdtile_region regions[MDTILE_MAX_REGIONS];
};
static_assert(sizeof(LatticeRegionsParams) <= 4096, "kernel argument block must stay under 4 KiB");
// with tile skipping (mdtile_blend_lattice_sparse): tile_bs is the COMPACT batches', `batch` holds those
struct LatticeSparseParams : LatticeBlendParams {
    const int* slot;          // slot[t] = place of tile t in the compact batches; anything outside [0, num_active) = the tile is not active
    const void* fill;         // [N, C, H, W] in the storage type: the value of every pixel that is not live
    int num_active;
};
static_assert(sizeof(LatticeSparseParams) <= 4096, "kernel argument block must stay under 4 KiB");

// floor(a / b), b > 0 (C's `/` truncates towards zero: wrong for the negative numerators left of the first stride)
__host__ __device__ __forceinline__ int floor_div(int a, int b) {
    const int q = a / b;
    return a - q * b < 0 ? q - 1 : q;
}
__host__ __device__ __forceinline__ int lat_origin(const LatAxis& a, int k) { return a.off + k * a.stride; }
__host__ __device__ __forceinline__ int lat_pushed(const LatAxis& a, int k) {
    const int u = lat_origin(a, k), last = a.extent - a.tile;
    return u < 0 ? 0 : u > last ? last : u;
}
// the tiles whose lattice box meets the coordinates [p_lo, p_hi] (p_lo <= p_hi, both on the canvas): lo .. hi, never empty
struct Cover { int lo, hi; };
__device__ __forceinline__ Cover lat_cover(const LatAxis& a, int p_lo, int p_hi) {
    Cover c;
    c.lo = floor_div(p_lo - a.tile - a.off, a.stride) + 1;
    if (c.lo < 0) c.lo = 0;
    c.hi = floor_div(p_hi - a.off, a.stride);
    if (c.hi > a.K) c.hi = a.K;
    return c;
}

// wsum of pixel (y, x): the candidates are the tile rows `rows` (all cover y) and the tile columns `cand` (a superset of those that cover x:
// the columns of x's quad); ascending tile index, fp32 from +0.0
template <bool MOD>
__device__ __forceinline__ float lat_wsum(const LatticeParams& P, int y, int x, Cover rows, Cover cand, const float* __restrict__ tile_w) {
    float s = 0.0f;
    for (int r = rows.lo; r <= rows.hi; ++r) {
        const int wy = y - lat_origin(P.ay, r);
        for (int c = cand.lo; c <= cand.hi; ++c) {
            const int d = x - lat_origin(P.ax, c);
            if (d < 0 || d >= P.ax.tile) continue;
            if (MOD) s += tile_w[wy * P.ax.tile + d];
            else s += 1.0f;
        }
    }
    return s;
}

// ---- host integers ---------------------------------------------------------------------------------------------------------------
// tiles of a moving axis at shift s: K + 1, K = ceil((extent - tile - (s - stride)) / stride)  (the numerator is positive: tile < extent, s <= stride)
int axis_tiles(int extent, int tile, int stride, int s) { return (extent - tile - (s - stride) + stride - 1) / stride + 1; }

LatAxis kernel_axis(int extent, int tile, int stride, int s, int count) {
    LatAxis a;
    a.extent = extent; a.tile = tile;
    if (tile >= extent) { a.stride = 1; a.off = 0; a.K = 0; }
    else { a.stride = stride; a.off = s - stride; a.K = count - 1; }
    return a;
}

// Is *lat what mdtile_lattice_make writes?  The struct is the caller's memory: every field the kernels' addresses depend on is checked again.
int lattice_check(const char* fn, const mdtile_lattice* l) {
    MDT_CHECK_ARG(l, "%s: null lattice", fn);
    MDT_CHECK_ARG(l->w > 0 && l->h > 0 && l->w <= 65535 && l->h <= 65535 && l->tile_w > 0 && l->tile_h > 0 && l->tile_w <= l->w && l->tile_h <= l->h &&
                      l->overlap >= 0 && l->tile_bs > 0,
                  "%s: bad lattice: canvas %dx%d, tile %dx%d, overlap %d, tile_bs %d (not from mdtile_lattice_make)", fn, l->w, l->h, l->tile_w, l->tile_h,
                  l->overlap, l->tile_bs);
    const int extent[2] = {l->w, l->h}, tile[2] = {l->tile_w, l->tile_h}, stride[2] = {l->stride_x, l->stride_y}, s[2] = {l->sx, l->sy},
              count[2] = {l->cols, l->rows};
    for (int a = 0; a < 2; ++a) {
        const char axis = a ? 'y' : 'x';
        if (tile[a] >= extent[a]) {
            MDT_CHECK_ARG(count[a] == 1, "%s: bad lattice: %d tiles along %c although the tile spans the canvas", fn, count[a], axis);
            continue;
        }
        MDT_CHECK_ARG(stride[a] == tile[a] - l->overlap && stride[a] > 0, "%s: bad lattice: stride_%c = %d, tile - overlap = %d", fn, axis, stride[a],
                      tile[a] - l->overlap);
        MDT_CHECK_ARG(s[a] >= 1 && s[a] <= stride[a], "%s: shift s%c = %d outside [1, %d] (the stride) on an axis that moves", fn, axis, s[a], stride[a]);
        MDT_CHECK_ARG(count[a] == axis_tiles(extent[a], tile[a], stride[a], s[a]), "%s: bad lattice: %d tiles along %c, the shift gives %d", fn, count[a], axis,
                      axis_tiles(extent[a], tile[a], stride[a], s[a]));
    }
    MDT_CHECK_ARG(l->cols <= 32767 && l->rows <= 32767 && l->num_tiles == l->cols * l->rows, "%s: bad lattice: %d tiles for %d x %d", fn, l->num_tiles, l->cols,
                  l->rows);
    MDT_CHECK_ARG(l->num_batches == (l->num_tiles + l->tile_bs - 1) / l->tile_bs && l->num_batches > 0 &&
                      l->tile_bs == (l->num_tiles + l->num_batches - 1) / l->num_batches,
                  "%s: bad lattice: %d batches of %d for %d tiles", fn, l->num_batches, l->tile_bs, l->num_tiles);
    return MDTILE_OK;
}

void fill_params(LatticeParams& P, const mdtile_lattice* l, int N, int C) {
    P.ax = kernel_axis(l->w, l->tile_w, l->stride_x, l->sx, l->cols);
    P.ay = kernel_axis(l->h, l->tile_h, l->stride_y, l->sy, l->rows);
    P.cols = l->cols; P.tile_bs = l->tile_bs; P.N = N; P.C = C;
}

// what both calls with batches ask of their count
int batches_check(const char* fn, const mdtile_lattice* l, int num_batches) {
    MDT_CHECK_ARG(num_batches == l->num_batches, "%s: %d batches given, the lattice has %d", fn, num_batches, l->num_batches);
    MDT_CHECK_ARG(num_batches <= MDTILE_MAX_BATCHES, "%s: %d batches > MDTILE_MAX_BATCHES=%d (the lattice has no packed form: raise the tile batch size)", fn,
                  num_batches, MDTILE_MAX_BATCHES);
    return MDTILE_OK;
}

// Is *sub what mdtile_lattice_subset_make writes?  The flags it was made from are not kept, so what can be checked is the lattice, the count and
// the batching rule on it; the slot table is the device's, and the kernels treat every entry outside [0, num_active) as "not active".
int subset_check(const char* fn, const mdtile_lattice_subset* sub) {
    MDT_CHECK_ARG(sub, "%s: null subset", fn);
    if (int rc = lattice_check(fn, &sub->lat)) return rc;
    MDT_CHECK_ARG(sub->num_active >= 1 && sub->num_active <= sub->lat.num_tiles, "%s: bad subset: num_active = %d outside [1, %d] (the lattice's tiles)", fn,
                  sub->num_active, sub->lat.num_tiles);
    MDT_CHECK_ARG(sub->num_batches > 0 && sub->tile_bs > 0 && sub->num_batches == (sub->num_active - 1) / sub->tile_bs + 1 &&
                      sub->tile_bs == (sub->num_active - 1) / sub->num_batches + 1,      // ceil without a sum that could pass INT_MAX
                  "%s: bad subset: %d batches of %d for %d active tiles (not the rule num_batches = ceil(Ta / tile_bs), tile_bs = ceil(Ta / num_batches))", fn,
                  sub->num_batches, sub->tile_bs, sub->num_active);
    MDT_CHECK_ARG(sub->d_slot, "%s: null d_slot: the blend and the gather find an active tile's place in the compact batches there", fn);
    return MDTILE_OK;
}

int subset_batches_check(const char* fn, const mdtile_lattice_subset* sub, int num_batches) {
    MDT_CHECK_ARG(num_batches == sub->num_batches, "%s: %d batches given, the subset has %d", fn, num_batches, sub->num_batches);
    MDT_CHECK_ARG(num_batches <= MDTILE_MAX_BATCHES, "%s: %d batches > MDTILE_MAX_BATCHES=%d (raise the tile batch size, or run the full lattice)", fn, num_batches,
                  MDTILE_MAX_BATCHES);
    return MDTILE_OK;
}

}  // namespace
