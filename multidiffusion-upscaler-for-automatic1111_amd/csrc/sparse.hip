// Tile skipping for img2img inpainting: which grid tiles an inpaint mask touches, the gather of those tiles into compact
// batches, and the overlap blend of their model outputs for a SPARSE plan (mdtile_plan_create_subset) -- the parent's geometry and covering
// tables plus slot[T] (rank of a tile among the active ones, ascending tile index, or -1) and active[Ta].
//
// The blend is the gather of blend.hip / wrap.hip -- one thread owns a quad of a row for one or more planes and walks the parent's covering tile
// rows x tile columns in ASCENDING tile index (rows outer, columns inner) -- with one thing added: a tile that is not active has no output.  A
// pixel is LIVE iff every grid tile of the parent that covers it is active.  At a live pixel the sum runs over the same terms in the same order
// as mdtile_blend's on the parent plan (fp32 accumulation from +0.0, -ffp-contract=off, Mixture of Diffusers term out * (tile_w * rescale[y, x]),
// MultiDiffusion epilogue weights > 1 ? buf / weights : buf with the PARENT's full maps, rounded once): bit-identical.  At any other pixel the
// output is the bit pattern of fill[n, c, y, x] -- copied as integers, so NaN payloads and -0.0 survive in every dtype -- and no tile output is
// read for it: liveness is decided from the slot table before the first tile value is loaded.
//
// Not here (refused with an error that names the reason): custom regions, MDTILE_BLEND_* flags, row bands, wrap-around parents,
// mdtile_gather_range, mdtile_blend / mdtile_blend_finalize / mdtile_blend_dispatch and mdtile_weight_map_add_grid on a sparse plan.
#include "launchers.h"

using namespace mdt;

namespace {

// ---- activity: active[t] = some element of mask[:, y_t : y_t + th, x_t : x_t + tw] is not equal to zero --------------------------------------
// One block per tile.  A lane ORs `!(v == 0.0f)` over its quads (NaN, denormals, negatives and fractions count; +0.0 and -0.0 do not), a wave
// reduces by ballot, the four waves meet in LDS and lane 0 of wave 0 stores the flag: every entry is written by exactly one plain store, the
// array needs no clearing and nothing is atomic.
__global__ __launch_bounds__(256) void k_tile_activity(int W, int H, int tw, int th, int cols, int planes, const int* __restrict__ xs,
                                                       const int* __restrict__ ys, const float* __restrict__ mask, int* __restrict__ active) {
    __shared__ int s_any[4];
    const int t = blockIdx.x;
    const int r = t / cols, c = t - r * cols;
    const int x0 = xs[c], y0 = ys[r];                       // a plain tile never passes the edge: x0 + tw <= W, y0 + th <= H
    const int tw4 = (tw + 3) >> 2;
    const int per_plane = tw4 * th;
    const long long total = (long long)per_plane * planes;
    bool any = false;
    for (long long q = threadIdx.x; q < total; q += 256) {
        const int plane = (int)(q / per_plane), rem = (int)(q - (long long)plane * per_plane);
        const int ty = rem / tw4, tx = (rem - ty * tw4) << 2;
        const float* src = mask + ((size_t)plane * H + y0 + ty) * W + x0 + tx;
        if (tx + 3 < tw) {
            float v[4];
            load4<float>(src, v);
            any = any || !(v[0] == 0.0f) || !(v[1] == 0.0f) || !(v[2] == 0.0f) || !(v[3] == 0.0f);
        } else {
            for (int j = 0; tx + j < tw; ++j) any = any || !(src[j] == 0.0f);
        }
    }
    const bool wave_any = __ballot(any) != 0;
    if ((threadIdx.x & 63) == 0) s_any[threadIdx.x >> 6] = wave_any ? 1 : 0;
    __syncthreads();
    if (threadIdx.x == 0) active[t] = (s_any[0] | s_any[1] | s_any[2] | s_any[3]) ? 1 : 0;
}

// ---- gather of the active tiles ----------------------------------------------------------------------------------------------------------------
struct SparseGatherParams {
    int W, H, tw, th, cols, tile_bs, N, C;
    int s_lo, _pad;
    const int *xs, *ys, *active;
    const void* x_in;
    void* batch[MDTILE_MAX_BATCHES];
};
static_assert(sizeof(SparseGatherParams) <= 4096, "kernel argument block must stay under 4 KiB");

// active tile number s (its slot) = tile t = active[s]: x_tile[(s mod tile_bs) N + n, c, ty, tx] of batch s / tile_bs = x_in[n, c, y_t + ty, x_t + tx].
// grid: x = quads over (th rows x tw4), y = plane (n*C + c), z = slot
template <typename T>
__global__ __launch_bounds__(256) void k_sparse_gather(const SparseGatherParams P) {
    const int tw4 = (P.tw + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= tw4 * P.th) return;
    const int ty = idx / tw4, tx0 = (idx - ty * tw4) << 2;
    const int plane = blockIdx.y, n = plane / P.C, c = plane - n * P.C;
    const int s = P.s_lo + blockIdx.z;
    const int t = P.active[s];
    const int r = t / P.cols, cc = t - r * P.cols;
    const T* src = reinterpret_cast<const T*>(P.x_in) + (((size_t)n * P.C + c) * P.H + P.ys[r] + ty) * P.W + P.xs[cc] + tx0;
    const int b = s / P.tile_bs, i = s - b * P.tile_bs;
    T* dst = reinterpret_cast<T*>(P.batch[b]) + (((size_t)i * P.N + n) * P.C + c) * ((size_t)P.th * P.tw) + (size_t)ty * P.tw + tx0;
    if (tx0 + 3 < P.tw) {
        float v[4];
        load4<T>(src, v);
        store4<T>(dst, v);
    } else {
        for (int j = 0; tx0 + j < P.tw; ++j) dst[j] = src[j];
    }
}

// ---- blend ---------------------------------------------------------------------------------------------------------------------------------------
struct SparseBlendParams {
    int W, H, tw, th, cols, tile_bs, N, C;
    const int *xs, *ys, *slot;
    const int4 *colquad, *rowinfo;
    const float *weights, *tile_w, *rescale;
    const void* fill;
    void* out;
    const void* batch[MDTILE_MAX_BATCHES];
};
static_assert(sizeof(SparseBlendParams) <= 4096, "kernel argument block must stay under 4 KiB");

// the storage type as an integer of its size: what passes `fill` through without a float conversion
template <typename T> struct RawOf { using type = unsigned short; };
template <> struct RawOf<float> { using type = unsigned int; };
template <typename R> struct __attribute__((packed, aligned(sizeof(R)))) raw4_u { R v[4]; };   // 4 elements at an element-aligned address

template <typename T> __device__ __forceinline__ typename RawOf<T>::type raw_bits(float v);
template <> __device__ __forceinline__ unsigned int raw_bits<float>(float v) { return __float_as_uint(v); }
template <> __device__ __forceinline__ unsigned short raw_bits<__half>(float v) { return __half_as_ushort(__float2half_rn(v)); }
template <> __device__ __forceinline__ unsigned short raw_bits<__hip_bfloat16>(float v) {
    const __hip_bfloat16 h = __float2bfloat16(v);
    unsigned short u;
    __builtin_memcpy(&u, &h, sizeof(u));
    return u;
}

// 4 consecutive elements at an address aligned to their total size (16 bytes of fp32, 8 bytes of a 16-bit type): one load instruction
template <typename T> __device__ __forceinline__ void load4_aligned(const T* p, float (&o)[4]);
template <> __device__ __forceinline__ void load4_aligned<float>(const float* p, float (&o)[4]) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
}
template <> __device__ __forceinline__ void load4_aligned<__half>(const __half* p, float (&o)[4]) {
    const ushort4 t = *reinterpret_cast<const ushort4*>(p);
    o[0] = __half2float(__ushort_as_half(t.x)); o[1] = __half2float(__ushort_as_half(t.y));
    o[2] = __half2float(__ushort_as_half(t.z)); o[3] = __half2float(__ushort_as_half(t.w));
}
template <> __device__ __forceinline__ void load4_aligned<__hip_bfloat16>(const __hip_bfloat16* p, float (&o)[4]) {
    const ushort4 t = *reinterpret_cast<const ushort4*>(p);
    o[0] = __uint_as_float((unsigned)t.x << 16); o[1] = __uint_as_float((unsigned)t.y << 16);
    o[2] = __uint_as_float((unsigned)t.z << 16); o[3] = __uint_as_float((unsigned)t.w << 16);
}

// One thread owns one quad (4 consecutive canvas columns of one row) for PP planes.  The tile rows that cover the canvas row are the run
// rowinfo[y].x and the tile columns that cover ANY pixel of the quad the run colquad[xq].x, both of the parent (first | count << 16, plain runs).
// Pass 1 reads only the slot table: pixel j is live iff no covering tile has slot < 0.  Pass 2 walks the same tiles in the same order and adds,
// for an active tile, the pixels that are covered AND live: one vector load per plane when the quad is one aligned piece of the tile row and
// all four pixels are live, per-element loads of exactly those pixels otherwise.
template <typename T, int METHOD, int PP>
__global__ __launch_bounds__(256) void k_sparse_blend(const SparseBlendParams P) {
    using R = typename RawOf<T>::type;
    const int W4 = (P.W + 3) >> 2;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= W4 * P.H) return;
    const int y = idx / W4, xq = idx - y * W4;
    const int x0 = xq << 2;
    const int p0 = blockIdx.y * PP;                        // the host guarantees N*C % PP == 0
    const int nvalid = P.W - x0 < 4 ? P.W - x0 : 4;
    const size_t tile_elems = (size_t)P.th * P.tw;

    const int cpack = P.colquad[xq].x, rpack = P.rowinfo[y].x;
    const int c_first = cpack & 0xffff, c_count = cpack >> 16;
    const int r_first = rpack & 0xffff, r_count = rpack >> 16;

    // pass 1: liveness, from the slot table alone
    bool live[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) live[j] = j < nvalid;
    for (int kr = 0; kr < r_count; ++kr) {
        const int r = r_first + kr;
        for (int k = 0; k < c_count; ++k) {
            const int c = c_first + k;
            if (P.slot[r * P.cols + c] >= 0) continue;
            const int tx = x0 - P.xs[c];                   // may be negative: the column covers a later pixel of the quad only
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (tx + j >= 0 && tx + j < P.tw) live[j] = false;
        }
    }
    const bool all_live = live[0] && live[1] && live[2] && live[3];
    const bool any_live = live[0] || live[1] || live[2] || live[3];

    float acc[PP][4];
#pragma unroll
    for (int pp = 0; pp < PP; ++pp)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[pp][j] = 0.f;

    if (any_live) {
        float resc[4] = {0.f, 0.f, 0.f, 0.f};
        if (METHOD == MDTILE_METHOD_MOD) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (live[j]) resc[j] = P.rescale[(size_t)y * P.W + x0 + j];
        }

        // pass 2: ascending tile index, rows outer, columns inner
        for (int kr = 0; kr < r_count; ++kr) {
            const int r = r_first + kr;
            const int ty = y - P.ys[r];                    // in [0, th): rowinfo holds exactly the rows that cover y
            const size_t roff = (size_t)ty * P.tw;         // the tile row inside a [th, tw] plane (and inside the tile-weight map)
            for (int k = 0; k < c_count; ++k) {
                const int c = c_first + k;
                const int s = P.slot[r * P.cols + c];
                if (s < 0) continue;                       // no pixel it covers is live
                const int b = s / P.tile_bs, i = s - b * P.tile_bs;
                const int tx = x0 - P.xs[c];
                const T* row = reinterpret_cast<const T*>(P.batch[b]) + ((size_t)i * P.N * P.C + p0) * tile_elems + roff;
                // one contiguous piece of the tile row, every pixel live, at an address aligned for the vector load in this plane and
                // (tile_elems % 4 == 0) in the others
                const bool whole = all_live && tx >= 0 && tx + 3 < P.tw;
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
                        const int txj = tx + j;
                        if (!live[j] || txj < 0 || txj >= P.tw) continue;
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

        // MD normalisation: x = where(weights > 1, buf / weights, buf), the parent's full weight map
        if (METHOD == MDTILE_METHOD_MD) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (!live[j]) continue;
                const float w = P.weights[(size_t)y * P.W + x0 + j];
                if (w > 1.0f) {
#pragma unroll
                    for (int pp = 0; pp < PP; ++pp) acc[pp][j] = acc[pp][j] / w;
                }
            }
        }
    }

#pragma unroll
    for (int pp = 0; pp < PP; ++pp) {
        const size_t off = ((size_t)(p0 + pp) * P.H + y) * P.W + x0;
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
    }
}

template <typename T, int PP>
void launch_sparse_blend(const SparseBlendParams& P, int method, hipStream_t s) {
    dim3 grid(cdiv((long long)P.H * ((P.W + 3) / 4), 256), (P.N * P.C) / PP), block(256);
    if (method == MDTILE_METHOD_MD) hipLaunchKernelGGL((k_sparse_blend<T, MDTILE_METHOD_MD, PP>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((k_sparse_blend<T, MDTILE_METHOD_MOD, PP>), grid, block, 0, s, P);
}

template <typename T>
void launch_sparse_blend_planes(const SparseBlendParams& P, int method, hipStream_t s) {
    // planes per thread: 4 while that leaves >= ~128k threads (2 per lane of the chip) and divides N*C, as blend.hip sizes k_blend
    const int planes = P.N * P.C;
    const long long work = (long long)P.H * ((P.W + 3) / 4) * planes;
    if (planes % 4 == 0 && work / 4 >= 131072) launch_sparse_blend<T, 4>(P, method, s);
    else if (planes % 2 == 0 && work / 2 >= 131072) launch_sparse_blend<T, 2>(P, method, s);
    else launch_sparse_blend<T, 1>(P, method, s);
}

}  // namespace

extern "C" int mdtile_tile_activity(const mdtile_plan* p, const float* d_mask, int planes, int* d_active, mdtile_stream_t stream) {
    MDT_CHECK_ARG(p && d_mask && d_active, "mdtile_tile_activity: null argument");
    MDT_CHECK_ARG(!plan_wraps(p), "mdtile_tile_activity: refused on a %s plan: tile skipping is not combined with wrap-around", wrap_kind(p));
    MDT_CHECK_ARG(!plan_sparse(p), "mdtile_tile_activity: refused on a sparse plan: the activity is asked of the full plan");
    MDT_CHECK_ARG(planes > 0 && planes <= 65535, "mdtile_tile_activity: bad planes=%d", planes);
    if (int rc = plan_upload(p)) return rc;
    hipLaunchKernelGGL(k_tile_activity, dim3(p->T), dim3(256), 0, as_stream(stream), p->w, p->h, p->tw, p->th, p->cols, planes, p->d_xs, p->d_ys, d_mask,
                       d_active);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

// the active slots [s_lo, s_hi) into the plan's compact batch buffers ptrs[0 .. nptrs) (holes are fine: only the batches of those slots are touched)
int mdt::sparse_gather(const mdtile_plan* p, int dtype, int N, int C, const void* d_x_in, void* const* ptrs, int nptrs, int s_lo, int s_hi, hipStream_t s) {
    MDT_CHECK_ARG(p && d_x_in && ptrs, "mdtile_gather: null argument");
    MDT_CHECK_ARG(N > 0 && C > 0 && N * C <= 65535, "mdtile_gather: bad N=%d C=%d", N, C);
    MDT_CHECK_ARG(dtype >= 0 && dtype <= 2, "mdtile_gather: bad dtype %d", dtype);
    MDT_CHECK_ARG(s_lo >= 0 && s_hi <= p->Ta && s_lo < s_hi && s_hi - s_lo <= 65535, "mdtile_gather: bad range [%d,%d) of %d active tiles", s_lo, s_hi, p->Ta);
    MDT_CHECK_ARG(nptrs == p->num_batches && nptrs <= MDTILE_MAX_BATCHES, "mdtile_gather: %d batches given, the sparse plan has %d", nptrs, p->num_batches);
    for (int q = s_lo; q < s_hi; ++q) MDT_CHECK_ARG(ptrs[q / p->tile_bs], "mdtile_gather: null batch pointer %d", q / p->tile_bs);
    if (int rc = plan_upload(p)) return rc;
    SparseGatherParams P;
    memset(&P, 0, sizeof(P));
    P.W = p->w; P.H = p->h; P.tw = p->tw; P.th = p->th; P.cols = p->cols; P.tile_bs = p->tile_bs; P.N = N; P.C = C;
    P.s_lo = s_lo; P.xs = p->d_xs; P.ys = p->d_ys; P.active = p->d_active; P.x_in = d_x_in;
    for (int b = 0; b < nptrs; ++b) P.batch[b] = ptrs[b];
    dim3 grid(cdiv((long long)p->th * ((p->tw + 3) / 4), 256), N * C, s_hi - s_lo), block(256);
    switch (dtype) {
        case MDTILE_DT_F32: hipLaunchKernelGGL(k_sparse_gather<float>, grid, block, 0, s, P); break;
        case MDTILE_DT_F16: hipLaunchKernelGGL(k_sparse_gather<__half>, grid, block, 0, s, P); break;
        default: hipLaunchKernelGGL(k_sparse_gather<__hip_bfloat16>, grid, block, 0, s, P); break;
    }
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_blend_sparse(const mdtile_plan* p, const mdtile_blend_args* a, const void* const* batch_out, int num_batches, const void* d_fill,
                                   mdtile_stream_t stream) {
    MDT_CHECK_ARG(p && a, "mdtile_blend_sparse: null plan/args");
    MDT_CHECK_ARG(plan_sparse(p), "mdtile_blend_sparse: not a sparse plan (mdtile_plan_create_subset): the blend of a full plan is mdtile_blend");
    // what this form does not do, by name
    MDT_CHECK_ARG(a->flags == 0, "mdtile_blend_sparse: a sparse plan takes no MDTILE_BLEND_* flags (flags=%d): no partial sums, tile range or packed buffer",
                  a->flags);
    MDT_CHECK_ARG(a->row_lo == 0 && a->row_hi == 0, "mdtile_blend_sparse: a sparse plan takes no row band [%d,%d): tile skipping is not combined with the multi-GPU path",
                  a->row_lo, a->row_hi);
    MDT_CHECK_ARG(a->N > 0 && a->C > 0 && a->N * a->C <= 65535, "mdtile_blend_sparse: bad N=%d C=%d", a->N, a->C);
    MDT_CHECK_ARG(a->method == MDTILE_METHOD_MD || a->method == MDTILE_METHOD_MOD, "mdtile_blend_sparse: bad method %d", a->method);
    MDT_CHECK_ARG(a->dtype >= 0 && a->dtype <= 2, "mdtile_blend_sparse: bad dtype %d", a->dtype);
    MDT_CHECK_ARG(a->d_x_out, "mdtile_blend_sparse: null output");
    MDT_CHECK_ARG(d_fill, "mdtile_blend_sparse: null fill: the pixels no active tile decides need a value");
    MDT_CHECK_ARG(batch_out && num_batches == p->num_batches && num_batches <= MDTILE_MAX_BATCHES, "mdtile_blend_sparse: %d batches given, the sparse plan has %d",
                  num_batches, p->num_batches);
    if (a->method == MDTILE_METHOD_MD) MDT_CHECK_ARG(a->d_weights, "mdtile_blend_sparse: MultiDiffusion needs d_weights (the parent's map)");
    else MDT_CHECK_ARG(a->d_tile_w && a->d_rescale, "mdtile_blend_sparse: Mixture of Diffusers needs d_tile_w and d_rescale (the parent's map)");
    for (int b = 0; b < num_batches; ++b) MDT_CHECK_ARG(batch_out[b], "mdtile_blend_sparse: null batch pointer %d", b);
    if (int rc = plan_upload(p)) return rc;
    SparseBlendParams P;
    memset(&P, 0, sizeof(P));
    P.W = p->w; P.H = p->h; P.tw = p->tw; P.th = p->th; P.cols = p->cols; P.tile_bs = p->tile_bs; P.N = a->N; P.C = a->C;
    P.xs = p->d_xs; P.ys = p->d_ys; P.slot = p->d_slot; P.colquad = p->d_colquad; P.rowinfo = p->d_rowinfo;
    P.weights = a->d_weights; P.tile_w = a->d_tile_w; P.rescale = a->d_rescale; P.fill = d_fill; P.out = a->d_x_out;
    for (int b = 0; b < num_batches; ++b) P.batch[b] = batch_out[b];
    hipStream_t s = as_stream(stream);
    switch (a->dtype) {
        case MDTILE_DT_F32: launch_sparse_blend_planes<float>(P, a->method, s); break;
        case MDTILE_DT_F16: launch_sparse_blend_planes<__half>(P, a->method, s); break;
        default: launch_sparse_blend_planes<__hip_bfloat16>(P, a->method, s); break;
    }
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}
