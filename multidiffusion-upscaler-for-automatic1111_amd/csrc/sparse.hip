// Tile skipping for img2img inpainting: which grid tiles an inpaint mask touches (the kernel here), and the entry point of the
// overlap blend of their model outputs for a SPARSE plan (mdtile_plan_create_subset) -- the parent's geometry and covering tables plus
// slot[T] (rank of a tile among the active ones, ascending tile index, or -1) and active[Ta].  The gather of the active tiles into compact
// batches and the blend run the kernels of wrap.hip (k_wrap_gather with the `active` table, k_walk_blend<..., SPARSE = true>): a sparse plan's
// parent is a plain plan, which the walk on the circle serves unchanged.
//
// The blend is the gather of blend.hip -- one thread owns a quad of a row for one or more planes and walks the parent's covering tile
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

extern "C" int mdtile_blend_sparse(const mdtile_plan* p, const mdtile_blend_args* a, const void* const* batch_out, int num_batches, const void* d_fill,
                                   mdtile_stream_t stream) {
    MDT_CHECK_ARG(p && a, "mdtile_blend_sparse: null plan/args");
    MDT_CHECK_ARG(plan_sparse(p), "mdtile_blend_sparse: not a sparse plan (mdtile_plan_create_subset): the blend of a full plan is mdtile_blend");
    return walk_blend(p, a, batch_out, num_batches, 0, d_fill, as_stream(stream));   // wrap.hip
}
