// Region prompt control on a wrap-around canvas: rectangles that may cross x = W-1 -> 0 and y = H-1 -> 0 on the axes that wrap,
// on the grid at rest or displaced by this step's shift.  Four entry points -- mdtile_blend, mdtile_blend_shift and the plain rect calls keep
// their kernels and their refusals:
//   mdtile_gather_rect_wrap, mdtile_weight_map_add_rect_wrap, mdtile_region_noise_wrap   the plain rect kernels (blend.hip, maps.hip) with the
//                                                                                        rectangle's coordinates taken on the circle (rel())
//   mdtile_blend_wrap_regions   the argument checks here, the kernel in wrap.hip (k_walk_blend<..., REGIONS = true>, whose text has the arithmetic)
#include "launchers.h"
#include "walk.h"

using namespace mdt;

namespace {

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
    return walk_blend_regions(p, a, batch_out, num_batches, wr, num_fg, as_stream(stream));      // wrap.hip
}
