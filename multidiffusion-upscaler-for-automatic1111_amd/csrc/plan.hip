// Grid planning: host-side integer logic + the small device lookup tables the gather-formulated kernels use.
// Upstream behaviour followed: tile_utils/utils.py:160-177 (split_bboxes), tile_methods/abstractdiffusion.py:173-186
// (init_grid_bbox), scripts/tilevae.py:390-462 (split_tiles / get_best_tile_size).
#include <algorithm>
#include <cmath>
#include <vector>

#include "launchers.h"

namespace mdt {
static thread_local char g_err[512] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace mdt

extern "C" int mdtile_version(void) { return MDTILE_VERSION; }

int mdt::device_cus() {
    static const int n = [] {
        int dev = 0, cus = 256;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
            cus = prop.multiProcessorCount;
        return cus;
    }();
    return n;
}

// ---- arithmetic of the matrix-core kernels: split-bf16 ("bf16x3") by default, exact fp32 MFMA or single bf16 on request ----
// g_precision bits: 1 = convs on exact fp32, 2 = attention on exact fp32 (MDTILE_CONV_MODE / MDTILE_ATTN_MODE presets, either or both),
// 4 = single-term bf16 MFMAs (MDTILE_PRECISION_BF16), 8 = MDTILE_PRECISION_F16.  A strict bit wins over bits 4 / 8 for the kernels it covers.
namespace mdt {
static int g_precision = [] {
    const char* c = getenv("MDTILE_CONV_MODE");
    const char* a = getenv("MDTILE_ATTN_MODE");
    return ((c && strcmp(c, "f32") == 0) ? 1 : 0) | ((a && strcmp(a, "f32") == 0) ? 2 : 0);
}();
bool conv_strict_f32() { return (g_precision & 1) != 0; }
bool attn_strict_f32() { return (g_precision & 2) != 0; }
bool mfma_single_term() { return (g_precision & 4) != 0; }
bool mode_f16() { return (g_precision & 8) != 0; }
}  // namespace mdt
extern "C" int mdtile_set_precision(int mode) {
    if (mode != MDTILE_PRECISION_BF16X3 && mode != MDTILE_PRECISION_F32 && mode != MDTILE_PRECISION_BF16 && mode != MDTILE_PRECISION_F16) {
        mdt::set_error("mdtile_set_precision: unknown mode %d", mode);
        return MDTILE_E_ARG;
    }
    mdt::g_precision = mode == MDTILE_PRECISION_F32 ? 3 : mode == MDTILE_PRECISION_BF16 ? 4 : mode == MDTILE_PRECISION_F16 ? 8 : 0;
    return MDTILE_OK;
}
extern "C" int mdtile_get_precision(void) {
    return mdt::g_precision == 3 ? MDTILE_PRECISION_F32 : (mdt::g_precision & 4) ? MDTILE_PRECISION_BF16 : (mdt::g_precision & 8) ? MDTILE_PRECISION_F16 : MDTILE_PRECISION_BF16X3;
}
extern "C" const char* mdtile_last_error(void) { return mdt::g_err; }

// 1-D origins: count = ceil((extent-ov)/(tile-ov)); step is a double; origin = min(trunc(i*step), extent-tile).
static void origins_1d(int extent, int tile, int ov, std::vector<int>& out) {
    int n = (int)std::ceil((double)(extent - ov) / (double)(tile - ov));
    if (n < 1) n = 1;
    double step = n > 1 ? (double)(extent - tile) / (double)(n - 1) : 0.0;
    out.resize(n);
    for (int i = 0; i < n; ++i) {
        int o = (int)((double)i * step);
        out[i] = o < extent - tile ? o : extent - tile;
    }
}

// per canvas coordinate: first tile index covering it and how many consecutive tiles do (origins are non-decreasing)
static void cover_ranges(int extent, int tile, const std::vector<int>& org, std::vector<int>& packed) {
    packed.assign(extent, 0);
    int n = (int)org.size();
    for (int p = 0; p < extent; ++p) {
        int first = -1, cnt = 0;
        for (int i = 0; i < n; ++i)
            if (org[i] <= p && p < org[i] + tile) {
                if (first < 0) first = i;
                ++cnt;
            }
        packed[p] = (first < 0 ? 0 : first) | (cnt << 16);
    }
}

extern "C" mdtile_plan* mdtile_plan_create(int w, int h, int tile_w, int tile_h, int overlap, int tile_bs, int clamp) {
    if (w <= 0 || h <= 0 || tile_w <= 0 || tile_h <= 0 || tile_bs <= 0 || w > 65535 || h > 65535) {
        mdt::set_error("mdtile_plan_create: bad arguments w=%d h=%d tile=%dx%d bs=%d", w, h, tile_w, tile_h, tile_bs);
        return nullptr;
    }
    int tw = tile_w, th = tile_h, ov = overlap;
    if (clamp) {
        tw = tile_w < w ? tile_w : w;
        th = tile_h < h ? tile_h : h;
        int mn = tile_w < tile_h ? tile_w : tile_h;  // NOTE: requested, not clamped, sizes (abstractdiffusion.py:178)
        ov = overlap < mn - 4 ? overlap : mn - 4;
        if (ov < 0) ov = 0;
    } else if (tw > w || th > h || ov < 0) {
        mdt::set_error("mdtile_plan_create: raw grid needs tile <= canvas and overlap >= 0");
        return nullptr;
    }
    if (tw - ov == 0 || th - ov == 0) {  // upstream raises ZeroDivisionError here (utils.py:161-162)
        mdt::set_error("mdtile_plan_create: overlap %d equals the canvas-clamped tile %dx%d (division by zero upstream)", ov, tw, th);
        return nullptr;
    }
    std::vector<int> xs, ys, cr, rr;
    origins_1d(w, tw, ov, xs);
    origins_1d(h, th, ov, ys);
    if (xs.size() > 32767 || ys.size() > 32767) {
        mdt::set_error("mdtile_plan_create: too many tiles");
        return nullptr;
    }
    cover_ranges(w, tw, xs, cr);
    cover_ranges(h, th, ys, rr);

    mdtile_plan* p = new mdtile_plan();
    p->w = w; p->h = h; p->tw = tw; p->th = th; p->ov = ov;
    p->cols = (int)xs.size(); p->rows = (int)ys.size(); p->T = p->cols * p->rows;
    p->num_batches = (p->T + tile_bs - 1) / tile_bs;
    p->tile_bs = (p->T + p->num_batches - 1) / p->num_batches;
    // one host block [xs | ys | colrange | rowrange]; mirrored to the device lazily (mdt::plan_upload) so that the
    // integer planning works on a machine without a GPU.
    const int W4 = (w + 3) / 4;
    const size_t head = xs.size() + ys.size() + cr.size() + rr.size();
    p->quad_off = (head + 3) & ~(size_t)3;
    p->table_len = p->quad_off + 4 * (size_t)W4 + 4 * (size_t)h;
    p->h_table = new int[p->table_len]();
    int* q = p->h_table;
    p->h_xs = q; memcpy(q, xs.data(), xs.size() * sizeof(int)); q += xs.size();
    p->h_ys = q; memcpy(q, ys.data(), ys.size() * sizeof(int)); q += ys.size();
    memcpy(q, cr.data(), cr.size() * sizeof(int)); q += cr.size();
    memcpy(q, rr.data(), rr.size() * sizeof(int));
    // 16-byte records (see common.h).  A quad's candidate columns are the union over its (in-canvas) pixels; origins are
    // non-decreasing and every pixel is covered, so the union is a contiguous index range.
    auto origin3 = [](const std::vector<int>& org, int first, int k) { return first + k < (int)org.size() ? org[first + k] : 0; };
    int* cq = p->h_table + p->quad_off;
    p->nc_max = p->nr_max = 0;
    for (int xq = 0; xq < W4; ++xq) {
        int first = 1 << 30, last = -1;
        for (int j = 0; j < 4 && 4 * xq + j < w; ++j) {
            const int f = cr[4 * xq + j] & 0xffff, n = cr[4 * xq + j] >> 16;
            if (n == 0) continue;
            if (f < first) first = f;
            if (f + n - 1 > last) last = f + n - 1;
        }
        if (last < 0) { first = 0; last = -1; }
        cq[4 * xq + 0] = first | ((last - first + 1) << 16);
        if (last - first + 1 > p->nc_max) p->nc_max = last - first + 1;
        for (int k = 0; k < 3; ++k) cq[4 * xq + 1 + k] = origin3(xs, first, k);
    }
    int* ri = cq + 4 * (size_t)W4;
    for (int y = 0; y < h; ++y) {
        const int f = rr[y] & 0xffff;
        ri[4 * y + 0] = rr[y];
        if ((rr[y] >> 16) > p->nr_max) p->nr_max = rr[y] >> 16;
        for (int k = 0; k < 3; ++k) ri[4 * y + 1 + k] = origin3(ys, f, k);
    }
    p->d_xs = p->d_ys = p->d_colrange = p->d_rowrange = nullptr;
    p->d_colquad = p->d_rowinfo = nullptr;
    return p;
}

// ---- the canvas closed in x (panoramas), in y, or in both (seamless textures: a torus) ---------------------------------------------------
// start and length of the cyclic run of set members (the covering tiles of a canvas coordinate or quad: on a wrapped axis the tiles whose
// origin lies on the arc of `tile` coordinates that ends at it); all members -> (0, n).  A plain axis gives a run that never passes n.
static int cyclic_run(const std::vector<char>& member) {
    const int n = (int)member.size();
    int cnt = 0, first = 0;
    for (int c = 0; c < n; ++c) {
        cnt += member[c] ? 1 : 0;
        if (member[c] && !member[(c + n - 1) % n]) first = c;
    }
    return first | (cnt << 16);
}

// origins of one axis: on the circle when it wraps (stride extent / n <= tile - ov, so cyclic neighbours overlap by >= ov everywhere, the seam
// included), origins_1d when it does not
static void axis_origins(int extent, int tile, int ov, bool wrap, std::vector<int>& out) {
    if (!wrap) return origins_1d(extent, tile, ov, out);
    const int n = (int)std::ceil((double)extent / (double)(tile - ov));
    out.resize(n);
    for (int i = 0; i < n; ++i) out[i] = (int)((double)i * (double)extent / (double)n);
}

// does the tile with origin `org` cover coordinate p?  (a plain tile never passes the edge: org + tile <= extent)
static inline bool axis_covers(int p, int org, int tile, int extent, bool wrap) {
    return wrap ? ((p - org + extent) % extent) < tile : (org <= p && p < org + tile);
}

// the run tables of one axis: range[p] = the run of the tiles that cover coordinate p, rec[4 * g] (the .x of a 16-byte record) = the run of
// the tiles that cover ANY coordinate of group g of `group` consecutive ones (4: the column quads; 1: the rows, whose record repeats range[p]).
// Returns the longest run of a record.
static int axis_runs(const std::vector<int>& org, int tile, int extent, bool wrap, int group, int* range, int* rec) {
    const int n = (int)org.size();
    std::vector<char> member(n), any(n);
    int longest = 0;
    for (int g = 0; g * group < extent; ++g) {
        std::fill(any.begin(), any.end(), 0);
        for (int p = g * group; p < (g + 1) * group && p < extent; ++p) {
            for (int i = 0; i < n; ++i) {
                member[i] = axis_covers(p, org[i], tile, extent, wrap);
                any[i] = any[i] || member[i];
            }
            range[p] = cyclic_run(member);
        }
        rec[4 * g] = cyclic_run(any);
        if ((rec[4 * g] >> 16) > longest) longest = rec[4 * g] >> 16;
    }
    return longest;
}

extern "C" mdtile_plan* mdtile_plan_create_wrap(int w, int h, int tile_w, int tile_h, int overlap, int tile_bs, int wrap_x, int wrap_y) {
    if (!wrap_x && !wrap_y) {
        mdt::set_error("mdtile_plan_create_wrap: neither axis wraps: the plain grid is mdtile_plan_create");
        return nullptr;
    }
    if (w <= 0 || h <= 0 || tile_w <= 0 || tile_h <= 0 || tile_bs <= 0 || w > 65535 || h > 65535) {
        mdt::set_error("mdtile_plan_create_wrap: bad arguments w=%d h=%d tile=%dx%d bs=%d", w, h, tile_w, tile_h, tile_bs);
        return nullptr;
    }
    // the clamp of mdtile_plan_create(clamp = 1)
    const int tw = tile_w < w ? tile_w : w, th = tile_h < h ? tile_h : h;
    const int mn = tile_w < tile_h ? tile_w : tile_h;
    int ov = overlap < mn - 4 ? overlap : mn - 4;
    if (ov < 0) ov = 0;
    if (wrap_x && tw >= w) {
        mdt::set_error("mdtile_plan_create_wrap: x axis: tile width %d >= canvas width %d: a tile would meet itself across the seam", tw, w);
        return nullptr;
    }
    if (wrap_y && th >= h) {
        mdt::set_error("mdtile_plan_create_wrap: y axis: tile height %d >= canvas height %d: a tile would meet itself across the seam", th, h);
        return nullptr;
    }
    if (tw - ov == 0 || th - ov == 0) {
        mdt::set_error("mdtile_plan_create_wrap: overlap %d equals the canvas-clamped tile %dx%d (division by zero upstream)", ov, tw, th);
        return nullptr;
    }
    std::vector<int> xs, ys;
    axis_origins(w, tw, ov, wrap_x != 0, xs);
    axis_origins(h, th, ov, wrap_y != 0, ys);
    if (xs.size() > 32767 || ys.size() > 32767) {
        mdt::set_error("mdtile_plan_create_wrap: too many tiles");
        return nullptr;
    }
    const int cols = (int)xs.size(), rows = (int)ys.size();

    mdtile_plan* p = new mdtile_plan();
    p->wrap_x = wrap_x ? 1 : 0;
    p->wrap_y = wrap_y ? 1 : 0;
    p->w = w; p->h = h; p->tw = tw; p->th = th; p->ov = ov;
    p->cols = cols; p->rows = rows; p->T = cols * rows;
    p->num_batches = (p->T + tile_bs - 1) / tile_bs;
    p->tile_bs = (p->T + p->num_batches - 1) / p->num_batches;
    // the block layout of mdtile_plan_create (mdt::plan_upload serves every kind): [xs | ys | colrange | rowrange | pad | colquad | rowinfo]
    const int W4 = (w + 3) / 4;
    const size_t head = (size_t)cols + rows + w + h;
    p->quad_off = (head + 3) & ~(size_t)3;
    p->table_len = p->quad_off + 4 * (size_t)W4 + 4 * (size_t)h;
    p->h_table = new int[p->table_len]();
    p->h_xs = p->h_table; memcpy(p->h_xs, xs.data(), xs.size() * sizeof(int));
    p->h_ys = p->h_xs + cols; memcpy(p->h_ys, ys.data(), ys.size() * sizeof(int));
    int* cr = p->h_ys + rows;
    int* cq = p->h_table + p->quad_off;
    p->nc_max = axis_runs(xs, tw, w, wrap_x != 0, 4, cr, cq);
    p->nr_max = axis_runs(ys, th, h, wrap_y != 0, 1, cr + w, cq + 4 * (size_t)W4);
    p->d_xs = p->d_ys = p->d_colrange = p->d_rowrange = nullptr;
    p->d_colquad = p->d_rowinfo = nullptr;
    return p;
}

// the canvas closed in x alone, under its first name
extern "C" mdtile_plan* mdtile_plan_create_wrap_x(int w, int h, int tile_w, int tile_h, int overlap, int tile_bs) {
    return mdtile_plan_create_wrap(w, h, tile_w, tile_h, overlap, tile_bs, 1, 0);
}

extern "C" int mdtile_plan_wrap_x(const mdtile_plan* p) { return p && p->wrap_x ? 1 : 0; }
extern "C" int mdtile_plan_wrap_y(const mdtile_plan* p) { return p && p->wrap_y ? 1 : 0; }

// ---- the tiles an inpaint mask touches ------------------------------------------------------------------------------------
// The parent's geometry and covering tables, copied (the parent may be destroyed first), plus slot[T] and active[Ta] behind them.
extern "C" mdtile_plan* mdtile_plan_create_subset(const mdtile_plan* parent, const int* h_active, int tile_bs) {
    if (!parent || !h_active || tile_bs <= 0) {
        mdt::set_error("mdtile_plan_create_subset: bad arguments (null parent / flags, or tile_bs=%d)", tile_bs);
        return nullptr;
    }
    if (mdt::plan_wraps(parent)) {
        mdt::set_error("mdtile_plan_create_subset: the parent is a %s plan: tile skipping is not combined with wrap-around", mdt::wrap_kind(parent));
        return nullptr;
    }
    if (mdt::plan_sparse(parent)) {
        mdt::set_error("mdtile_plan_create_subset: the parent is a sparse plan itself: take the subset of the full plan");
        return nullptr;
    }
    int Ta = 0;
    for (int t = 0; t < parent->T; ++t) Ta += h_active[t] ? 1 : 0;
    if (Ta == 0) {
        mdt::set_error("mdtile_plan_create_subset: no active tile (Ta == 0 of %d): there is nothing to run", parent->T);
        return nullptr;
    }
    const int nb = (Ta + tile_bs - 1) / tile_bs;
    if (nb > MDTILE_MAX_BATCHES) {
        mdt::set_error("mdtile_plan_create_subset: %d batches > MDTILE_MAX_BATCHES=%d (a sparse plan has no packed form: raise the tile batch size)", nb,
                       MDTILE_MAX_BATCHES);
        return nullptr;
    }
    mdtile_plan* p = new mdtile_plan(*parent);
    p->Ta = Ta;
    p->num_batches = nb;
    p->tile_bs = (Ta + nb - 1) / nb;
    p->slot_off = parent->table_len;                       // a multiple of 4 ints: quad_off is, and both record tables are
    p->table_len = p->slot_off + (size_t)parent->T + (size_t)Ta;
    p->h_table = new int[p->table_len]();
    memcpy(p->h_table, parent->h_table, parent->table_len * sizeof(int));
    p->h_xs = p->h_table;
    p->h_ys = p->h_table + p->cols;
    int* slot = p->h_table + p->slot_off;
    int* active = slot + p->T;
    for (int t = 0, s = 0; t < p->T; ++t) {
        slot[t] = h_active[t] ? s : -1;
        if (h_active[t]) active[s++] = t;
    }
    p->d_xs = p->d_ys = p->d_colrange = p->d_rowrange = p->d_slot = p->d_active = nullptr;   // its own device mirror, made on first use
    p->d_colquad = p->d_rowinfo = nullptr;
    return p;
}

extern "C" int mdtile_plan_active(const mdtile_plan* p, int* ids) {
    if (!p || !mdt::plan_sparse(p)) return 0;
    if (ids) memcpy(ids, p->h_table + p->slot_off + p->T, (size_t)p->Ta * sizeof(int));
    return p->Ta;
}

namespace mdt {
int plan_upload(const mdtile_plan* cp) {
    mdtile_plan* p = const_cast<mdtile_plan*>(cp);
    if (p->d_xs) return MDTILE_OK;
    int* d = nullptr;
    MDT_HIP(hipMalloc(&d, p->table_len * sizeof(int)));
    hipError_t e = hipMemcpy(d, p->h_table, p->table_len * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        set_error("plan_upload: hipMemcpy failed: %s", hipGetErrorString(e));
        return MDTILE_E_HIP;
    }
    p->d_xs = d; p->d_ys = d + p->cols; p->d_colrange = p->d_ys + p->rows; p->d_rowrange = p->d_colrange + p->w;
    p->d_colquad = reinterpret_cast<int4*>(d + p->quad_off);          // hipMalloc is 256-B aligned, quad_off % 4 == 0
    p->d_rowinfo = p->d_colquad + (p->w + 3) / 4;
    if (plan_sparse(p)) {
        p->d_slot = d + p->slot_off;
        p->d_active = p->d_slot + p->T;
    }
    return MDTILE_OK;
}
}  // namespace mdt

extern "C" void mdtile_plan_destroy(mdtile_plan* p) {
    if (!p) return;
    if (p->d_xs) (void)hipFree(p->d_xs);
    delete[] p->h_table;
    delete p;
}

extern "C" int mdtile_plan_info(const mdtile_plan* p, int* info8) {
    MDT_CHECK_ARG(p && info8, "mdtile_plan_info: null argument");
    info8[0] = p->cols; info8[1] = p->rows; info8[2] = mdt::plan_tiles(p); info8[3] = p->num_batches;
    info8[4] = p->tile_bs; info8[5] = p->tw; info8[6] = p->th; info8[7] = p->ov;
    return MDTILE_OK;
}

extern "C" int mdtile_plan_bboxes(const mdtile_plan* p, int* xywh) {
    MDT_CHECK_ARG(p && xywh, "mdtile_plan_bboxes: null argument");
    if (mdt::plan_sparse(p)) {   // the active boxes, ascending parent index
        const int* active = p->h_table + p->slot_off + p->T;
        for (int s = 0; s < p->Ta; ++s) {
            int* o = xywh + 4 * s;
            o[0] = p->h_xs[active[s] % p->cols]; o[1] = p->h_ys[active[s] / p->cols]; o[2] = p->tw; o[3] = p->th;
        }
        return MDTILE_OK;
    }
    for (int r = 0; r < p->rows; ++r)
        for (int c = 0; c < p->cols; ++c) {
            int* o = xywh + 4 * (r * p->cols + c);
            o[0] = p->h_xs[c]; o[1] = p->h_ys[r]; o[2] = p->tw; o[3] = p->th;
        }
    return MDTILE_OK;
}

// ---- Tiled VAE split (scripts/tilevae.py:390-462) -----------------------------------------------------------
static int best_tile_size(int lower, int upper) {
    for (int div = 32; div >= 2; div /= 2) {
        int rem = lower % div;
        if (rem == 0) return lower;
        int cand = lower - rem + div;
        if (cand <= upper) return cand;
    }
    return lower;
}

// get_best_tile_size (scripts/tilevae.py:390-403): smallest multiple of 32 / 16 / 8 / 4 / 2 >= lowerbound that still fits under upperbound
extern "C" int mdtile_vae_best_tile_size(int lowerbound, int upperbound) { return best_tile_size(lowerbound, upperbound); }

extern "C" int mdtile_vae_split_tiles(int h, int w, int tile_size, int is_decoder, int* in_bboxes, int* out_bboxes, int cap) {
    MDT_CHECK_ARG(h > 0 && w > 0 && tile_size > 0, "mdtile_vae_split_tiles: bad arguments");
    const int pad = is_decoder ? 11 : 32;
    int nh = (int)std::ceil((double)(h - 2 * pad) / (double)tile_size);
    int nw = (int)std::ceil((double)(w - 2 * pad) / (double)tile_size);
    if (nh < 1) nh = 1;
    if (nw < 1) nw = 1;
    int rh = best_tile_size((int)std::ceil((double)(h - 2 * pad) / (double)nh), tile_size);
    int rw = best_tile_size((int)std::ceil((double)(w - 2 * pad) / (double)nw), tile_size);
    int n = nh * nw;
    if (cap <= 0 || !in_bboxes || !out_bboxes) return n;
    MDT_CHECK_ARG(cap >= n, "mdtile_vae_split_tiles: capacity %d < %d tiles", cap, n);
    auto mn = [](int a, int b) { return a < b ? a : b; };
    auto mx = [](int a, int b) { return a > b ? a : b; };
    for (int i = 0; i < nh; ++i)
        for (int j = 0; j < nw; ++j) {
            int b[4] = {pad + j * rw, mn(pad + (j + 1) * rw, w), pad + i * rh, mn(pad + (i + 1) * rh, h)};
            int o[4] = {b[0] > pad ? b[0] : 0, b[1] < w - pad ? b[1] : w, b[2] > pad ? b[2] : 0, b[3] < h - pad ? b[3] : h};
            int* ob = out_bboxes + 4 * (i * nw + j);
            int* ib = in_bboxes + 4 * (i * nw + j);
            for (int k = 0; k < 4; ++k) ob[k] = is_decoder ? o[k] * 8 : o[k] / 8;  // Python // on non-negative ints
            ib[0] = mx(0, b[0] - pad); ib[1] = mn(w, b[1] + pad); ib[2] = mx(0, b[2] - pad); ib[3] = mn(h, b[3] + pad);
        }
    return n;
}
