// Tiled VAE tile skipping for img2img inpainting (include/mdtile.h): which output boxes of a decode the job's overlay mask
// touches (mdtile_mask_activity_u8), and the assembly that completes an image from the decoded tiles alone (mdtile_vae_assemble_sparse): the
// tiles pasted by mdtile_vae_assemble's own check and kernel (vae_assemble.hip), every other box filled from the init image's bytes or with
// zeros.  The fill is a layout change, interleaved bytes to planar fp32, on the row walk of vae_row_copy.h.
#include <vector>

#include "launchers.h"
#include "vae_row_copy.h"

using namespace mdt;

namespace {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ---- activity: active[b] = some byte of mask[y1:y2, x1:x2] is not zero ---------------------------------------------------------------------
// block (bx, b): its four waves take the rows of box b, one row per wave at a time.  A row segment is read as scalar bytes up to its first
// 16-byte boundary, 16 bytes per lane from there, scalar bytes behind the last whole 16; a wave stops at the first row in which any lane saw a
// non-zero byte and its lane 0 stores 1.  The flags were cleared in front of the launch, every store writes the same value: no atomics.
__global__ __launch_bounds__(256) void k_mask_activity_u8(const uint8_t* __restrict__ mask, int RW, const int* __restrict__ boxes4,
                                                          int* __restrict__ active) {
    const int b = blockIdx.y;
    const int x1 = boxes4[4 * b], x2 = boxes4[4 * b + 1], y1 = boxes4[4 * b + 2], y2 = boxes4[4 * b + 3];
    const int lane = threadIdx.x & 63;
    const int w = x2 - x1, nwaves = gridDim.x * 4;
    for (int y = y1 + blockIdx.x * 4 + (threadIdx.x >> 6); y < y2; y += nwaves) {
        const uint8_t* s = mask + (size_t)y * RW + x1;
        int head = (int)((16 - (reinterpret_cast<size_t>(s) & 15)) & 15);
        head = head < w ? head : w;
        unsigned any = 0;
        if (lane < head) any = s[lane];
        const uint8_t* sb = s + head;
        const int n16 = (w - head) >> 4;
        const u32x4* sv = reinterpret_cast<const u32x4*>(sb);
        for (int j = lane; j < n16; j += 64) {
            const u32x4 v = sv[j];
            any |= v.x | v.y | v.z | v.w;
        }
        const int tail = (w - head) & 15;
        if (lane < tail) any |= sb[16 * n16 + lane];
        if (__ballot(any != 0) != 0) {
            if (lane == 0) active[b] = 1;
            return;
        }
    }
}

// ---- fill: result[n, c, y, x] = (float)fill[y, x, c] / 127.5f - 1.0f, or +0.0f ---------------------------------------------------------------
struct FillArgs {
    int box[MDTILE_VAE_FILL_CHUNK][4];   // x1, x2, y1, y2
    const uint8_t* fill;                 // [RH, RW, C] or null
    float* dst;
    long long dst_plane;                 // RH * RW
    int dst_pitch;                       // RW
    int N, C;
};
static_assert(sizeof(FillArgs) <= 4096, "the table of one launch travels in the kernel arguments");

// block (bx, b): its four waves take rows (channel, yy) of box b.  The wave reads the row's bytes of its channel -- one contiguous run of
// cw * C bytes, every lane four pixels of it -- once and stores the values to that channel's plane of every image n.
template <bool HAS_FILL>
__global__ __launch_bounds__(256) void k_vae_fill(const FillArgs a) {
    const int* bx = a.box[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int cw = bx[1] - bx[0], ch = bx[3] - bx[2];
    const int rows = a.C * ch;
    const int nwaves = gridDim.x * 4;
    for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += nwaves) {
        const int c = r / ch, y = bx[2] + (r - c * ch);     // one division per row
        const size_t off = (size_t)y * a.dst_pitch + bx[0];
        for (int n = 0; n < a.N; ++n) {
            float* d = a.dst + (size_t)(n * a.C + c) * a.dst_plane + off;
            if constexpr (HAS_FILL) {
                const uint8_t* s = a.fill + off * a.C + c;
                const int C = a.C;
                store_row(d, cw, lane, [=](int i) { return (float)s[(size_t)i * C] / 127.5f - 1.0f; });
            } else {
                store_row(d, cw, lane, [](int) { return 0.0f; });
            }
        }
    }
}

struct Box {
    int x1, x2, y1, y2;
};

}  // namespace

extern "C" int mdtile_mask_activity_u8(const uint8_t* d_mask, int RH, int RW, const int* d_boxes4, int n_boxes, int* d_active,
                                       mdtile_stream_t stream) {
    MDT_CHECK_ARG(d_mask && d_boxes4 && d_active, "mdtile_mask_activity_u8: null argument");
    MDT_CHECK_ARG(RH > 0 && RW > 0, "mdtile_mask_activity_u8: bad mask size %d x %d", RW, RH);
    MDT_CHECK_ARG(n_boxes >= 1 && n_boxes <= MDTILE_MASK_ACTIVITY_MAX_BOXES, "mdtile_mask_activity_u8: n_boxes %d is not in 1 .. %d", n_boxes,
                  MDTILE_MASK_ACTIVITY_MAX_BOXES);
    hipStream_t s = as_stream(stream);
    // the boxes are checked on the host before anything is written: a box outside the mask would be read out of bounds
    std::vector<int> h(4 * (size_t)n_boxes);
    MDT_HIP(hipMemcpyAsync(h.data(), d_boxes4, h.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    MDT_HIP(hipStreamSynchronize(s));
    int max_h = 0;
    for (int i = 0; i < n_boxes; ++i) {
        const int* b = &h[4 * (size_t)i];
        MDT_CHECK_ARG(b[0] < b[1] && b[2] < b[3], "mdtile_mask_activity_u8: box %d: x %d..%d y %d..%d is empty", i, b[0], b[1], b[2], b[3]);
        MDT_CHECK_ARG(b[0] >= 0 && b[2] >= 0 && b[1] <= RW && b[3] <= RH, "mdtile_mask_activity_u8: box %d: x %d..%d y %d..%d lies outside the %d x %d mask",
                      i, b[0], b[1], b[2], b[3], RW, RH);
        max_h = b[3] - b[2] > max_h ? b[3] - b[2] : max_h;
    }
    MDT_HIP(hipMemsetAsync(d_active, 0, sizeof(int) * (size_t)n_boxes, s));
    // about 2048 blocks (8 per CU) over the boxes; a box never gets more blocks than it has 4-row groups
    int bx = (max_h + 3) / 4, cap = 2048 / n_boxes;
    cap = cap > 0 ? cap : 1;
    bx = bx < cap ? bx : cap;
    hipLaunchKernelGGL(k_mask_activity_u8, dim3((unsigned)bx, (unsigned)n_boxes), dim3(256), 0, s, d_mask, RW, d_boxes4, d_active);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

extern "C" int mdtile_vae_assemble_sparse(const mdtile_vae_tile* tiles, int n_tiles, const int* fill_boxes4, int n_fill, const uint8_t* d_fill_u8,
                                          int N, int C, float* d_result, int RH, int RW, mdtile_stream_t stream) {
    const char* who = "mdtile_vae_assemble_sparse";
    MDT_CHECK_ARG(n_tiles >= 0 && n_fill >= 0 && (fill_boxes4 || n_fill == 0), "%s: bad arguments", who);
    MDT_CHECK_ARG((long long)n_tiles + n_fill <= MDTILE_VAE_SPARSE_MAX_BOXES, "%s: %d tiles + %d fill boxes are more than %d boxes", who, n_tiles, n_fill,
                  MDTILE_VAE_SPARSE_MAX_BOXES);
    if (int rc = vae_assemble_check(who, tiles, n_tiles, N, C, 1, d_result, RH, RW)) return rc;
    MDT_CHECK_ARG((long long)C * RH <= 0x7fffffff, "%s: result too large", who);
    int cur = 0;
    MDT_HIP(hipGetDevice(&cur));
    MDT_CHECK_ARG(!d_fill_u8 || device_of(d_fill_u8) == cur, "%s: the fill image is not device memory of the calling device %d", who, cur);
    // every box of the call: the tiles' out boxes, then the fill boxes
    std::vector<Box> boxes;
    boxes.reserve((size_t)n_tiles + n_fill);
    for (int i = 0; i < n_tiles; ++i) boxes.push_back(Box{tiles[i].out_bbox4[0], tiles[i].out_bbox4[1], tiles[i].out_bbox4[2], tiles[i].out_bbox4[3]});
    for (int i = 0; i < n_fill; ++i) {
        const int* b = fill_boxes4 + 4 * (size_t)i;
        MDT_CHECK_ARG(b[0] < b[1] && b[2] < b[3], "%s: fill box %d: x %d..%d y %d..%d is empty", who, i, b[0], b[1], b[2], b[3]);
        MDT_CHECK_ARG(b[0] >= 0 && b[2] >= 0 && b[1] <= RW && b[3] <= RH, "%s: fill box %d: x %d..%d y %d..%d lies outside the %d x %d result", who, i,
                      b[0], b[1], b[2], b[3], RW, RH);
        boxes.push_back(Box{b[0], b[1], b[2], b[3]});
    }
    long long area = 0;
    for (size_t i = 0; i < boxes.size(); ++i) {
        const Box& p = boxes[i];
        area += (long long)(p.x2 - p.x1) * (p.y2 - p.y1);
        for (size_t j = 0; j < i; ++j) {
            const Box& q = boxes[j];
            if (p.x1 >= q.x2 || q.x1 >= p.x2 || p.y1 >= q.y2 || q.y1 >= p.y2) continue;
            const bool same = p.x1 == q.x1 && p.x2 == q.x2 && p.y1 == q.y1 && p.y2 == q.y2;
            MDT_CHECK_ARG(!(same && (int)i >= n_tiles && (int)j < n_tiles), "%s: fill box %d x %d..%d y %d..%d is also tile %d's out box", who,
                          (int)i - n_tiles, p.x1, p.x2, p.y1, p.y2, (int)j);
            MDT_CHECK_ARG(false, "%s: %s %d and %s %d overlap (x %d..%d y %d..%d, x %d..%d y %d..%d)", who, (int)j < n_tiles ? "tile" : "fill box",
                          (int)j < n_tiles ? (int)j : (int)j - n_tiles, (int)i < n_tiles ? "tile" : "fill box", (int)i < n_tiles ? (int)i : (int)i - n_tiles,
                          q.x1, q.x2, q.y1, q.y2, p.x1, p.x2, p.y1, p.y2);
        }
    }
    MDT_CHECK_ARG(area == (long long)RH * RW, "%s: the %d tiles and %d fill boxes cover %lld of the result's %lld pixels (area sum)", who, n_tiles, n_fill,
                  area, (long long)RH * RW);

    hipStream_t s = as_stream(stream);
    if (int rc = vae_assemble_launch(tiles, n_tiles, N, C, 1, d_result, RH, RW, s)) return rc;
    FillArgs a;
    a.fill = d_fill_u8;
    a.dst = d_result;
    a.dst_plane = (long long)RH * RW;
    a.dst_pitch = RW;
    a.N = N;
    a.C = C;
    for (int c0 = 0; c0 < n_fill; c0 += MDTILE_VAE_FILL_CHUNK) {
        const int nb = n_fill - c0 < MDTILE_VAE_FILL_CHUNK ? n_fill - c0 : MDTILE_VAE_FILL_CHUNK;
        long long max_rows = 0;
        for (int k = 0; k < nb; ++k) {
            const int* b = fill_boxes4 + 4 * (size_t)(c0 + k);
            for (int j = 0; j < 4; ++j) a.box[k][j] = b[j];
            const long long rows = (long long)C * (b[3] - b[2]);
            max_rows = rows > max_rows ? rows : max_rows;
        }
        // about 2048 blocks (8 per CU) over the chunk; a box never gets more blocks than it has 4-row groups
        long long bx = (max_rows + 3) / 4, cap = 2048 / nb;
        bx = bx < cap ? bx : cap;
        const dim3 grid((unsigned)(bx > 0 ? bx : 1), nb);
        if (d_fill_u8) hipLaunchKernelGGL(k_vae_fill<true>, grid, dim3(256), 0, s, a);
        else hipLaunchKernelGGL(k_vae_fill<false>, grid, dim3(256), 0, s, a);
        MDT_LAUNCH_CHECK();
    }
    return MDTILE_OK;
}
