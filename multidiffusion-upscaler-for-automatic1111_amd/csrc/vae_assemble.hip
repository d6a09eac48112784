// Tiled VAE: every finished tile of one call into the image -- crop_valid_region + `result[...] = tile` (tilevae.py:248-259, 630-632)
// of up to MDTILE_VAE_ASSEMBLE_CHUNK tiles per launch.  The tiles may live on other devices of the process (one-process multi-device
// sweep, scripts/tilevae.py): the kernel reads them through the peer mapping, which mdtile_vae_assemble checks and enables first.
#include "launchers.h"
#include "vae_row_copy.h"

using namespace mdt;

namespace {

struct AsmTile {
    const float* src;   // first element of the valid window in plane 0
    long long dst_off;  // oy0 * RW + ox0
    int src_plane;      // th * tw
    int src_pitch;      // tw
    int cw, ch;         // valid window: columns, rows
};

struct AsmArgs {
    AsmTile t[MDTILE_VAE_ASSEMBLE_CHUNK];
    float* dst;
    long long dst_plane;  // RH * RW
    int dst_pitch;        // RW
    int planes;           // N * C
};

// block (bx, t): its four waves take rows (plane, yy) of tile t, one row per wave at a time.  Per row the destination gets whole 16-byte
// stores from its first 16-byte boundary on (a scalar head / tail around them); the source is read 16 bytes at a time when it has the same
// phase -- always on the decoder (windows start at multiples of 8 px), not always on the encoder (margins from a division by 8).
__global__ __launch_bounds__(256) void k_vae_assemble(const AsmArgs a) {
    const AsmTile& t = a.t[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int rows = a.planes * t.ch;
    const int nwaves = gridDim.x * 4;
    for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += nwaves) {
        const int p = r / t.ch, yy = r - p * t.ch;     // one division per row
        const float* s = t.src + (size_t)p * t.src_plane + (size_t)yy * t.src_pitch;
        float* d = a.dst + (size_t)p * a.dst_plane + t.dst_off + (size_t)yy * a.dst_pitch;
        copy_row(s, d, t.cw, lane);
    }
}

}  // namespace

// the device that owns `p` (device memory of this process), or -1
int mdt::device_of(const void* p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return attr.type == hipMemoryTypeDevice ? attr.device : -1;
}

extern "C" int mdtile_enable_peer_access(int device, int peer) {
    int n = 0;
    MDT_HIP(hipGetDeviceCount(&n));
    MDT_CHECK_ARG(device >= 0 && device < n && peer >= 0 && peer < n, "mdtile_enable_peer_access: device %d / peer %d of %d", device, peer, n);
    if (device == peer) return MDTILE_OK;
    int can = 0;
    MDT_HIP(hipDeviceCanAccessPeer(&can, device, peer));
    MDT_CHECK_ARG(can, "mdtile_enable_peer_access: device %d cannot read the memory of device %d", device, peer);
    int cur = 0;
    MDT_HIP(hipGetDevice(&cur));
    MDT_HIP(hipSetDevice(device));
    const hipError_t e = hipDeviceEnablePeerAccess(peer, 0);
    (void)hipGetLastError();      // hipErrorPeerAccessAlreadyEnabled must not reach the next launch check
    MDT_HIP(hipSetDevice(cur));
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
        set_error("mdtile_enable_peer_access(%d, %d): %s", device, peer, hipGetErrorString(e));
        return MDTILE_E_HIP;
    }
    return MDTILE_OK;
}

// what mdtile_vae_assemble asks of its table, for `who` (mdtile_vae_assemble, mdtile_vae_assemble_sparse); maps every source device
int mdt::vae_assemble_check(const char* who, const mdtile_vae_tile* tiles, int n_tiles, int N, int C, int is_decoder, const float* d_result, int RH,
                            int RW) {
    MDT_CHECK_ARG((tiles || n_tiles == 0) && d_result && n_tiles >= 0 && N > 0 && C > 0 && RH > 0 && RW > 0, "%s: bad arguments", who);
    int cur = 0;
    MDT_HIP(hipGetDevice(&cur));
    MDT_CHECK_ARG(device_of(d_result) == cur, "%s: the result is not device memory of the calling device %d", who, cur);
    // validate the whole table (and map every source device) before the first launch: an error return leaves the image untouched
    unsigned long long peers_ok = 0;   // bit d: device d's memory is readable from here
    for (int i = 0; i < n_tiles; ++i) {
        const mdtile_vae_tile& t = tiles[i];
        MDT_CHECK_ARG(t.tile && t.th > 0 && t.tw > 0, "%s: tile %d: bad arguments", who, i);
        int m[4];
        for (int k = 0; k < 4; ++k) m[k] = t.out_bbox4[k] - (is_decoder ? t.in_bbox4[k] * 8 : t.in_bbox4[k] / 8);   // tilevae.py:257-258
        const int cw = t.tw + m[1] - m[0], ch = t.th + m[3] - m[2];
        MDT_CHECK_ARG(m[0] >= 0 && m[2] >= 0 && m[1] <= 0 && m[3] <= 0 && cw > 0 && ch > 0,
                      "%s: tile %d: inconsistent bboxes (margins %d %d %d %d)", who, i, m[0], m[1], m[2], m[3]);
        MDT_CHECK_ARG(cw == t.out_bbox4[1] - t.out_bbox4[0] && ch == t.out_bbox4[3] - t.out_bbox4[2],
                      "%s: tile %d: crop %dx%d != target window %dx%d", who, i, cw, ch, t.out_bbox4[1] - t.out_bbox4[0],
                      t.out_bbox4[3] - t.out_bbox4[2]);
        MDT_CHECK_ARG(t.out_bbox4[0] >= 0 && t.out_bbox4[2] >= 0 && t.out_bbox4[1] <= RW && t.out_bbox4[3] <= RH,
                      "%s: tile %d: target window outside the result", who, i);
        MDT_CHECK_ARG((long long)N * C * ch <= 0x7fffffff && (long long)t.th * t.tw <= 0x7fffffff, "%s: tile %d too large", who, i);
        const int dev = device_of(t.tile);
        MDT_CHECK_ARG(dev >= 0 && dev < 64, "%s: tile %d is not device memory", who, i);
        if (dev != cur && !(peers_ok >> dev & 1)) {
            const int rc = mdtile_enable_peer_access(cur, dev);
            if (rc != MDTILE_OK) return rc;
            peers_ok |= 1ull << dev;
        }
    }
    return MDTILE_OK;
}

// the launches of mdtile_vae_assemble for a table that vae_assemble_check has passed
int mdt::vae_assemble_launch(const mdtile_vae_tile* tiles, int n_tiles, int N, int C, int is_decoder, float* d_result, int RH, int RW, hipStream_t s) {
    AsmArgs a;
    a.dst = d_result;
    a.dst_plane = (long long)RH * RW;
    a.dst_pitch = RW;
    a.planes = N * C;
    for (int c0 = 0; c0 < n_tiles; c0 += MDTILE_VAE_ASSEMBLE_CHUNK) {
        const int nt = n_tiles - c0 < MDTILE_VAE_ASSEMBLE_CHUNK ? n_tiles - c0 : MDTILE_VAE_ASSEMBLE_CHUNK;
        long long max_rows = 0;
        for (int k = 0; k < nt; ++k) {
            const mdtile_vae_tile& t = tiles[c0 + k];
            const int m0 = t.out_bbox4[0] - (is_decoder ? t.in_bbox4[0] * 8 : t.in_bbox4[0] / 8);
            const int m2 = t.out_bbox4[2] - (is_decoder ? t.in_bbox4[2] * 8 : t.in_bbox4[2] / 8);
            AsmTile& q = a.t[k];
            q.src = t.tile + (size_t)m2 * t.tw + m0;
            q.src_plane = t.th * t.tw;
            q.src_pitch = t.tw;
            q.cw = t.out_bbox4[1] - t.out_bbox4[0];
            q.ch = t.out_bbox4[3] - t.out_bbox4[2];
            q.dst_off = (long long)t.out_bbox4[2] * RW + t.out_bbox4[0];
            const long long rows = (long long)N * C * q.ch;
            max_rows = rows > max_rows ? rows : max_rows;
        }
        // about 2048 blocks (8 per CU) over the chunk; a tile never gets more blocks than it has 4-row groups
        long long bx = (max_rows + 3) / 4, cap = 2048 / nt;
        bx = bx < cap ? bx : cap;
        hipLaunchKernelGGL(k_vae_assemble, dim3((unsigned)(bx > 0 ? bx : 1), nt), dim3(256), 0, s, a);
        MDT_LAUNCH_CHECK();
    }
    return MDTILE_OK;
}

extern "C" int mdtile_vae_assemble(const mdtile_vae_tile* tiles, int n_tiles, int N, int C, int is_decoder, float* d_result, int RH, int RW,
                                   mdtile_stream_t stream) {
    MDT_CHECK_ARG(tiles, "mdtile_vae_assemble: bad arguments");
    if (int rc = vae_assemble_check("mdtile_vae_assemble", tiles, n_tiles, N, C, is_decoder, d_result, RH, RW)) return rc;
    return vae_assemble_launch(tiles, n_tiles, N, C, is_decoder, d_result, RH, RW, as_stream(stream));
}

// ---- the assembly with cross-faded tile borders (include/mdtile.h: mdtile_vae_assemble_blend) --------------------------
namespace {

struct SeamSrc {
    const float* p;   // element (0, 0) of plane 0 of the padded tile
    long long off;    // index of image pixel (0, 0) in that plane: -(ty0 * pitch + tx0), (tx0, ty0) = the image position of element (0, 0)
    int plane;        // th * tw
    int pitch;        // tw
};

struct SeamTile {
    SeamSrc s[9];     // the tile's 3 x 3 neighbourhood in the grid, row-major, itself at [4]; a neighbour that does not exist is never read
    int ox0, oy0;     // out box origin
    int cw, ch;       // out box: columns, rows
    int nb;           // neighbours: bit 0 left, 1 right, 2 up, 3 down
    int pad_;
};

struct SeamArgs {
    SeamTile t[MDTILE_VAE_BLEND_CHUNK];
    float* dst;
    long long dst_plane;  // RH * RW
    int dst_pitch;        // RW
    int planes;           // N * C
    int band;             // b
};
static_assert(sizeof(SeamArgs) <= 4096, "the table of one launch travels in the kernel arguments");

// value of image pixel (x, row) in a source whose row starts at index `row` (SeamSrc::off + plane and row terms)
__device__ __forceinline__ float seam_at(const SeamSrc& s, long long row, int x) { return s.p[row + x]; }

// k_vae_assemble's structure: block (bx, t), its four waves take rows (plane, yy) of tile t's out box.  Per row the vertical partner (up,
// down or none) and aT / aB are wave-uniform; the head band (b columns, left partner) and the tail band (b columns, right partner) blend
// 2 or 4 sources per pixel; the columns between them are one source (k_vae_assemble's 16-byte non-temporal copy) or, on a row inside a
// row band, two.  Sums in ascending tile index: (up, left) < (up, right) < (down, left) < (down, right).
__global__ __launch_bounds__(256) void k_vae_seam_blend(const SeamArgs a) {
    const SeamTile& t = a.t[blockIdx.y];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = a.band;
    const int rows = a.planes * t.ch;
    const int nwaves = gridDim.x * 4;
    const int hb = (t.nb & 1) ? b : 0, tb = (t.nb & 2) ? b : 0;   // columns of the head / tail band
    const int cm = t.cw - hb - tb;                                // columns between them (>= 0: the bands fit the tile)
    const float d2 = (float)(4 * b), d4 = (float)(16 * b * b);
    for (int r = blockIdx.x * 4 + wave; r < rows; r += nwaves) {
        const int p = r / t.ch, yy = r - p * t.ch;     // one division per row
        const int y = t.oy0 + yy;
        // the row band this row lies in: grid rows (rT, rB) of the neighbourhood with weights (aT, aB); aB == 0: none
        int rT = 1, rB = 1, aB = 0;
        if ((t.nb & 4) && yy < b) {
            rT = 0;
            aB = 2 * (yy + b) + 1;
        } else if ((t.nb & 8) && yy >= t.ch - b) {
            rB = 2;
            aB = 2 * (yy - t.ch + b) + 1;
        }
        const int aT = 4 * b - aB;
        const SeamSrc* sT = t.s + 3 * rT;
        const SeamSrc* sB = t.s + 3 * rB;
        long long oT[3], oB[3];                        // row starts in the (left, middle, right) source of the upper / lower grid row
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            oT[c] = (long long)p * sT[c].plane + sT[c].off + (long long)y * sT[c].pitch;
            oB[c] = (long long)p * sB[c].plane + sB[c].off + (long long)y * sB[c].pitch;
        }
        float* d = a.dst + (size_t)p * a.dst_plane + (size_t)y * a.dst_pitch + t.ox0;
        // head band (cL = 0: columns 0, 1 of the neighbourhood) and tail band (cL = 1: columns 1, 2)
#pragma unroll
        for (int cL = 0; cL < 2; ++cL) {
            const int n = cL ? tb : hb, x0 = cL ? t.cw - tb : 0;
            for (int j = lane; j < n; j += 64) {
                const int xx = x0 + j, x = t.ox0 + xx;
                const int aR = 2 * (j + (cL ? 0 : b)) + 1, aL = 4 * b - aR;
                float acc = 0.0f;
                if (aB == 0) {
                    acc = acc + (float)aL * seam_at(sT[cL], oT[cL], x);
                    acc = acc + (float)aR * seam_at(sT[cL + 1], oT[cL + 1], x);
                    d[xx] = acc / d2;
                } else {
                    acc = acc + (float)(aT * aL) * seam_at(sT[cL], oT[cL], x);
                    acc = acc + (float)(aT * aR) * seam_at(sT[cL + 1], oT[cL + 1], x);
                    acc = acc + (float)(aB * aL) * seam_at(sB[cL], oB[cL], x);
                    acc = acc + (float)(aB * aR) * seam_at(sB[cL + 1], oB[cL + 1], x);
                    d[xx] = acc / d4;
                }
            }
        }
        if (aB != 0) {                                 // between the bands, inside a row band: the tiles above and below
            for (int j = lane; j < cm; j += 64) {
                const int xx = hb + j, x = t.ox0 + xx;
                float acc = 0.0f;
                acc = acc + (float)aT * seam_at(sT[1], oT[1], x);
                acc = acc + (float)aB * seam_at(sB[1], oB[1], x);
                d[xx] = acc / d2;
            }
            continue;
        }
        // between the bands, in no row band: k_vae_assemble's copy of the tile's own columns [hb, cw - tb)
        const float* s = t.s[4].p + (oT[1] + t.ox0 + hb);
        d += hb;
        copy_row(s, d, cm, lane);
    }
}

}  // namespace

extern "C" int mdtile_vae_assemble_blend(const mdtile_vae_tile* tiles, int rows, int cols, int N, int C, int is_decoder, int band,
                                         float* d_result, int RH, int RW, mdtile_stream_t stream) {
    MDT_CHECK_ARG(tiles && d_result && rows > 0 && cols > 0 && N > 0 && C > 0 && RH > 0 && RW > 0, "mdtile_vae_assemble_blend: bad arguments");
    MDT_CHECK_ARG((long long)rows * cols <= 0x7fffffff, "mdtile_vae_assemble_blend: %d x %d tiles", rows, cols);
    MDT_CHECK_ARG(band >= 1 && band <= 1024, "mdtile_vae_assemble_blend: band %d is not in 1 .. 1024", band);
    int cur = 0;
    MDT_HIP(hipGetDevice(&cur));
    MDT_CHECK_ARG(device_of(d_result) == cur, "mdtile_vae_assemble_blend: the result is not device memory of the calling device %d", cur);
    const int n_tiles = rows * cols;
    auto margin = [&](const mdtile_vae_tile& t, int k) { return t.out_bbox4[k] - (is_decoder ? t.in_bbox4[k] * 8 : t.in_bbox4[k] / 8); };
    // validate the whole table (and map every source device) before the first launch: an error return leaves the image untouched
    unsigned long long peers_ok = 0;   // bit d: device d's memory is readable from here
    for (int i = 0; i < n_tiles; ++i) {
        const mdtile_vae_tile& t = tiles[i];
        const int gr = i / cols, gc = i - gr * cols;
        MDT_CHECK_ARG(t.tile && t.th > 0 && t.tw > 0, "mdtile_vae_assemble_blend: tile %d: bad arguments", i);
        int m[4];
        for (int k = 0; k < 4; ++k) m[k] = margin(t, k);
        const int cw = t.tw + m[1] - m[0], ch = t.th + m[3] - m[2];
        MDT_CHECK_ARG(m[0] >= 0 && m[2] >= 0 && m[1] <= 0 && m[3] <= 0 && cw > 0 && ch > 0,
                      "mdtile_vae_assemble_blend: tile %d: inconsistent bboxes (margins %d %d %d %d)", i, m[0], m[1], m[2], m[3]);
        MDT_CHECK_ARG(cw == t.out_bbox4[1] - t.out_bbox4[0] && ch == t.out_bbox4[3] - t.out_bbox4[2],
                      "mdtile_vae_assemble_blend: tile %d: crop %dx%d != target window %dx%d", i, cw, ch, t.out_bbox4[1] - t.out_bbox4[0],
                      t.out_bbox4[3] - t.out_bbox4[2]);
        // the grid: column borders as row 0 has them, row borders as column 0 has them, from 0 to the result's size
        const int* o = t.out_bbox4;
        const int* o_col = tiles[gc].out_bbox4;
        const int* o_row = tiles[gr * cols].out_bbox4;
        MDT_CHECK_ARG(o[0] == o_col[0] && o[1] == o_col[1] && o[2] == o_row[2] && o[3] == o_row[3] &&
                          o[0] == (gc == 0 ? 0 : tiles[i - 1].out_bbox4[1]) && o[2] == (gr == 0 ? 0 : tiles[i - cols].out_bbox4[3]) &&
                          (gc < cols - 1 || o[1] == RW) && (gr < rows - 1 || o[3] == RH),
                      "mdtile_vae_assemble_blend: tile %d: out box x %d..%d y %d..%d does not lie on the %d x %d grid over the %d x %d result "
                      "(hole or overlap)", i, o[0], o[1], o[2], o[3], rows, cols, RW, RH);
        const int nbx = (gc > 0) + (gc < cols - 1), nby = (gr > 0) + (gr < rows - 1);
        MDT_CHECK_ARG(cw >= band * nbx, "mdtile_vae_assemble_blend: tile %d: %d px wide, %s", i, cw,
                      nbx == 2 && cw >= band ? "its two column bands overlap" : "the band is wider than the tile");
        MDT_CHECK_ARG(ch >= band * nby, "mdtile_vae_assemble_blend: tile %d: %d px tall, %s", i, ch,
                      nby == 2 && ch >= band ? "its two row bands overlap" : "the band is taller than the tile");
        MDT_CHECK_ARG((gc == 0 || m[0] >= band) && (gc == cols - 1 || -m[1] >= band) && (gr == 0 || m[2] >= band) &&
                          (gr == rows - 1 || -m[3] >= band),
                      "mdtile_vae_assemble_blend: tile %d: margin smaller than the band %d (margins %d %d %d %d)", i, band, m[0], -m[1], m[2], -m[3]);
        MDT_CHECK_ARG((long long)N * C * ch <= 0x7fffffff && (long long)t.th * t.tw <= 0x7fffffff, "mdtile_vae_assemble_blend: tile %d too large", i);
        const int dev = device_of(t.tile);
        MDT_CHECK_ARG(dev >= 0 && dev < 64, "mdtile_vae_assemble_blend: tile %d is not device memory", i);
        if (dev != cur && !(peers_ok >> dev & 1)) {
            const int rc = mdtile_enable_peer_access(cur, dev);
            if (rc != MDTILE_OK) return rc;
            peers_ok |= 1ull << dev;
        }
    }
    hipStream_t s = as_stream(stream);
    SeamArgs a;
    a.dst = d_result;
    a.dst_plane = (long long)RH * RW;
    a.dst_pitch = RW;
    a.planes = N * C;
    a.band = band;
    for (int c0 = 0; c0 < n_tiles; c0 += MDTILE_VAE_BLEND_CHUNK) {
        const int nt = n_tiles - c0 < MDTILE_VAE_BLEND_CHUNK ? n_tiles - c0 : MDTILE_VAE_BLEND_CHUNK;
        long long max_rows = 0;
        for (int k = 0; k < nt; ++k) {
            const int i = c0 + k, gr = i / cols, gc = i - gr * cols;
            SeamTile& q = a.t[k];
            q.nb = (gc > 0 ? 1 : 0) | (gc < cols - 1 ? 2 : 0) | (gr > 0 ? 4 : 0) | (gr < rows - 1 ? 8 : 0);
            q.pad_ = 0;
            for (int dr = -1; dr <= 1; ++dr)
                for (int dc = -1; dc <= 1; ++dc) {
                    const int nr = gr + dr, nc = gc + dc;
                    const bool there = nr >= 0 && nr < rows && nc >= 0 && nc < cols;
                    const mdtile_vae_tile& t = tiles[there ? nr * cols + nc : i];
                    SeamSrc& src = q.s[3 * (dr + 1) + dc + 1];
                    src.p = t.tile;
                    src.plane = t.th * t.tw;
                    src.pitch = t.tw;
                    src.off = -((long long)(t.out_bbox4[2] - margin(t, 2)) * t.tw + (t.out_bbox4[0] - margin(t, 0)));
                }
            const mdtile_vae_tile& t = tiles[i];
            q.ox0 = t.out_bbox4[0];
            q.oy0 = t.out_bbox4[2];
            q.cw = t.out_bbox4[1] - t.out_bbox4[0];
            q.ch = t.out_bbox4[3] - t.out_bbox4[2];
            const long long nrows = (long long)N * C * q.ch;
            max_rows = nrows > max_rows ? nrows : max_rows;
        }
        // about 2048 blocks (8 per CU) over the chunk; a tile never gets more blocks than it has 4-row groups
        long long bx = (max_rows + 3) / 4, cap = 2048 / nt;
        bx = bx < cap ? bx : cap;
        hipLaunchKernelGGL(k_vae_seam_blend, dim3((unsigned)(bx > 0 ? bx : 1), nt), dim3(256), 0, s, a);
        MDT_LAUNCH_CHECK();
    }
    return MDTILE_OK;
}
