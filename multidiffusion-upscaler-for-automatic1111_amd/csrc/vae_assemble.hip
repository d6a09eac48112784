// Tiled VAE: every finished tile of one call into the image -- crop_valid_region + `result[...] = tile` (tilevae.py:248-259, 630-632)
// of up to MDTILE_VAE_ASSEMBLE_CHUNK tiles per launch.  The tiles may live on other devices of the process (one-process multi-device
// sweep, scripts/tilevae.py): the kernel reads them through the peer mapping, which mdtile_vae_assemble checks and enables first.
#include "common.h"

using namespace mdt;

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

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
        int head = (int)((16 - (reinterpret_cast<size_t>(d) & 15)) & 15) >> 2;
        head = head < t.cw ? head : t.cw;
        if (lane < head) d[lane] = s[lane];
        const float* sb = s + head;
        float* db = d + head;
        const int n4 = (t.cw - head) >> 2;
        const f32x4* sv = reinterpret_cast<const f32x4*>(sb);
        f32x4* dv = reinterpret_cast<f32x4*>(db);
        if ((reinterpret_cast<size_t>(sb) & 15) == 0) {
            for (int j = lane; j < n4; j += 256) {
                f32x4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j + u * 64 < n4) v[u] = __builtin_nontemporal_load(sv + j + u * 64);
#pragma unroll
                for (int u = 0; u < 4; ++u)
                    if (j + u * 64 < n4) __builtin_nontemporal_store(v[u], dv + j + u * 64);
            }
        } else {
            for (int j = lane; j < n4; j += 64) {
                const float* q = sb + 4 * j;
                f32x4 v = {q[0], q[1], q[2], q[3]};
                __builtin_nontemporal_store(v, dv + j);
            }
        }
        const int tail = (t.cw - head) & 3;
        if (lane < tail) db[4 * n4 + lane] = sb[4 * n4 + lane];
    }
}

// the device that owns `p` (device memory of this process), or -1
int device_of(const void* p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();
        return -1;
    }
    return attr.type == hipMemoryTypeDevice ? attr.device : -1;
}

}  // namespace

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

extern "C" int mdtile_vae_assemble(const mdtile_vae_tile* tiles, int n_tiles, int N, int C, int is_decoder, float* d_result, int RH, int RW,
                                   mdtile_stream_t stream) {
    MDT_CHECK_ARG(tiles && d_result && n_tiles >= 0 && N > 0 && C > 0 && RH > 0 && RW > 0, "mdtile_vae_assemble: bad arguments");
    int cur = 0;
    MDT_HIP(hipGetDevice(&cur));
    MDT_CHECK_ARG(device_of(d_result) == cur, "mdtile_vae_assemble: the result is not device memory of the calling device %d", cur);
    AsmArgs a;
    a.dst = d_result;
    a.dst_plane = (long long)RH * RW;
    a.dst_pitch = RW;
    a.planes = N * C;
    // validate the whole table (and map every source device) before the first launch: an error return leaves the image untouched
    unsigned long long peers_ok = 0;   // bit d: device d's memory is readable from here
    for (int i = 0; i < n_tiles; ++i) {
        const mdtile_vae_tile& t = tiles[i];
        MDT_CHECK_ARG(t.tile && t.th > 0 && t.tw > 0, "mdtile_vae_assemble: tile %d: bad arguments", i);
        int m[4];
        for (int k = 0; k < 4; ++k) m[k] = t.out_bbox4[k] - (is_decoder ? t.in_bbox4[k] * 8 : t.in_bbox4[k] / 8);   // tilevae.py:257-258
        const int cw = t.tw + m[1] - m[0], ch = t.th + m[3] - m[2];
        MDT_CHECK_ARG(m[0] >= 0 && m[2] >= 0 && m[1] <= 0 && m[3] <= 0 && cw > 0 && ch > 0,
                      "mdtile_vae_assemble: tile %d: inconsistent bboxes (margins %d %d %d %d)", i, m[0], m[1], m[2], m[3]);
        MDT_CHECK_ARG(cw == t.out_bbox4[1] - t.out_bbox4[0] && ch == t.out_bbox4[3] - t.out_bbox4[2],
                      "mdtile_vae_assemble: tile %d: crop %dx%d != target window %dx%d", i, cw, ch, t.out_bbox4[1] - t.out_bbox4[0],
                      t.out_bbox4[3] - t.out_bbox4[2]);
        MDT_CHECK_ARG(t.out_bbox4[0] >= 0 && t.out_bbox4[2] >= 0 && t.out_bbox4[1] <= RW && t.out_bbox4[3] <= RH,
                      "mdtile_vae_assemble: tile %d: target window outside the result", i);
        MDT_CHECK_ARG((long long)N * C * ch <= 0x7fffffff && (long long)t.th * t.tw <= 0x7fffffff, "mdtile_vae_assemble: tile %d too large", i);
        const int dev = device_of(t.tile);
        MDT_CHECK_ARG(dev >= 0 && dev < 64, "mdtile_vae_assemble: tile %d is not device memory", i);
        if (dev != cur && !(peers_ok >> dev & 1)) {
            const int rc = mdtile_enable_peer_access(cur, dev);
            if (rc != MDTILE_OK) return rc;
            peers_ok |= 1ull << dev;
        }
    }
    hipStream_t s = as_stream(stream);
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
