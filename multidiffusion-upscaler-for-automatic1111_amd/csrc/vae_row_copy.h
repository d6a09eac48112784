// One destination row of a Tiled VAE assembly, written by one wave: whole 16-byte stores from the row's first 16-byte boundary on, a scalar
// head / tail around them.  copy_row is the body of k_vae_assemble, of k_vae_seam_blend between its bands (vae_assemble.hip) and, through
// mdtile_vae_assemble's kernel, of mdtile_vae_assemble_sparse's tiles (vae_skip.hip); store_row is the same walk with computed values (the
// fill of mdtile_vae_assemble_sparse).
#pragma once
#include "common.h"

namespace mdt {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// d[0 .. cw) = s[0 .. cw), bit for bit.  The source is read 16 bytes at a time when it has the destination's phase -- always on the decoder
// (windows start at multiples of 8 px), not always on the encoder (margins from a division by 8).
__device__ __forceinline__ void copy_row(const float* s, float* d, int cw, int lane) {
    int head = (int)((16 - (reinterpret_cast<size_t>(d) & 15)) & 15) >> 2;
    head = head < cw ? head : cw;
    if (lane < head) d[lane] = s[lane];
    const float* sb = s + head;
    float* db = d + head;
    const int n4 = (cw - head) >> 2;
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
    const int tail = (cw - head) & 3;
    if (lane < tail) db[4 * n4 + lane] = sb[4 * n4 + lane];
}

// d[i] = at(i) for i in [0, cw): the same split of the row, the values computed
template <class At>
__device__ __forceinline__ void store_row(float* d, int cw, int lane, At at) {
    int head = (int)((16 - (reinterpret_cast<size_t>(d) & 15)) & 15) >> 2;
    head = head < cw ? head : cw;
    if (lane < head) d[lane] = at(lane);
    const int n4 = (cw - head) >> 2;
    f32x4* dv = reinterpret_cast<f32x4*>(d + head);
    for (int j = lane; j < n4; j += 64) {
        const int i = head + 4 * j;
        f32x4 v = {at(i), at(i + 1), at(i + 2), at(i + 3)};
        __builtin_nontemporal_store(v, dv + j);
    }
    const int tail = (cw - head) & 3;
    if (lane < tail) d[head + 4 * n4 + lane] = at(head + 4 * n4 + lane);
}

}  // namespace mdt
