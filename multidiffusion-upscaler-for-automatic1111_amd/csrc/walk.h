// What the quad blends share (wrap.hip: k_wrap_weight_grid, k_wrap_gather, k_walk_blend; wrap_regions.hip: the rect kernels; lattice.hip through
// lattice.h): the cyclic run of covering tile columns / rows, the circle-relative coordinate, the 4-element loads and raw stores of a quad, and
// the planes-per-thread rule of the launchers.
#pragma once
#include "common.h"

namespace mdt {

// the cyclic run (first | count << 16 over a list of `n` tile columns or rows) walked in ascending index: [0, head) then [first, first + count - head)
struct CyclicRun {
    int first, count, head;
    __device__ __forceinline__ CyclicRun(int packed, int n) {
        first = packed & 0xffff;
        count = packed >> 16;
        head = first + count > n ? first + count - n : 0;
    }
    __device__ __forceinline__ int at(int k) const { return k < head ? k : first + (k - head); }
};

// canvas coordinate p relative to a tile origin o, on the circle of `extent` coordinates: in [0, extent); covered by the tile iff < its size
__device__ __forceinline__ int rel(int p, int o, int extent) {
    const int d = p - o;
    return d < 0 ? d + extent : d;
}

// a coordinate p in [0, 2 extent) -- a sum of two that lie on the circle -- back onto it: one subtraction
__device__ __forceinline__ int onto(int p, int extent) { return p < extent ? p : p - extent; }

// the storage type as an integer of its size (what passes `fill` through without a float conversion), and 4 of them at an element-aligned
// address (one load / store instruction: gfx950 runs in unaligned-access mode)
template <typename T> struct RawOf { using type = unsigned short; };
template <> struct RawOf<float> { using type = unsigned int; };
template <typename R> struct __attribute__((packed, aligned(sizeof(R)))) raw4_u { R v[4]; };

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

// planes per thread of a quad blend on a W x H canvas: 4 while that leaves >= ~128k threads (2 per lane of the chip) and divides N*C, as blend.hip
// sizes k_blend
inline int planes_per_thread(int W, int H, int planes) {
    const long long work = (long long)H * ((W + 3) / 4) * planes;
    if (planes % 4 == 0 && work / 4 >= 131072) return 4;
    return planes % 2 == 0 && work / 2 >= 131072 ? 2 : 1;
}

}  // namespace mdt
