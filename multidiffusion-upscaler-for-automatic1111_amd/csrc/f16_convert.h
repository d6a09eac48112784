// The ONE conversion that defines the rounding contract of MDTILE_PRECISION_F16 (include/mdtile.h): clamp to the largest finite fp16
// (v_med3_f32: no Inf is ever written or multiplied), then v_cvt_pk_f16_f32 rounds a PAIR to nearest even.  Every producer of fp16
// operands goes through cvt2h: the record-out epilogue and k_rec_from_f32_f16 (conv_rec_common.h, vae_conv_rec.hip), the staging of the
// hand-over conv and the weight packer (vae_conv_bf16x3.hip).
#pragma once

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned mdt_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ unsigned cvt2h(float a, float b) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 p = {__builtin_amdgcn_fmed3f(a, -65504.0f, 65504.0f), __builtin_amdgcn_fmed3f(b, -65504.0f, 65504.0f)};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(p, h2));
}

// 8 values -> one 16-byte fp16 record
__device__ __forceinline__ void cvt8h(const float (&v)[8], mdt_u32x4& hi) {
#pragma unroll
    for (int j = 0; j < 4; ++j) hi[j] = cvt2h(v[2 * j], v[2 * j + 1]);
}
