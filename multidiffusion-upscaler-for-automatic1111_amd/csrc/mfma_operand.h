// Operand format of a matrix-core kernel body that is compiled more than once (no include guard: every body includes this file at its top).
//   MDT_OPERAND_F16 = 0: bf16 fragments on v_mfma_f32_32x32x16_bf16 (BF16X3, and the one-term forms of MDTILE_PRECISION_BF16)
//   MDT_OPERAND_F16 = 1: fp16 fragments on v_mfma_f32_32x32x16_f16 (MDTILE_PRECISION_F16; one-term bodies only) -- the same fragment shape,
//                        4 VGPRs per operand, the same lane -> (row, k) map, so the LDS images, DMA pieces and waits of the bf16 twin serve as they are
// Macros, not an overloaded helper: the bf16 kernels' token stream -- and with it their code -- stays what it was.
#undef MDT_FRAG
#undef MDT_MFMA
#if MDT_OPERAND_F16
#define MDT_FRAG f16x8
#define MDT_MFMA __builtin_amdgcn_mfma_f32_32x32x16_f16
#else
#define MDT_FRAG bf16x8
#define MDT_MFMA __builtin_amdgcn_mfma_f32_32x32x16_bf16
#endif
