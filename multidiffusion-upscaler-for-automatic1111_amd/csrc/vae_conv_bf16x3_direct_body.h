// Body of k_conv3x3_bf16x3 / k_conv3x3_bf16x1 (csrc/vae_conv_bf16x3.hip includes this file twice, the way vae_conv_rec.hip shares its bodies):
//   MDT_B3_TERMS = 3: the three-term kernel; = 1: MDTILE_PRECISION_BF16, w_hi x x_hi only.  The one-term form still splits and stages both
//   planes of its input (the LDS images and the load / store schedule are the three-term kernel's); it reads only the hi fragments.
//   MDT_OPERAND_F16 = 1 (with MDT_B3_TERMS = 1; k_conv3x3_f16, MDTILE_PRECISION_F16, GNS forms only): the activated input is rounded to fp16 while it is
//   staged (clamp to +-65504, v_cvt_pk_f16_f32; only the hi image is written) and the weights are the fp16 plane of mdtile_conv_pack_f16
#include "mfma_operand.h"
template <int MT, bool GNS, int S = 1, bool ST = false>
__global__ __launch_bounds__(512, (MT == 4 && S == 1) ? 4 : 2) void MDT_B3_KERNEL(const ConvBParams P) {
    constexpr int NT = MDT_B3_TERMS, NHL = NT == 3 ? 2 : 1;   // products per MFMA site (3: w_lo x_hi, w_hi x_lo, w_hi x_hi; 1: w_hi x_hi), weight planes read
    constexpr int TH_ = 8;
    constexpr bool WDMA = MT == 4, IB1 = MT == 4 || S == 2, TERM_MAJOR = MT == 4;   // (S = 2: the 72 KB halo tile exists once)
    constexpr int BM = MT * 32;
    constexpr int WAVES_M = MT / 2, WAVES_R = 8 / WAVES_M, NROW = TH_ / WAVES_R;
    constexpr int HCOL = TW + 1;                                   // S = 2: records per column parity of a row
    constexpr int COLSL = S == 1 ? COLS : 2 * HCOL;                // records per LDS row
    constexpr int ROWS_ = S == 1 ? TH_ + 2 : 2 * TH_ + 1, IN_REC_ = 2 * ROWS_ * COLSL;   // halo tile records per hl per stage
    constexpr int NPASS = (IN_REC_ + 511) / 512;                  // staging passes of the 512 threads
    constexpr int W_REC = 2 * 3 * MT * 64;              // records per weight chunk (hi block then lo block)
    constexpr int NWREG = (W_REC + 511) / 512;          // 3 (MT = 4) or 2 (MT = 2, half of the threads on the 2nd)
    // LDS (16-byte records): input [2 stages][hl][IN_REC_], weights [2 stages][W_REC]
    constexpr int IN_STAGE = 2 * IN_REC_, NIST = IB1 ? 1 : 2, WST = 2;
    __shared__ u32x4 smem[NIST * IN_STAGE + WST * W_REC];
    __shared__ float4 coef_l[GNS ? 2 * MAX_GN_CIN / 4 : 1];   // a[0..Cin) at 0, s[0..Cin) at MAX_GN_CIN
    u32x4* const in_l = smem;
    u32x4* const w_l = smem + NIST * IN_STAGE;

    // ---- block -> (pixel tile, cout block): XCD = id % 8 keeps all cout blocks of a pixel tile on one L2
    const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
    const int ptile = (slot / P.NCB) * 8 + xcd, cb = slot % P.NCB;
    if (ptile >= P.ptiles) return;
    const int b = blockIdx.y;
    const int py = ptile / P.PX, px = ptile - py * P.PX;
    const int y0 = py * TH_, x0 = px * TW;
    if (GNS) {
        float* cl = reinterpret_cast<float*>(coef_l);
        const float* cg = P.coef + (size_t)b * 2 * P.Cin;
        for (int c = threadIdx.x; c < P.Cin; c += 512) {
            cl[c] = cg[c];
            cl[MAX_GN_CIN + c] = cg[P.Cin + c];
        }
        __syncthreads();
    }

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kg = lane >> 5;
    const int wm = wave % WAVES_M, wr = wave / WAVES_M;
    const size_t HWin = (size_t)P.Hin * P.Win;
    const float* xb = P.x + (size_t)b * P.Cin * HWin;

    // ---- input staging map: record s = tid + 512 i -> (cg, r, c); source offset inside a channel plane, valid flag
    // (zero padding).  Loads are unconditional at a clamped address and zeroed by the flag: straight-line code.
    const int wave_u = __builtin_amdgcn_readfirstlane(wave);   // provably wave-uniform
    int soff[NPASS], scg[NPASS];
    float smask[NPASS];
#pragma unroll
    for (int i = 0; i < NPASS; ++i) {
        int s = tid + 512 * i;
        if (s >= IN_REC_) s = IN_REC_ - 1;                      // lanes past the end shadow the last record (never stored)
        const int cg = s / (ROWS_ * COLSL), p = s - cg * (ROWS_ * COLSL);
        const int r = p / COLSL, c = p - r * COLSL;
        int gy, gx;
        bool inside;
        if (S == 1) {
            gy = y0 + r - 1; gx = x0 + c - 1;
            inside = gy >= 0 && gy < P.H && gx >= 0 && gx < P.W;
        } else {           // LDS column c = parity * HCOL + i  <->  input column 2 i + parity of the halo tile (65 of the 66 slots are used)
            const int par = c / HCOL, ci = c - par * HCOL, col = 2 * ci + par;
            gy = 2 * y0 + r; gx = 2 * x0 + col;
            inside = col <= 2 * TW && gy < P.Hin && gx < P.Win;
        }
        scg[i] = cg;
        soff[i] = inside ? gy * P.Win + gx : 0;
        smask[i] = inside ? 1.0f : 0.0f;
    }
    float rin[NPASS][8];
    u32x4 rwt[WDMA ? 1 : NWREG];

    auto load_input = [&](int k) {       // K-step k: channels 16k .. 16k+15
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            if (wave_u * 64 + 512 * i < IN_REC_) {               // whole waves past the end of the record list skip the pass
                const float* src = xb + (size_t)kstep_c0(k, scg[i], P.perm) * HWin + soff[i];
#pragma unroll
                for (int j = 0; j < 8; ++j) rin[i][j] = src[(size_t)kstep_cj(j, P.perm) * HWin];
            }
        }
    };
    auto store_input = [&](int stage, int k) {   // k: the K-step held in rin (channels 16k ..)
        u32x4* dst = in_l + stage * IN_STAGE;
#pragma unroll
        for (int i = 0; i < NPASS; ++i) {
            if (wave_u * 64 + 512 * i < IN_REC_) {
                float v[8];
                if (GNS) {
                    const int c4 = kstep_c0(k, scg[i], P.perm) >> 2, c4b = c4 + (P.perm ? 2 : 1);   // channels j = 4..7 sit 8 (perm) or 4 further
                    const float4 a0 = coef_l[c4], a1 = coef_l[c4b], s0 = coef_l[MAX_GN_CIN / 4 + c4], s1 = coef_l[MAX_GN_CIN / 4 + c4b];
                    const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
                    const float sv[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        const float t = fmaf(rin[i][j], av[j], sv[j]);
                        // silu(t) = t / (1 + e^-t): v_exp_f32 + v_rcp_f32 (<= ~2 ulp; the operands are rounded to 16 bits next)
                        v[j] = smask[i] != 0.0f ? t * __builtin_amdgcn_rcpf(1.0f + __expf(-t)) : 0.0f;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[j] = rin[i][j] * smask[i];
                }
#if MDT_OPERAND_F16
                u32x4 hi;
                cvt8h(v, hi);
                if (tid + 512 * i < IN_REC_) dst[tid + 512 * i] = hi;
#else
                u32x4 hi, lo;
                split8(v, hi, lo);
                if (tid + 512 * i < IN_REC_) {
                    dst[tid + 512 * i] = hi;
                    dst[IN_REC_ + tid + 512 * i] = lo;
                }
#endif
            }
        }
    };
    const u32x4* wsrc = P.w + (size_t)cb * P.NK * 3 * W_REC;
    auto load_weights = [&](int ph) {    // phase ph = k*3 + dy: one contiguous chunk of W_REC records (-> LDS stage ph & 1)
        const u32x4* src = wsrc + (size_t)ph * W_REC;
#pragma unroll
        for (int i = 0; i < NWREG; ++i)
            if (wave_u * 64 + 512 * i < W_REC) {   // W_REC is a multiple of 64: whole waves
                if (WDMA)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + tid + 512 * i),
                                                     (__attribute__((address_space(3))) void*)(w_l + (ph % WST) * W_REC + wave_u * 64 + 512 * i), 16, 0, 0);
                else
                    rwt[WDMA ? 0 : i] = src[tid + 512 * i];
            }
    };
    auto store_weights = [&](int stage) {
        if (WDMA) {
            __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's part of the chunk has landed (the barrier covers the others)
            return;
        }
        u32x4* dst = w_l + stage * W_REC;
#pragma unroll
        for (int i = 0; i < NWREG; ++i)
            if (wave_u * 64 + 512 * i < W_REC) dst[tid + 512 * i] = rwt[WDMA ? 0 : i];
    };

    f32x16 acc[2][NROW];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NROW; ++n)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[m][n][q] = 0.0f;

    const int nph = P.NK * 3;
    load_input(0);
    load_weights(0);
    store_input(0, 0);
    store_weights(0);
    __syncthreads();

    for (int ph = 0; ph < nph; ++ph) {
        const int k = ph / 3, dy = ph - 3 * k;
        if (dy == 0 && k + 1 < P.NK) load_input(k + 1);
        if (ph + 1 < nph) load_weights(ph + 1);

        const u32x4* wst = w_l + (ph % WST) * W_REC;
        const u32x4* ist = in_l + (IB1 ? 0 : (k & 1)) * IN_STAGE;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            MDT_FRAG a[2][2];   // [m][hl]
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int hl = 0; hl < NHL; ++hl) {
                    a[m][hl] = __builtin_bit_cast(MDT_FRAG, wst[((hl * 3 + dx) * MT + wm * 2 + m) * 64 + lane]);
                }
            if (TERM_MAJOR) {
                MDT_FRAG bh[NROW], bl[NROW];
#pragma unroll
                for (int n = 0; n < NROW; ++n) {
                    const int rec = S == 1 ? (kg * ROWS_ + wr * NROW + n + dy) * COLS + l31 + dx
                                           : (kg * ROWS_ + 2 * (wr * NROW + n) + dy) * COLSL + (dx & 1) * HCOL + l31 + (dx >> 1);
                    bh[n] = __builtin_bit_cast(MDT_FRAG, ist[rec]);
                    bl[n] = NT == 3 ? __builtin_bit_cast(MDT_FRAG, ist[IN_REC_ + rec]) : bh[n];
                }
#pragma unroll
                for (int t = 3 - NT; t < 3; ++t) {
#pragma unroll
                    for (int n = 0; n < NROW; ++n)
#pragma unroll
                        for (int m = 0; m < 2; ++m)
                            acc[m][n] = MDT_MFMA(a[m][t == 0 ? 1 : 0], t == 1 ? bl[n] : bh[n], acc[m][n], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0x07F7);   // everything but MFMAs may cross: keeps the term-major order
                }
            } else {
#pragma unroll
                for (int n = 0; n < NROW; ++n) {
                    const int rec = S == 1 ? (kg * ROWS_ + wr * NROW + n + dy) * COLS + l31 + dx
                                           : (kg * ROWS_ + 2 * (wr * NROW + n) + dy) * COLSL + (dx & 1) * HCOL + l31 + (dx >> 1);
                    const MDT_FRAG bh = __builtin_bit_cast(MDT_FRAG, ist[rec]), bl = NT == 3 ? __builtin_bit_cast(MDT_FRAG, ist[IN_REC_ + rec]) : bh;
#pragma unroll
                    for (int m = 0; m < 2; ++m) {
                        if constexpr (NT == 3) {
                            acc[m][n] = MDT_MFMA(a[m][1], bh, acc[m][n], 0, 0, 0);   // w_lo * x_hi
                            acc[m][n] = MDT_MFMA(a[m][0], bl, acc[m][n], 0, 0, 0);   // w_hi * x_lo
                        }
                        acc[m][n] = MDT_MFMA(a[m][0], bh, acc[m][n], 0, 0, 0);   // w_hi * x_hi
                    }
                }
            }
        }

        if (ph + 1 < nph) store_weights((ph + 1) & 1);
        if (dy == 2 && k + 1 < P.NK) {
            if (IB1) __syncthreads();      // single input stage: every wave must be done reading K-step k before it is overwritten
            store_input(IB1 ? 0 : ((k + 1) & 1), k + 1);
        }
        __syncthreads();
    }

    // ---- epilogue: + bias (+ residual), store NCHW.  C/D layout of a 32x32 MFMA: col = lane & 31, row = (q&3) + 8*(q>>2) + 4*(lane>>5)
    // (128-byte runs along x per register).  All loads of a tile are issued before the first store.
    const size_t HW = (size_t)P.H * P.W;
    const int x = x0 + l31;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int cbase = cb * BM + (wm * 2 + m) * 32 + 4 * kg;
        float bq[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int co = cbase + (q & 3) + 8 * (q >> 2);
            bq[q] = P.bias ? P.bias[co < P.Cout ? co : P.Cout - 1] : 0.0f;
        }
        float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};   // ST: this lane's part of the four quads of the tile (rows 8 j + 4 kg ..)
#pragma unroll
        for (int n = 0; n < NROW; ++n) {
            const int y = y0 + wr * NROW + n;
            if (y < P.H && x < P.W) {
                const size_t o0 = ((size_t)b * P.Cout) * HW + (size_t)y * P.W + x;
                float rq[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int co = cbase + (q & 3) + 8 * (q >> 2);
                    rq[q] = P.res ? P.res[o0 + (size_t)(co < P.Cout ? co : P.Cout - 1) * HW] : 0.0f;
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int co = cbase + (q & 3) + 8 * (q >> 2);
                    const float v = acc[m][n][q] + bq[q] + rq[q];
                    if (co < P.Cout) P.y[o0 + (size_t)co * HW] = v;
                    if (ST) {                  // (the launcher only takes Cout % BM == 0 here: every cout of the block exists)
                        s1[q >> 2] += v;
                        s2[q >> 2] = fmaf(v, v, s2[q >> 2]);
                    }
                }
            }
        }
        if (ST) {
            // a lane's fp32 sums cover 2 rows x 4 couts; from here on fp64 (an fp32 tree over the block would round at 1e-7 of the BLOCK's sum
            // of squares, which var = E[x^2] - mean^2 amplifies by mean^2 / var).  The 32 pixels of a row sit in the 32 lanes of a
            // half-wave: xor offsets < 32 stay inside it.
            double d1[4], d2[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                d1[j] = (double)s1[j];
                d2[j] = (double)s2[j];
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) {
                    d1[j] += __shfl_xor(d1[j], off, 64);
                    d2[j] += __shfl_xor(d2[j], off, 64);
                }
            }
            if (l31 == 0) {
                double2* sl = reinterpret_cast<double2*>(smem);      // the K loop ended behind a barrier: the operand stages are free
#pragma unroll
                for (int j = 0; j < 4; ++j) sl[wr * (BM / 4) + (wm * 2 + m) * 8 + 2 * j + kg] = make_double2(d1[j], d2[j]);
            }
        }
    }
    if (ST) {
        __syncthreads();
        if (tid < BM / 2) {            // (quad, sum | sum of squares): the row groups of the block in a fixed order
            const double* sl = reinterpret_cast<const double*>(smem);
            double t = 0.0;
#pragma unroll
            for (int r = 0; r < WAVES_R; ++r) t += sl[r * (BM / 2) + tid];
            P.gn_part[(((size_t)b * P.ptiles + ptile) * P.NCB + cb) * (BM / 2) + tid] = t;
        }
    }
}
