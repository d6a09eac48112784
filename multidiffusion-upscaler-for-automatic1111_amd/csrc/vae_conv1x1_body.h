// Body of k_conv1x1_bf16x3 / k_conv1x1_bf16x1 (csrc/vae_conv1x1_bf16x3.hip includes this file twice, the way vae_conv_rec.hip shares its bodies):
//   MDT_C1_TERMS = 3: the three-term kernel; = 1: MDTILE_PRECISION_BF16, w_hi x x_hi only.  The one-term form stages both planes of its input as
//   before; it reads only the hi fragments.
template <int MT, int PXT>
__global__ __launch_bounds__(512, PXT == 128 ? 4 : 2) void MDT_C1_KERNEL(const Conv1Params P) {
    constexpr int NT = MDT_C1_TERMS, NHL = NT == 3 ? 2 : 1;   // products per MFMA site (3: w_lo x_hi, w_hi x_lo, w_hi x_hi; 1: w_hi x_hi), weight planes read
    constexpr int BM = MT * 32;
    constexpr int IN_REC1 = 2 * 2 * PXT;             // records per hl per stage: [ks][kg][px]
    constexpr int NG = PXT / 128;                    // 8-channel groups a thread stages per phase (512 threads x NG = 4 groups x PXT px)
    constexpr int WAVES_M = MT / 2, WAVES_C = 8 / WAVES_M, NCOL = (PXT / 32) / WAVES_C;   // column tiles (32 px) per wave
    static_assert(NCOL >= 1 && NG >= 1, "block shape");
    constexpr int W_REC = 2 * 2 * MT * 64;           // [hl][ks][mt][lane]
    constexpr int NWREG = W_REC / 512;               // 4 (MT = 8), 2 (MT = 4) or 1 (MT = 2)
    constexpr int IN_STAGE = 2 * IN_REC1;
    __shared__ u32x4 smem[2 * IN_STAGE + 2 * W_REC];
    u32x4* const in_l = smem;
    u32x4* const w_l = smem + 2 * IN_STAGE;

    const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
    const int ptile = (slot / P.NCB) * 8 + xcd, cb = slot % P.NCB;
    if (ptile >= P.ptiles) return;
    const int b = blockIdx.y;
    const size_t p0 = (size_t)ptile * PXT;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kg = lane >> 5;
    const int wm = wave % WAVES_M, wc = wave / WAVES_M;
    const float* xb = P.x + (size_t)b * P.Cin * P.HW;

    // staging map: thread -> pixel (tid % PXT) and NG consecutive 8-channel groups gi = (tid / PXT) * NG + g of the phase's four
    // (gi = 2 * K-step + kg: channels 32 ph + 8 gi + j, LDS record gi * PXT + px)
    const int spx = tid & (PXT - 1), sgb = (tid / PXT) * NG;
    const bool pin = p0 + spx < P.HW;
    const size_t soff = pin ? p0 + spx : 0;
    float rin[2][NG][8];         // [register set][8-channel group][channel]
    u32x4 rwt[2][NWREG];

    auto load_input = [&](int set, int ph) {       // phase ph: channels 32 ph .. 32 ph + 31
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const float* src = xb + (size_t)(ph * 32 + (sgb + g) * 8) * P.HW + soff;
#pragma unroll
            for (int j = 0; j < 8; ++j) rin[set][g][j] = src[(size_t)j * P.HW];
        }
    };
    auto store_input = [&](int set, int stage) {
        u32x4* dst = in_l + stage * IN_STAGE;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = pin ? rin[set][g][j] : 0.0f;
            u32x4 hi, lo;
            split8c(v, hi, lo);
            const int rec = (sgb + g) * PXT + spx;
            dst[rec] = hi;
            dst[IN_REC1 + rec] = lo;
        }
    };
    const u32x4* wsrc = P.w + (size_t)cb * P.NP * W_REC;
    auto load_weights = [&](int set, int ph) {
        const u32x4* src = wsrc + (size_t)ph * W_REC;
#pragma unroll
        for (int i = 0; i < NWREG; ++i) rwt[set][i] = src[tid + 512 * i];
    };
    auto store_weights = [&](int set, int stage) {
        u32x4* dst = w_l + stage * W_REC;
#pragma unroll
        for (int i = 0; i < NWREG; ++i) dst[tid + 512 * i] = rwt[set][i];
    };

    f32x16 acc[2][NCOL];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NCOL; ++n)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[m][n][q] = 0.0f;

    load_input(0, 0);
    load_weights(0, 0);
    if (P.NP > 1) {
        load_input(1, 1);
        load_weights(1, 1);
    }
    store_input(0, 0);
    store_weights(0, 0);
    __syncthreads();

    // phase ph sits in LDS stage ph & 1 and came through register set ph & 1; while it computes, phase ph + 2 is requested into the
    // same register set (free since its contents went to LDS) and phase ph + 1 -- requested a whole phase ago -- is written to LDS
    // behind the MFMAs.  Two phases per trip keep the register-set index a compile-time constant.
    auto phase = [&](int ph, auto set_tag) {
        constexpr int set = decltype(set_tag)::value;
        if (ph + 2 < P.NP) {
            load_input(set, ph + 2);
            load_weights(set, ph + 2);
        }
        const u32x4* wst = w_l + set * W_REC;
        const u32x4* ist = in_l + set * IN_STAGE;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 a[2][2];   // [m][hl]
#pragma unroll
            for (int m = 0; m < 2; ++m)
#pragma unroll
                for (int hl = 0; hl < NHL; ++hl)
                    a[m][hl] = __builtin_bit_cast(bf16x8, wst[((hl * 2 + ks) * MT + wm * 2 + m) * 64 + lane]);
#pragma unroll
            for (int n = 0; n < NCOL; ++n) {
                const int rec = (ks * 2 + kg) * PXT + (wc * NCOL + n) * 32 + l31;
                const bf16x8 bh = __builtin_bit_cast(bf16x8, ist[rec]), bl = NT == 3 ? __builtin_bit_cast(bf16x8, ist[IN_REC1 + rec]) : bh;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    if constexpr (NT == 3) {
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m][1], bh, acc[m][n], 0, 0, 0);   // w_lo * x_hi
                        acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m][0], bl, acc[m][n], 0, 0, 0);   // w_hi * x_lo
                    }
                    acc[m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[m][0], bh, acc[m][n], 0, 0, 0);   // w_hi * x_hi
                }
            }
        }
        if (ph + 1 < P.NP) {
            store_weights(set ^ 1, set ^ 1);
            store_input(set ^ 1, set ^ 1);
        }
        __syncthreads();
    };
    for (int ph = 0; ph < P.NP; ph += 2) {
        phase(ph, std::integral_constant<int, 0>{});
        if (ph + 1 < P.NP) phase(ph + 1, std::integral_constant<int, 1>{});
    }

    // epilogue: + bias (+ residual).  C/D layout of a 32x32 MFMA: col = lane & 31, row = (q&3) + 8*(q>>2) + 4*(lane>>5)
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        const int cbase = cb * BM + (wm * 2 + m) * 32 + 4 * kg;
        float bq[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int co = cbase + (q & 3) + 8 * (q >> 2);
            bq[q] = P.bias ? P.bias[co < P.Cout ? co : P.Cout - 1] : 0.0f;
        }
#pragma unroll
        for (int n = 0; n < NCOL; ++n) {
            const size_t p = p0 + (wc * NCOL + n) * 32 + l31;
            if (p < P.HW) {
                const size_t o0 = ((size_t)b * P.Cout) * P.HW + p;
                float rq[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int co = cbase + (q & 3) + 8 * (q >> 2);
                    rq[q] = P.res ? P.res[o0 + (size_t)(co < P.Cout ? co : P.Cout - 1) * P.HW] : 0.0f;
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int co = cbase + (q & 3) + 8 * (q >> 2);
                    if (co < P.Cout) P.y[o0 + (size_t)co * P.HW] = acc[m][n][q] + bq[q] + rq[q];
                }
            }
        }
    }
}
