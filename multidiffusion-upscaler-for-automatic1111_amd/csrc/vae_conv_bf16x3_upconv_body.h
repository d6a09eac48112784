// Body of k_upconv_bf16x3 / k_upconv_bf16x1 (csrc/vae_conv_bf16x3.hip includes this file twice, the way vae_conv_rec.hip shares its bodies):
//   MDT_B3_TERMS = 3: the three-term kernel; = 1: MDTILE_PRECISION_BF16, w_hi x x_hi only.  The one-term form still splits and stages both
//   planes of its input (the LDS images and the load / store schedule are the three-term kernel's); it reads only the hi fragments.
template <int MT>
__global__ __launch_bounds__(512) void MDT_B3_KERNEL(const ConvBParams P) {
    constexpr int NT = MDT_B3_TERMS, NHL = NT == 3 ? 2 : 1;   // products per MFMA site (3: w_lo x_hi, w_hi x_lo, w_hi x_hi; 1: w_hi x_hi), weight planes read
    constexpr int BM = MT * 32;
    constexpr int WAVES_M = MT / 2, WAVES_R = 8 / WAVES_M, NROW = TH / WAVES_R;
    constexpr int W_REC = 2 * 2 * 2 * MT * 64;          // [hl][b][v][mt][lane] records per (a, cb, k, u) chunk
    constexpr int NWREG = W_REC / 512;                   // 4 (MT = 4) or 2 (MT = 2)
    constexpr int IN_STAGE = 2 * IN_REC;
    __shared__ u32x4 smem[2 * IN_STAGE + 2 * W_REC];
    u32x4* const in_l = smem;
    u32x4* const w_l = smem + 2 * IN_STAGE;

    // block -> (input pixel tile, cout block, row parity); XCD = id % 8 keeps every (cb, a) of a pixel tile on one L2
    const int id = blockIdx.x, xcd = id & 7, slot = id >> 3;
    const int per = P.NCB * 2;
    const int ptile = (slot / per) * 8 + xcd, rem = slot % per, cb = rem >> 1, a = rem & 1;
    if (ptile >= P.ptiles) return;
    const int b = blockIdx.y;
    const int py = ptile / P.PX, px = ptile - py * P.PX;
    const int y0 = py * TH, x0 = px * TW;              // INPUT coordinates

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kg = lane >> 5;
    const int wm = wave % WAVES_M, wr = wave / WAVES_M;
    const size_t HWin = (size_t)P.Hin * P.Win;
    const float* xb = P.x + (size_t)b * P.Cin * HWin;

    const int wave_u = __builtin_amdgcn_readfirstlane(wave);
    const bool has_rec1 = wave_u * 64 + 512 < IN_REC;
    int soff[2], scg[2];
    float smask[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        int s = tid + 512 * i;
        if (s >= IN_REC) s = IN_REC - 1;
        const int cg = s / (ROWS * COLS), p = s - cg * (ROWS * COLS);
        const int r = p / COLS, c = p - r * COLS;
        const int gy = y0 + r - 1, gx = x0 + c - 1;
        const bool inside = gy >= 0 && gy < P.Hin && gx >= 0 && gx < P.Win;
        scg[i] = cg;
        soff[i] = inside ? gy * P.Win + gx : 0;
        smask[i] = inside ? 1.0f : 0.0f;
    }
    float rin[2][8];
    u32x4 rwt[NWREG];

    auto load_input = [&](int k) {
        {
            const float* src = xb + (size_t)kstep_c0(k, scg[0], P.perm) * HWin + soff[0];
#pragma unroll
            for (int j = 0; j < 8; ++j) rin[0][j] = src[(size_t)kstep_cj(j, P.perm) * HWin];
        }
        if (has_rec1) {
            const float* src = xb + (size_t)kstep_c0(k, scg[1], P.perm) * HWin + soff[1];
#pragma unroll
            for (int j = 0; j < 8; ++j) rin[1][j] = src[(size_t)kstep_cj(j, P.perm) * HWin];
        }
    };
    auto store_input = [&](int stage) {
        u32x4* dst = in_l + stage * IN_STAGE;
        {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = rin[0][j] * smask[0];
            u32x4 hi, lo;
            split8(v, hi, lo);
            dst[tid] = hi;
            dst[IN_REC + tid] = lo;
        }
        if (has_rec1) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = rin[1][j] * smask[1];
            u32x4 hi, lo;
            split8(v, hi, lo);
            if (tid + 512 < IN_REC) {
                dst[tid + 512] = hi;
                dst[IN_REC + tid + 512] = lo;
            }
        }
    };
    const int nph = P.NK * 2;
    const u32x4* wsrc = P.w + ((size_t)a * P.NCB + cb) * nph * W_REC;
    auto load_weights = [&](int ph) {
        const u32x4* src = wsrc + (size_t)ph * W_REC;
#pragma unroll
        for (int i = 0; i < NWREG; ++i) rwt[i] = src[tid + 512 * i];
    };
    auto store_weights = [&](int stage) {
        u32x4* dst = w_l + stage * W_REC;
#pragma unroll
        for (int i = 0; i < NWREG; ++i) dst[tid + 512 * i] = rwt[i];
    };

    f32x16 acc[2][2][NROW];   // [b][m][n]
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int n = 0; n < NROW; ++n)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc[bb][m][n][q] = 0.0f;

    load_input(0);
    load_weights(0);
    store_input(0);
    store_weights(0);
    __syncthreads();

    for (int ph = 0; ph < nph; ++ph) {
        const int k = ph >> 1, u = ph & 1;
        if (u == 0 && k + 1 < P.NK) load_input(k + 1);
        if (ph + 1 < nph) load_weights(ph + 1);

        const u32x4* wst = w_l + (ph & 1) * W_REC;
        const u32x4* ist = in_l + (k & 1) * IN_STAGE;
        const int rbase = kg * ROWS + wr * NROW + a + u;   // halo row of output row n: + n
#pragma unroll
        for (int s = 0; s < 3; ++s) {                      // column shift s = b + v
            bf16x8 bh[NROW], bl[NROW];
#pragma unroll
            for (int n = 0; n < NROW; ++n) {
                const int rec = (rbase + n) * COLS + l31 + s;
                bh[n] = __builtin_bit_cast(bf16x8, ist[rec]);
                bl[n] = NT == 3 ? __builtin_bit_cast(bf16x8, ist[IN_REC + rec]) : bh[n];
            }
#pragma unroll
            for (int bb = 0; bb < 2; ++bb) {
                const int v = s - bb;
                if (v < 0 || v > 1) continue;
#pragma unroll
                for (int m = 0; m < 2; ++m) {
                    const bf16x8 ah = __builtin_bit_cast(bf16x8, wst[(((0 * 2 + bb) * 2 + v) * MT + wm * 2 + m) * 64 + lane]);
                    const bf16x8 al = NT == 1 ? ah : __builtin_bit_cast(bf16x8, wst[(((1 * 2 + bb) * 2 + v) * MT + wm * 2 + m) * 64 + lane]);
#pragma unroll
                    for (int n = 0; n < NROW; ++n) {
                        if constexpr (NT == 3) {
                            acc[bb][m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh[n], acc[bb][m][n], 0, 0, 0);   // w_lo * x_hi
                            acc[bb][m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl[n], acc[bb][m][n], 0, 0, 0);   // w_hi * x_lo
                        }
                        acc[bb][m][n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh[n], acc[bb][m][n], 0, 0, 0);   // w_hi * x_hi
                    }
                }
            }
        }

        if (ph + 1 < nph) store_weights((ph + 1) & 1);
        if (u == 1 && k + 1 < P.NK) store_input((k + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue: + bias (+ residual); lane owns output px (2X, 2X+1) of row 2Y + a: one float2 per cout
    const size_t HW = (size_t)P.H * P.W;
    const int xi = x0 + l31;
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
        for (int n = 0; n < NROW; ++n) {
            const int yi = y0 + wr * NROW + n;
            if (yi < P.Hin && xi < P.Win) {
                const size_t o0 = ((size_t)b * P.Cout) * HW + (size_t)(2 * yi + a) * P.W + 2 * xi;
                float2 rq[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int co = cbase + (q & 3) + 8 * (q >> 2);
                    rq[q] = P.res ? *reinterpret_cast<const float2*>(P.res + o0 + (size_t)(co < P.Cout ? co : P.Cout - 1) * HW)
                                  : make_float2(0.0f, 0.0f);
                }
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int co = cbase + (q & 3) + 8 * (q >> 2);
                    if (co < P.Cout)
                        *reinterpret_cast<float2*>(P.y + o0 + (size_t)co * HW) =
                            make_float2(acc[0][m][n][q] + bq[q] + rq[q].x, acc[1][m][n][q] + bq[q] + rq[q].y);
                }
            }
        }
    }
}
