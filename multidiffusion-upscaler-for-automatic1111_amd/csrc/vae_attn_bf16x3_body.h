// Body of k_attn_bf16x3 / k_attn_bf16x1 (csrc/vae_attn_bf16x3.hip includes this file twice, the way vae_conv_rec.hip shares its bodies):
//   MDT_AT_TERMS = 3: the three-term kernel; = 1: MDTILE_PRECISION_BF16, QK^T and P.V on the hi halves only (K_hi x Q_hi, V_hi x P_hi).
//   The slab DMA, the barriers and their waits are the three-term kernel's (lo planes staged as before); the one-term form reads only
//   the hi fragments and loads only the hi V^T fragments.
template <int C>
__global__ __launch_bounds__(512, 2) void MDT_AT_KERNEL(const u32x4* __restrict__ Qr, const u32x4* __restrict__ Kr, const u32x4* __restrict__ Vr,
                                                        float* __restrict__ out, int T, int T128, int Tk, int Tk128, float scale, int nsplit,
                                                        float* __restrict__ part, float* __restrict__ pstat) {
    constexpr int NTERM = MDT_AT_TERMS, NHL = NTERM == 3 ? 2 : 1;   // products per MFMA site (3: lo x hi, hi x lo, hi x hi; 1: hi x hi), planes read
    // T / T128: QUERY tokens (rows of the output); Tk / Tk128: KEY tokens.  They differ only when a row band of the queries
    // attends to keys / values gathered from every band (sequence-parallel estimator, mdtile/seqpar.py).
    constexpr int NKS = C / 16, NMT = C / 32, KSS = 4, NSS = NKS / KSS;     // channel k-steps, 32-channel output tiles, k-steps / slab, slabs
    constexpr int WAVES_M = NMT < 8 ? NMT : 8, WAVES_N = 8 / WAVES_M, MT_W = NMT / WAVES_M, NT_W = 4 / WAVES_N;
    constexpr int HALF_REC = 4 * KSS * 2 * 64;                              // K (or Q) part of a slab: [tile 4][ks][hl][lane]
    constexpr int STAGE_REC = 2 * HALF_REC;                                 // 4096 records = 64 KB = exactly the P records of a key block
    static_assert(NSS >= 2 && NSS % 2 == 0 && STAGE_REC == P_REC, "slab sizing");
    __shared__ u32x4 smem[2 * STAGE_REC + STAT_FLOATS / 4];
    u32x4* const slab = smem;
    float* const smax = reinterpret_cast<float*>(smem + 2 * STAGE_REC);
    float* const ssum = smax + 4 * BQ;
    float* const salpha = ssum + 4 * BQ;

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, kg = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kt_w = wave >> 1, qh = wave & 1;                      // score phase: key tile, query-tile pair
    const int wm = wave % WAVES_M, wn = wave / WAVES_M;             // output phase: channel tiles, query tiles
    // block -> (query block, key split), XCD-aware: workgroups go to XCDs round-robin (id % 8), so the `nsplit` key ranges of one
    // query block are handed to consecutive slots of ONE XCD: the Q records every key block re-streams stay in that XCD's L2.
    const int b = blockIdx.y;
    const int bid = blockIdx.x, bxcd = bid & 7, bslot = bid >> 3;
    const int qb = (bslot / nsplit) * 8 + bxcd;
    const int split = bslot - (bslot / nsplit) * nsplit;
    if (qb * BQ >= T128) return;
    const int tiles = T128 / 32, ktiles = Tk128 / 32, groups = Tk128 / 16, nkb = Tk128 / BK;
    const u32x4* Qb = Qr + (size_t)b * tiles * NKS * 128 + (size_t)qb * 4 * NKS * 128;
    const u32x4* Kb = Kr + (size_t)b * ktiles * NKS * 128;
    const u32x4* Vb = Vr + (size_t)b * groups * NMT * 128;

    // slab s of key block kb -> stage: 8 DMA pieces per wave (4 K + 4 Q); piece i covers records [512 (wave/2*... see below)
    // source of tile t, slab s: KSS * 2 * 64 = 512 contiguous records at ((t * NKS + KSS * s) * 128); a wave-instruction moves 64
    // of them: piece index d in [0, 32) of a half -> tile d >> 3, records (d & 7) * 64 .. + 64
    const unsigned lane16 = lane * 16;
    auto issue_S = [&](int kb, int s, int stage) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int half = i >> 2;                     // 0: K, 1: Q (compile-time)
            const int d = wave * 4 + (i & 3);            // 0 .. 31
            const int t4 = d >> 3, off = (d & 7) * 64;
            const u32x4* src = (half == 0 ? Kb + ((size_t)(kb * 4 + t4) * NKS + KSS * s) * 128 : Qb + ((size_t)t4 * NKS + KSS * s) * 128) + off;
            dma16a(src, lane16, slab + stage * STAGE_REC + half * HALF_REC + d * 64);
        }
    };

    f32x16 acc_o[MT_W][NT_W];
#pragma unroll
    for (int m = 0; m < MT_W; ++m)
#pragma unroll
        for (int n = 0; n < NT_W; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_o[m][n][r] = 0.0f;
    float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.0f, 0.0f};   // for queries (2*qh + j)*32 + l31

    // key-range split: each part keeps its own running (max, sum) and an un-normalised output; k_attn_combine merges them
    const int kb_lo = (int)((long long)nkb * split / nsplit), kb_hi = (int)((long long)nkb * (split + 1) / nsplit);
    int base = 0;                                  // stage of slab 0 of the current key block; slab s sits in stage (base + s) & 1
    issue_S(kb_lo, 0, 0);
    for (int kb = kb_lo; kb < kb_hi; ++kb) {
        // ------------------------------------------------ scores: St tiles (kt_w, 2*qh + j), all channels
        f32x16 st[2];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) st[j][r] = 0.0f;
        bf16x8 fa[2][2], fb[2][2][2];              // [set][hl], [set][j][hl]
#pragma unroll 1
        for (int s = 0; s < NSS; ++s) {
            const int stage = (base + s) & 1;
            __builtin_amdgcn_s_waitcnt(0x0F70);    // vmcnt(0): this wave's pieces of slab s have landed
            asm volatile("" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            // the other stage is free now (slab s-1 / the previous block's P are consumed by every wave): next slab goes out.
            // Staggered between the two waves of a SIMD (w, w + 4): waves 0-3 issue their 8 pieces right behind the barrier, waves 4-7
            // after their first k-step's MFMAs -- one of the pair always feeds the matrix pipe.
            if (s + 1 < NSS && wave < 4) issue_S(kb, s + 1, stage ^ 1);
            const u32x4* ka = slab + stage * STAGE_REC + (kt_w * KSS * 2) * 64 + lane;
            const u32x4* qa = slab + stage * STAGE_REC + HALF_REC + (2 * qh * KSS * 2) * 64 + lane;
            auto load_ks = [&](int set, int ks) {
#pragma unroll
                for (int hl = 0; hl < NHL; ++hl) {
                    fa[set][hl] = __builtin_bit_cast(bf16x8, ka[(ks * 2 + hl) * 64]);
#pragma unroll
                    for (int j = 0; j < 2; ++j) fb[set][j][hl] = __builtin_bit_cast(bf16x8, qa[((j * KSS + ks) * 2 + hl) * 64]);
                }
            };
            load_ks(0, 0);
#pragma unroll
            for (int ks = 0; ks < KSS; ++ks) {
                const int set = ks & 1;
                MDT_PIN();
                if (ks + 1 < KSS) load_ks(set ^ 1, ks + 1);
                MDT_PIN();
#pragma unroll
                for (int term = 3 - NTERM; term < 3; ++term)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        st[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[set][term == 0 ? 1 : 0], fb[set][j][term == 1 ? 1 : 0], st[j], 0, 0, 0);
                MDT_PIN();
                if (ks == 0 && s + 1 < NSS && wave >= 4) issue_S(kb, s + 1, stage ^ 1);
            }
        }
        // ------------------------------------------------ V^T fragments of the first two 16-key steps go out now (latency under the softmax)
        const u32x4* vsrc = Vb + ((size_t)kb * 8 * NMT + wm * MT_W) * 128 + lane;      // + p * NMT * 128 + (m * 2 + hl) * 64
        u32x4 fv[3][MT_W][2];
        auto load_v = [&](int set, int p) {
#pragma unroll
            for (int m = 0; m < MT_W; ++m)
#pragma unroll
                for (int hl = 0; hl < NHL; ++hl) fv[set][m][hl] = vsrc[(size_t)p * NMT * 128 + (m * 2 + hl) * 64];
        };
        load_v(0, 0);
        load_v(1, 1);
        // ------------------------------------------------ online softmax (lane = query column, 16 keys of tile kt_w per j)
        // (scores are kept in the log2 domain: s' = s * scale * log2(e), so that exp(s - m) = exp2(s' - m') is one v_exp_f32)
        const int key0 = kb * BK + kt_w * 32 + 4 * kg;
        const float scale2 = scale * 1.4426950408889634f;
        const bool ragged = (kb + 1) * BK > Tk;          // only the last key block holds padded keys
        float mx[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float m = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float sv = st[j][r] * scale2;
                if (ragged && key0 + (r & 3) + 8 * (r >> 2) >= Tk) sv = -INFINITY;
                st[j][r] = sv;
                m = fmaxf(m, sv);
            }
            m = fmaxf(m, __shfl_xor(m, 32, 64));
            mx[j] = m;
            if (kg == 0) smax[kt_w * BQ + (2 * qh + j) * 32 + l31] = m;
        }
        // raw barrier + lgkmcnt(0) only: __syncthreads() would also drain vmcnt, i.e. the V^T prefetch just issued (and, further
        // down, the next slab's DMA).  (Also: every wave is done with the last slab.)
        __builtin_amdgcn_s_waitcnt(0xC07F);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // the stage of the last slab is free: the next key block's slab 0 goes there and lands under the softmax + output phase
        if (kb + 1 < kb_hi) issue_S(kb + 1, 0, base ^ 1);
        u32x4* const p_l = slab + base * STAGE_REC;  // P records of this key block: the stage slab NSS-2 sat in
        float alpha[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = (2 * qh + j) * 32 + l31;
            const float m_blk = fmaxf(fmaxf(smax[q], smax[BQ + q]), fmaxf(smax[2 * BQ + q], smax[3 * BQ + q]));
            const float m_new = fmaxf(m_run[j], m_blk);      // finite: every key block holds >= 1 valid key
            alpha[j] = __builtin_amdgcn_exp2f(m_run[j] - m_new);   // exp2(-inf) = 0 on the first block
            m_run[j] = m_new;
            float ps = 0.0f;
            float pv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                pv[r] = __builtin_amdgcn_exp2f(st[j][r] - m_new);   // masked keys: exp2(-inf) = 0
                ps += pv[r];
            }
            ps += __shfl_xor(ps, 32, 64);
            if (kg == 0) {
                ssum[kt_w * BQ + q] = ps;
                if (kt_w == 0) salpha[q] = alpha[j];
            }
            // P records for the output MFMAs: k-step (kt_w*2 + s2) of this key block, query tile 2*qh + j.
            // register r = 8*s2 + i  <->  key 16*s2 + (i & 3) + 8*(i >> 2) + 4*kg of the tile == the Vrec key order.
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                float v8[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) v8[i] = pv[8 * s2 + i];
                u32x4 hi, lo;
                split8v(v8, hi, lo);
                u32x4* d = p_l + (((kt_w * 2 + s2) * 4 + (2 * qh + j)) * 2) * 64;
                d[lane] = hi;
                d[64 + lane] = lo;
            }
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);          // lgkmcnt(0): P records and the partial sums are written
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int q = (2 * qh + j) * 32 + l31;
            l_run[j] = l_run[j] * alpha[j] + ((ssum[q] + ssum[BQ + q]) + (ssum[2 * BQ + q] + ssum[3 * BQ + q]));
        }
        // ------------------------------------------------ output: rescale, then Ot += V^T P^T over the 128 keys (no barrier inside)
        {
            // the running maximum of a query settles after a few key blocks: when no query of this wave's tiles moved (alpha == 1
            // everywhere) the MT_W * NT_W * 16 multiplies are skipped (wave-uniform branch)
            float an[NT_W];
            bool moved = false;
#pragma unroll
            for (int n = 0; n < NT_W; ++n) {
                an[n] = salpha[(wn * NT_W + n) * 32 + l31];
                moved = moved || an[n] != 1.0f;
            }
            if (__any(moved)) {
#pragma unroll
                for (int n = 0; n < NT_W; ++n)
#pragma unroll
                    for (int m = 0; m < MT_W; ++m)
#pragma unroll
                        for (int r = 0; r < 16; ++r) acc_o[m][n][r] *= an[n];
            }
        }
        constexpr int HN = NT_W >= 2 ? NT_W / 2 : 1, NH = NT_W / HN;     // query tiles per half-step, half-steps per 16-key step
        bf16x8 fp[2][HN][2];                                              // [set][n][hl]
        auto load_p = [&](int set, int p, int h) {
#pragma unroll
            for (int n = 0; n < HN; ++n)
#pragma unroll
                for (int hl = 0; hl < NHL; ++hl)
                    fp[set][n][hl] = __builtin_bit_cast(bf16x8, p_l[((p * 4 + wn * NT_W + h * HN + n) * 2 + hl) * 64 + lane]);
        };
        load_p(0, 0, 0);
#pragma unroll
        for (int p = 0; p < 8; ++p) {
            const int vs = p % 3;
            if (p + 2 < 8) load_v((p + 2) % 3, p + 2);
#pragma unroll
            for (int h = 0; h < NH; ++h) {
                const int t = p * NH + h, ps_ = t & 1;
                MDT_PIN();
                if (t + 1 < 8 * NH) load_p(ps_ ^ 1, (t + 1) / NH, (t + 1) % NH);
                MDT_PIN();
#pragma unroll
                for (int term = 3 - NTERM; term < 3; ++term)
#pragma unroll
                    for (int n = 0; n < HN; ++n)
#pragma unroll
                        for (int m = 0; m < MT_W; ++m)
                            acc_o[m][h * HN + n] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                                __builtin_bit_cast(bf16x8, fv[vs][m][term == 0 ? 1 : 0]), fp[ps_][n][term == 1 ? 1 : 0], acc_o[m][h * HN + n], 0, 0, 0);
                MDT_PIN();
            }
        }
        base ^= 1;
    }

    // ---------------------------------------------------- normalise by the softmax denominator and store [B, C, T]
    __syncthreads();
    if (kt_w == 0 && kg == 0) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ql = (2 * qh + j) * 32 + l31;
            ssum[ql] = l_run[j];
            if (nsplit > 1) {   // (max, sum) of this part, per query: pstat[split][b][2][T128]
                float* ps = pstat + ((size_t)(split * gridDim.y + b) * 2) * T128 + qb * BQ + ql;
                ps[0] = m_run[j];
                ps[T128] = l_run[j];
            }
        }
    }
    __syncthreads();
    if (nsplit > 1) {
        float* ob = part + (size_t)(split * gridDim.y + b) * C * T;   // un-normalised part, same [C][T] layout as out
#pragma unroll
        for (int n = 0; n < NT_W; ++n) {
            const int q = qb * BQ + (wn * NT_W + n) * 32 + l31;
            if (q < T) {
#pragma unroll
                for (int m = 0; m < MT_W; ++m)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int c = (wm * MT_W + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                        ob[(size_t)c * T + q] = acc_o[m][n][r];
                    }
            }
        }
        return;
    }
    float* ob = out + (size_t)b * C * T;
#pragma unroll
    for (int n = 0; n < NT_W; ++n) {
        const int ql = (wn * NT_W + n) * 32 + l31;
        const int q = qb * BQ + ql;
        const float inv = 1.0f / ssum[ql];
        if (q < T) {
#pragma unroll
            for (int m = 0; m < MT_W; ++m)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = (wm * MT_W + m) * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
                    ob[(size_t)c * T + q] = acc_o[m][n][r] * inv;
                }
        }
    }
}
