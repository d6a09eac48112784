// Body of k_conv3x3_rec2 / k_conv3x3_rec2_1t (csrc/vae_conv_rec2.hip includes this file twice, the way vae_conv_rec.hip shares its bodies):
//   MDT_REC2_TERMS = 3: the three-term kernel (w_lo x_hi, w_hi x_lo, w_hi x_hi per product); = 1: MDTILE_PRECISION_BF16, w_hi x x_hi only and
//   only the hi fragments read -- the DMA pieces (lo planes included), ring slots and counted waits of every step are the three-term kernel's.
//   MDT_OPERAND_F16 = 1 (one-term only; k_conv3x3_rec2_f16 / _f16s, MDTILE_PRECISION_F16): fp16 fragments and MFMA; MDT_REC_OUT16 = 1: fp16 record-out epilogue
#include "mfma_operand.h"
template <int MW, int WM, int NROW>
__global__ __launch_bounds__(256, 2) void MDT_REC2_KERNEL(const ConvRParams P) {
    constexpr int NT = MDT_REC2_TERMS, NHL = NT == 3 ? 2 : 1;   // products per MFMA site (3: w_lo x_hi, w_hi x_lo, w_hi x_hi; 1: w_hi x_hi), planes read
    constexpr int WR = NWV / WM, TH = WR * NROW, MT = MW * WM, HN = NROW / 2;
    constexpr int ROWS = TH + 2, COLS = 34;
    using IS = InStage<ROWS, NWV>;
    constexpr int W_STEP = 2 * MT * 64;               // records of a step chunk [hl][mt][lane]
    constexpr int W_PH = 3 * W_STEP;                  // records of a packed phase chunk [hl][dx][mt][lane] (the layout in HBM)
    constexpr int W_PW = W_STEP / 64 / NWV;           // pieces per wave and step
    static_assert(W_STEP / 64 == W_PW * NWV && W_PW == 2, "a step chunk is two pieces per wave");
    static_assert(IS::PW == 6 && IS::DMA > 5 * NWV, "the counted waits below assume five input pieces from every wave (a sixth from some)");
    __shared__ u32x4 smem[2 * IS::PAD + 4 * W_STEP + 2 * EC2];
    u32x4* const in_l = smem;
    u32x4* const w_l = smem + 2 * IS::PAD;
    u32x4* const ec_l = smem + 2 * IS::PAD + 4 * W_STEP;

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, kg = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wr = wave / WM;
    const int Hp = P.H + 2, Wp = rec_pitch(P.W), Pn = P.Cin >> 3;
    const size_t plane = (size_t)Hp * Wp;

    // work -> (sample, pixel tile, cout block): as in k_conv3x3_rec (grid % 8 == 0 => `work % 8` is this block's XCD for all its
    // items: the cout blocks of a pixel tile stay on one L2)
    const int per_img = ((P.ptiles + 7) / 8) * 8 * P.NCB, total = per_img * P.B;
    auto decode = [&](int work, Item2& it) -> bool {
        it.b = work / per_img;
        const int r = work - it.b * per_img, xcd = r & 7, slot = r >> 3;
        const int ptile = (slot / P.NCB) * 8 + xcd;
        it.cb = slot % P.NCB;
        const int py = ptile / P.PX, px = ptile - py * P.PX;
        it.y0 = py * TH;
        it.x0 = px * 32;
        return ptile < P.ptiles;
    };
    auto next_valid = [&](int work, Item2& it) -> int {
        while (work < total && !decode(work, it)) work += gridDim.x;
        return work;
    };

    // input DMA map: piece di = wave + 4 i covers LDS records [64 di, 64 di + 64) of a stage; hl = di / HALF_DMA
    auto make_ioff = [&](const Item2& it, unsigned (&ioff)[IS::PW]) {
        int ln = lane;
        asm volatile("" : "+v"(ln));      // (g, r, c) re-derived per item, as in k_conv3x3_rec: kept across the loop they go to scratch
#pragma unroll
        for (int i = 0; i < IS::PW; ++i) {
            const int di = wave + NWV * i;
            int s = (di % IS::HALF_DMA) * 64 + ln;
            if (s >= IS::HALF) s = IS::HALF - 1;            // pad lanes shadow the last record (they land in the pad area)
            const int g = s / (ROWS * COLS), p = s - g * (ROWS * COLS);
            const int r = p / COLS, c = p - r * COLS;
            int pr = it.y0 + r, pc = it.x0 + c;             // padded coordinates (image row y0 + r - 1, image column x0 + c - 1)
            pr = pr < Hp ? pr : Hp - 1;                     // ragged block edge: clamp onto the zero border
            pc = (pc < P.W + 1 ? pc : P.W + 1) + REC_COL0;  // (column of the record image: the left border sits at REC_COL0)
            ioff[i] = (unsigned)(((size_t)g * plane + (size_t)pr * Wp + pc) * 16);
        }
    };
    auto issue_input_piece = [&](const Item2& it, const unsigned (&ioff)[IS::PW], int k, int stage, int i) {
        const int di = wave + NWV * i;
        if (di < IS::DMA) {
            const char* xb = reinterpret_cast<const char*>(P.x + (size_t)it.b * 2 * Pn * plane);
            const char* base = xb + ((size_t)(di / IS::HALF_DMA) * Pn + 2 * (size_t)k) * plane * 16;   // wave-uniform
            dma16(base, ioff[i], in_l + stage * IS::PAD + di * 64);
        }
    };
    const unsigned lane16 = lane * 16;
    // step chunk (k, dy, dx) of the item's cout block -> ring slot: piece p = wave + 4 i = (hl, m-tile) = (i, wave)
    auto issue_wstep = [&](const Item2& it, int k, int dy, int dx, int slot) {
        const char* wsrc = reinterpret_cast<const char*>(P.w + ((size_t)it.cb * P.NK + k) * 3 * W_PH + (size_t)dy * W_PH);
#pragma unroll
        for (int i = 0; i < W_PW; ++i) {
            const int p = wave + NWV * i, hl = p / MT, j = p % MT;
            dma16(wsrc + (size_t)(((hl * 3 + dx) * MT + j) * 64) * 16, lane16, w_l + slot * W_STEP + p * 64);
        }
    };
    // epilogue constants of an item's 128 couts: waves 0 / 1 / 2 fetch bias / a / s, 512 B each (lanes 0-31)
    auto issue_consts = [&](const Item2& it, int par) {
        if (lane < 32) {
            if (wave == 0 && P.bias) dma16(reinterpret_cast<const char*>(P.bias + it.cb * (MT * 32)), lane16, ec_l + par * EC2);
            if ((wave == 1 || wave == 2) && P.yrec && P.coef)
                dma16(reinterpret_cast<const char*>(P.coef + ((size_t)it.b * 2 + (wave - 1)) * P.Cout + it.cb * (MT * 32)), lane16,
                      ec_l + par * EC2 + wave * 32);
        }
    };

    MDT_FRAG fw[2][MW][2];   // [set][m][hl]
    MDT_FRAG fx[2][HN][2];   // [set = half-step][row][hl]
    const int wfrag = wm * MW * 64 + lane;                       // + slot*W_STEP + (hl*MT + m)*64
    const int xfrag = (kg * ROWS + wr * NROW) * COLS + l31;      // + stage*PAD + hl*HALF_PAD + (n + dy)*COLS + dx
    auto load_fw = [&](int set, int slot) {
        const u32x4* wst = w_l + slot * W_STEP + wfrag;
#pragma unroll
        for (int m = 0; m < MW; ++m)
#pragma unroll
            for (int hl = 0; hl < NHL; ++hl) fw[set][m][hl] = __builtin_bit_cast(MDT_FRAG, wst[(hl * MT + m) * 64]);
    };
    auto load_fx = [&](int set, int stage, int dy, int dx, int h) {
        const u32x4* ist = in_l + stage * IS::PAD + xfrag + (dy + h * HN) * COLS + dx;
#pragma unroll
        for (int n = 0; n < HN; ++n)
#pragma unroll
            for (int hl = 0; hl < NHL; ++hl) fx[set][n][hl] = __builtin_bit_cast(MDT_FRAG, ist[hl * IS::HALF_PAD + n * COLS]);
    };

    Item2 cur, nxt;
    int work = next_valid(blockIdx.x, cur);
    if (work >= total) return;
    unsigned ioff[IS::PW];
    make_ioff(cur, ioff);
#pragma unroll
    for (int i = 0; i < IS::PW; ++i) issue_input_piece(cur, ioff, 0, 0, i);
    issue_wstep(cur, 0, 0, 0, 0);
    issue_wstep(cur, 0, 0, 1, 1);
    issue_wstep(cur, 0, 0, 2, 2);
    issue_consts(cur, 0);
    startup_skew(P, wave, lane);
    int par = 0, r0 = 0;

    // a conv2's residual arrives in the accumulators, as in k_conv3x3_rec (conv_rec_common.h: ResRows)
    f32x16 acc[MW][NROW][1];
    const bool res_in_acc = P.res != nullptr && !(pdbg(P.dbg) & 1);
    auto res_rows = [&](const Item2& it, bool on) {
        ResRows<NROW> R;
        R.on = on; R.b = it.b; R.mt_global0 = it.cb * MT + wm * MW;
#pragma unroll
        for (int n = 0; n < NROW; ++n) R.ys[n] = it.y0 + wr * NROW + n;
        int le = lane;
        asm volatile("" : "+v"(le));
        R.x = it.x0 + (le & 31);
        R.x_ok = R.x < P.W;
        return R;
    };
    if (res_in_acc) {
        const ResRows<NROW> R0 = res_rows(cur, true);
#pragma unroll
        for (int m = 0; m < MW; ++m) residual_into_acc<NROW, MW, NROW>(P.res, P.Cout, (size_t)P.H * P.W, P.H, P.W, kg, R0, m, 0, acc);
    }
    while (true) {
        MDT_WAITV(0);          // this wave's pieces of the item's first operands have landed (and its stores of the last item are out)
        MDT_BARRIER();
        load_fw(0, r0);
        load_fx(0, 0, 0, 0, 0);
        const int work_n = next_valid(work + gridDim.x, nxt);
        const bool has_next = work_n < total;
        unsigned ioff_n[IS::PW];
        if (has_next) make_ioff(nxt, ioff_n);

        if (!res_in_acc) {
#pragma unroll
            for (int m = 0; m < MW; ++m)
#pragma unroll
                for (int n = 0; n < NROW; ++n)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[m][n][0][q] = 0.0f;
        }

        // one trip = 2 K-steps = 18 steps: register sets (fw: step parity, fx: half-step) and the input stage are compile-time,
        // the ring slot is rb + u (mod 4) with the trip's origin rb in a scalar register
        for (int k2 = 0; k2 < P.NK; k2 += 2) {
            const int rb = (r0 + k2) & 3;                     // 9 k2 = k2 (mod 4)
            const bool last_trip = k2 + 2 >= P.NK;
#pragma unroll
            for (int u = 0; u < 18; ++u) {
                const int kk = u / 9, s = u % 9, dy = s / 3, dx = s % 3;
                const int k = k2 + kk;
                const int ws = u & 1;
                // ---- half-step 0: rows 0 .. HN-1; the fragments of half-step 1 go out first
                MDT_PIN();
                load_fx(1, kk, dy, dx, 1);
                MDT_PIN();
#pragma unroll
                for (int term = 3 - NT; term < 3; ++term)
#pragma unroll
                    for (int n = 0; n < HN; ++n)
#pragma unroll
                        for (int m = 0; m < MW; ++m)
                            acc[m][n][0] = MDT_MFMA(fw[ws][m][term == 0 ? 1 : 0], fx[0][n][term == 1 ? 1 : 0],
                                                                                   acc[m][n][0], 0, 0, 0);   // w_lo x_hi, w_hi x_lo, w_hi x_hi
                MDT_PIN();
                // ---- the barrier of step t publishes chunk t+1 (and, at s = 8, the input stage of the next K-step).  Requested by
                // this wave after chunk t+1, oldest first: the input piece of step t-2, chunk t+2 (2 pieces), the input piece of
                // step t-1 -- input pieces go out at s = 0 .. 4 from every wave (s = 5: waves 0 / 1 only):
                //     s:  0  1  2  3  4  5  6  7  8
                //     N:  2  3  4  4  4  4  3  2  2
                // The last item of a block requests nothing in its last K-step: vmcnt(0).
                const bool tail = kk == 1 && last_trip && !has_next;
                if (tail) {
                    MDT_WAITV(0);
                } else if (s == 0 || s >= 7) {
                    MDT_WAITV(2);
                } else if (s == 1 || s == 6) {
                    MDT_WAITV(3);
                } else {
                    MDT_WAITV(4);
                }
                MDT_BARRIER();
                // ---- requests of step t: chunk t+3 into the slot of chunk t-1, one piece of the next K-step's input stage
                {
                    const int s3 = s + 3, slot3 = (rb + u + 3) & 3;
                    const bool into_next_item = kk == 1 && last_trip;      // "K-step k+1" is K-step 0 of the block's next item
                    if (s3 < 9) {
                        issue_wstep(cur, k, s3 / 3, s3 % 3, slot3);
                    } else if (!into_next_item) {
                        issue_wstep(cur, k + 1, (s3 - 9) / 3, (s3 - 9) % 3, slot3);
                    } else if (has_next) {
                        issue_wstep(nxt, 0, (s3 - 9) / 3, (s3 - 9) % 3, slot3);
                    }
                    if (s < IS::PW) {
                        if (!into_next_item) issue_input_piece(cur, ioff, k + 1, (kk + 1) & 1, s);
                        else if (has_next) issue_input_piece(nxt, ioff_n, 0, 0, s);
                    }
                    if (s == 6 && into_next_item && has_next) issue_consts(nxt, par ^ 1);
                }
                // ---- half-step 1: rows HN .. NROW-1; the fragments of step t+1 go out first
                MDT_PIN();
                if (u < 17) {
                    const int u1 = u + 1, kk1 = u1 / 9, s1 = u1 % 9;
                    load_fw(ws ^ 1, (rb + u1) & 3);
                    load_fx(0, kk1, s1 / 3, s1 % 3, 0);
                } else if (!last_trip) {
                    load_fw(ws ^ 1, (rb + 18) & 3);
                    load_fx(0, 0, 0, 0, 0);
                }
                MDT_PIN();
#pragma unroll
                for (int term = 3 - NT; term < 3; ++term)
#pragma unroll
                    for (int n = 0; n < HN; ++n)
#pragma unroll
                        for (int m = 0; m < MW; ++m)
                            acc[m][HN + n][0] = MDT_MFMA(fw[ws][m][term == 0 ? 1 : 0], fx[1][n][term == 1 ? 1 : 0],
                                                                                        acc[m][HN + n][0], 0, 0, 0);
                MDT_PIN();
            }
        }

        EpiCtx E;
        E.res = P.res; E.y32 = P.y32; E.yrec = P.yrec;
        E.has_bias = P.bias != nullptr; E.has_act = P.yrec != nullptr && P.coef != nullptr;
        E.Cout = P.Cout; E.H = P.H; E.W = P.W; E.b = cur.b; E.kg = kg;
        E.HW = (size_t)P.H * P.W; E.planeO = plane; E.WpO = Wp; E.dbg = pdbg(P.dbg);
        int le = lane;
        asm volatile("" : "+v"(le));      // (re-derived: a separate l31 kept alive through the epilogue goes to scratch)
        const int x = cur.x0 + (le & 31);
        int ys[NROW];
#pragma unroll
        for (int n = 0; n < NROW; ++n) ys[n] = cur.y0 + wr * NROW + n;
        if (!(pdbg(P.dbg) & 1)) {
            epilogue_item<1, NROW, MW, 32, false, MDT_REC_OUT16 != 0>(E, ec_l + par * EC2, acc, wm * MW, cur.cb * MT + wm * MW, ys, x, x < P.W, res_rows(nxt, has_next));
        }
        if (!has_next) break;
        work = work_n;
        cur = nxt;
        par ^= 1;
        r0 = (r0 + P.NK) & 3;                                // 9 NK = NK (mod 4)
#pragma unroll
        for (int i = 0; i < IS::PW; ++i) ioff[i] = ioff_n[i];
    }
}
