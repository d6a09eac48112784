// Body of k_upconv_rec2 / k_upconv_rec2_1t (csrc/vae_conv_rec2.hip includes this file twice, the way vae_conv_rec.hip shares its bodies):
//   MDT_REC2_TERMS = 3: the three-term kernel (w_lo x_hi, w_hi x_lo, w_hi x_hi per product); = 1: MDTILE_PRECISION_BF16, w_hi x x_hi only and
//   only the hi fragments read -- the DMA pieces (lo planes included), ring slots and counted waits of every step are the three-term kernel's.
// MDT_REC_OUT16 = 1 (k_upconv_rec_o16 / k_upconv_rec2_o16, MDTILE_PRECISION_F16): the three-term kernel with the fp16 record-out epilogue (R16)
#include "mfma_operand.h"
__global__ __launch_bounds__(256, 2) void MDT_REC2_KERNEL(const ConvRParams P) {
    constexpr int NT = MDT_REC2_TERMS, NHL = NT == 3 ? 2 : 1;   // products per MFMA site (3: w_lo x_hi, w_hi x_lo, w_hi x_hi; 1: w_hi x_hi), planes read
    constexpr int MT = 4, MW = 2, WM = 2, NROW = 2, TH = 4, R = 6;
    constexpr int ROWS = TH + 2, COLS = 34;
    using IS = InStage<ROWS, NWV>;
    constexpr int W_STEP = 2 * MT * 64;               // records of a step chunk [hl][mt][lane]
    constexpr int W_PH = 4 * W_STEP;                  // records of a packed phase chunk [hl][bb][v][mt][lane] (the layout in HBM)
    constexpr int W_PW = W_STEP / 64 / NWV;
    static_assert(W_PW == 2, "a step chunk is two pieces per wave");
    static_assert(IS::PW == 4 && IS::DMA > 3 * NWV, "the counted waits below assume three input pieces from every wave (a fourth from some)");
    __shared__ u32x4 smem[2 * IS::PAD + R * W_STEP + 2 * EC2];
    u32x4* const in_l = smem;
    u32x4* const w_l = smem + 2 * IS::PAD;
    u32x4* const ec_l = smem + 2 * IS::PAD + R * W_STEP;

    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, kg = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wr = wave / WM;
    const int Hp = P.HinF + 2, Wp = rec_pitch(P.WinF), Pn = P.Cin >> 3;      // pitches of the WHOLE input image; items tile its window
    const size_t plane = (size_t)Hp * Wp;

    struct Item {
        int b, cb, a, y0, x0;   // y0, x0: INPUT coordinates (relative to the window)
    };
    const int per = P.NCB * 2, per_img = ((P.ptiles + 7) / 8) * 8 * per, total = per_img * P.B;
    auto decode = [&](int work, Item& it) -> bool {
        it.b = work / per_img;
        const int r = work - it.b * per_img, xcd = r & 7, slot = r >> 3;
        const int ptile = (slot / per) * 8 + xcd, rem = slot % per;
        it.cb = rem >> 1;
        it.a = rem & 1;
        const int py = ptile / P.PX, px = ptile - py * P.PX;
        it.y0 = py * TH;
        it.x0 = px * 32;
        return ptile < P.ptiles;
    };
    auto next_valid = [&](int work, Item& it) -> int {
        while (work < total && !decode(work, it)) work += gridDim.x;
        return work;
    };
    auto make_ioff = [&](const Item& it, unsigned (&ioff)[IS::PW]) {
#pragma unroll
        for (int i = 0; i < IS::PW; ++i) {
            const int di = wave + NWV * i;
            int s = (di % IS::HALF_DMA) * 64 + lane;
            if (s >= IS::HALF) s = IS::HALF - 1;
            const int g = s / (ROWS * COLS), p = s - g * (ROWS * COLS);
            const int r = p / COLS, c = p - r * COLS;
            int pr = P.iy0[it.b & (REC_WIN_MAXB - 1)] + it.y0 + r, pc = P.ix0[it.b & (REC_WIN_MAXB - 1)] + it.x0 + c;   // inside the window's own border: the image's real neighbours
            pr = pr < Hp ? pr : Hp - 1;
            pc = (pc < P.WinF + 1 ? pc : P.WinF + 1) + REC_COL0;
            ioff[i] = (unsigned)(((size_t)g * plane + (size_t)pr * Wp + pc) * 16);
        }
    };
    auto issue_input_piece = [&](const Item& it, const unsigned (&ioff)[IS::PW], int k, int stage, int i) {
        const int di = wave + NWV * i;
        if (di < IS::DMA) {
            const char* xb = reinterpret_cast<const char*>(P.x + (size_t)it.b * 2 * Pn * plane);
            const char* base = xb + ((size_t)(di / IS::HALF_DMA) * Pn + 2 * (size_t)k) * plane * 16;
            dma16(base, ioff[i], in_l + stage * IS::PAD + di * 64);
        }
    };
    const int nph = P.NK * 2;
    const unsigned lane16 = lane * 16;
    // step chunk (k, u, c) of the item's (row parity, cout block) -> ring slot: piece p = wave + 4 i = (hl, m-tile) = (i, wave)
    auto issue_wstep = [&](const Item& it, int k, int u, int c, int slot) {
        const int bb = c >> 1, v = ((c + 1) >> 1) - bb;
        const char* wsrc = reinterpret_cast<const char*>(P.w + (((size_t)it.a * P.NCB + it.cb) * nph + (size_t)(k * 2 + u)) * W_PH);
#pragma unroll
        for (int i = 0; i < W_PW; ++i) {
            const int p = wave + NWV * i, hl = p / MT, j = p % MT;
            dma16(wsrc + (size_t)((((hl * 2 + bb) * 2 + v) * MT + j) * 64) * 16, lane16, w_l + slot * W_STEP + p * 64);
        }
    };
    auto issue_consts = [&](const Item& it, int par) {
        if (lane < 32) {
            if (wave == 0 && P.bias) dma16(reinterpret_cast<const char*>(P.bias + it.cb * (MT * 32)), lane16, ec_l + par * EC2);
            if ((wave == 1 || wave == 2) && P.yrec && P.coef)
                dma16(reinterpret_cast<const char*>(P.coef + ((size_t)it.b * 2 + (wave - 1)) * P.Cout + it.cb * (MT * 32)), lane16,
                      ec_l + par * EC2 + wave * 32);
        }
    };

    MDT_FRAG fw[2][MW][2];     // [set][m][hl]   weight tiles of one combo-step
    MDT_FRAG fx[2][NROW][2];   // [set][n][hl]   input rows of one column shift
    const int wfrag = wm * MW * 64 + lane;
    auto load_fw = [&](int set, int slot) {
        const u32x4* wst = w_l + slot * W_STEP + wfrag;
#pragma unroll
        for (int m = 0; m < MW; ++m)
#pragma unroll
            for (int hl = 0; hl < NHL; ++hl) fw[set][m][hl] = __builtin_bit_cast(MDT_FRAG, wst[(hl * MT + m) * 64]);
    };
    auto load_fx = [&](int set, int xfrag, int stage, int u, int s) {
        const u32x4* ist = in_l + stage * IS::PAD + xfrag + u * COLS + s;
#pragma unroll
        for (int n = 0; n < NROW; ++n)
#pragma unroll
            for (int hl = 0; hl < NHL; ++hl) fx[set][n][hl] = __builtin_bit_cast(MDT_FRAG, ist[hl * IS::HALF_PAD + n * COLS]);
    };

    Item cur, nxt;
    int work = next_valid(blockIdx.x, cur);
    if (work >= total) return;
    unsigned ioff[IS::PW];
    make_ioff(cur, ioff);
#pragma unroll
    for (int i = 0; i < IS::PW; ++i) issue_input_piece(cur, ioff, 0, 0, i);
#pragma unroll
    for (int t = 0; t < R - 1; ++t) issue_wstep(cur, t / 8, (t % 8) / 4, t % 4, t);      // (NK >= 2: the first 5 steps lie in K-step 0)
    issue_consts(cur, 0);
    startup_skew(P, wave, lane);
    int par = 0, r0 = 0;       // constants-buffer parity, ring slot of this item's step 0

    while (true) {
        MDT_WAITV(0);
        MDT_BARRIER();
        const int xfrag = (kg * ROWS + wr * NROW + cur.a) * COLS + l31;   // halo row of output row n at tap row u: + (n + u)*COLS
        load_fw(0, r0);
        load_fx(0, xfrag, 0, 0, 0);
        const int work_n = next_valid(work + gridDim.x, nxt);
        const bool has_next = work_n < total;
        unsigned ioff_n[IS::PW];
        if (has_next) make_ioff(nxt, ioff_n);

        f32x16 acc[MW][NROW][2];   // [m][n][bb]
#pragma unroll
        for (int m = 0; m < MW; ++m)
#pragma unroll
            for (int n = 0; n < NROW; ++n)
#pragma unroll
                for (int bb = 0; bb < 2; ++bb)
#pragma unroll
                    for (int q = 0; q < 16; ++q) acc[m][n][bb][q] = 0.0f;

        // one trip = 2 K-steps = 16 steps: the register sets (fw: step parity; fx: parity of tap row + shift) and the input stage
        // are compile-time, the ring slot is rb + e (mod 6) with the trip's origin rb in a scalar register
        int rb = r0;
        for (int k2 = 0; k2 < P.NK; k2 += 2) {
            const bool last_trip = k2 + 2 >= P.NK;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int kk = e >> 3, u = (e >> 2) & 1, c = e & 3, e8 = e & 7;
                const int s = (c + 1) >> 1, bb = c >> 1;
                const int k = k2 + kk;
                const int ws = e & 1, xs = (u + s) & 1;
                // ---- term 0 of this step (three-term form only)
                MDT_PIN();
                if constexpr (NT == 3) {
#pragma unroll
                    for (int n = 0; n < NROW; ++n)
#pragma unroll
                        for (int m = 0; m < MW; ++m)
                            acc[m][n][bb] = MDT_MFMA(fw[ws][m][1], fx[xs][n][0], acc[m][n][bb], 0, 0, 0);   // w_lo x_hi
                }
                MDT_PIN();
                // ---- the barrier of step t publishes chunk t+1 (and, at e8 = 7, the input stage of the next K-step).  Requested by
                // this wave after chunk t+1, oldest first: {input piece, chunk (2 pieces)} of the steps t-3, t-2, t-1 -- input pieces
                // go out at e8 = 0 .. 2 from every wave (e8 = 3: waves 0 / 1 only), in front of that step's chunk:
                //     e8:  0  1  2  3  4  5  6  7
                //     N :  6  7  8  9  8  7  6  6
                const bool tail = kk == 1 && last_trip && !has_next;
                if (tail) {
                    MDT_WAITV(0);
                } else if (e8 == 0 || e8 >= 6) {
                    MDT_WAITV(6);
                } else if (e8 == 1 || e8 == 5) {
                    MDT_WAITV(7);
                } else if (e8 == 2 || e8 == 4) {
                    MDT_WAITV(8);
                } else {
                    MDT_WAITV(9);
                }
                MDT_BARRIER();
                // ---- requests of step t: one piece of the next K-step's input stage, then chunk t+5 into the slot of chunk t-1
                {
                    const bool into_next_item = kk == 1 && last_trip;      // "K-step k+1" is K-step 0 of the block's next item
                    if (e8 < IS::PW) {
                        if (!into_next_item) issue_input_piece(cur, ioff, k + 1, (kk + 1) & 1, e8);
                        else if (has_next) issue_input_piece(nxt, ioff_n, 0, 0, e8);
                    }
                    const int e5 = e8 + (R - 1), slot5 = wrap6(rb + (e + R - 1) % 6);
                    if (e5 < 8) {
                        issue_wstep(cur, k, e5 >> 2, e5 & 3, slot5);
                    } else if (!into_next_item) {
                        issue_wstep(cur, k + 1, (e5 - 8) >> 2, (e5 - 8) & 3, slot5);
                    } else if (has_next) {
                        issue_wstep(nxt, 0, (e5 - 8) >> 2, (e5 - 8) & 3, slot5);
                    }
                    if (e8 == 6 && into_next_item && has_next) issue_consts(nxt, par ^ 1);
                }
                // ---- the fragments of step t+1 (the shift s = 1 is shared by c = 1 and c = 2)
                MDT_PIN();
                if (e < 15 || !last_trip) {
                    const int e1 = (e + 1) & 15, kk1 = e1 >> 3, u1 = (e1 >> 2) & 1, c1 = e1 & 3, s1 = (c1 + 1) >> 1;
                    load_fw(ws ^ 1, wrap6(rb + (e + 1) % 6));
                    if (c1 != 2) load_fx(((u1 + s1) & 1), xfrag, kk1, u1, s1);
                }
                MDT_PIN();
                // ---- terms 1, 2 of this step (the one-term form: term 2 only)
#pragma unroll
                for (int term = NT == 3 ? 1 : 2; term < 3; ++term)
#pragma unroll
                    for (int n = 0; n < NROW; ++n)
#pragma unroll
                        for (int m = 0; m < MW; ++m)
                            acc[m][n][bb] = MDT_MFMA(fw[ws][m][0], fx[xs][n][term == 1 ? 1 : 0], acc[m][n][bb], 0, 0, 0);   // w_hi x_lo, w_hi x_hi
                MDT_PIN();
            }
            rb = wrap6(rb + 16 % 6);
        }

        EpiCtx E;
        E.res = P.res; E.y32 = P.y32; E.yrec = P.yrec;
        E.has_bias = P.bias != nullptr; E.has_act = P.yrec != nullptr && P.coef != nullptr;
        E.Cout = P.Cout; E.H = P.H; E.W = P.W; E.b = cur.b; E.kg = kg;
        E.HW = (size_t)P.H * P.W; E.planeO = (size_t)(P.H + 2) * rec_pitch(P.W); E.WpO = rec_pitch(P.W); E.dbg = pdbg(P.dbg);
        const int xi = cur.x0 + l31;
        int ys[NROW];
#pragma unroll
        for (int n = 0; n < NROW; ++n) {
            const int yi = cur.y0 + wr * NROW + n;
            ys[n] = yi < P.Hin ? 2 * yi + cur.a : P.H;      // rows past the input's last row: marked invalid
        }
        if (!(pdbg(P.dbg) & 1)) {
            epilogue_item<2, NROW, MW, 32, false, MDT_REC_OUT16 != 0>(E, ec_l + par * EC2, acc, wm * MW, cur.cb * MT + wm * MW, ys, 2 * xi, xi < P.Win, ResRows<NROW>{});
        }
        if (!has_next) break;
        work = work_n;
        cur = nxt;
        par ^= 1;
        r0 = rb;                                             // the ring runs on: slot of the next item's step 0
#pragma unroll
        for (int i = 0; i < IS::PW; ++i) ioff[i] = ioff_n[i];
    }
}
