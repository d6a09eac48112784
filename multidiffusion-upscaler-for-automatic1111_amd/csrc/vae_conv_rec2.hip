// Record-image 3x3 conv and sub-pixel upsample conv, TWO INDEPENDENT 4-WAVE BLOCKS PER CU (round 4).
//
// Same arithmetic, same record images, same packed weights and the same per-accumulator MFMA order as vae_conv_rec.hip (the
// results are bit-identical to that file's kernels); what changes is who shares a SIMD.  There one 512-thread block owns the CU:
// its two waves per SIMD run in lock step, and the item's store epilogue (12.8 us of an 87 us item record -> record, 33 us of
// 108 us with the fp32 residual / fp32 output streams -- 17 % of the family's time, profiles/r3g) runs with the matrix pipes
// idle, because vmcnt retires loads and stores in order: a wave cannot leave its stores draining behind the next item's DMA
// waits.  Only ANOTHER wave's MFMAs can cover them.  gfx950 has one barrier per workgroup, so that other wave has to live in
// another workgroup: here a CU holds two 256-thread blocks (one wave each per SIMD, <= 80 KB of LDS, <= 256 registers), each
// working through its own items, and the second block to arrive on a CU starts half an item late, so that one block's epilogue
// (and every barrier / DMA wait of its K loop) sits under the other block's K loop.
//
// What that costs and how it is paid:
//   * half the LDS per block: an item is 128 couts x 8 rows x 32 px (wave tile unchanged: 64 couts x 4 rows, 8 accumulator
//     tiles); the weight ring holds STEP chunks -- one (K-step, dy, dx) = [hl][mt][lane] = 8 KB -- in 4 slots instead of phase
//     chunks in 3, the input stage [hl][kg][10][34] records stays double-buffered: 45 + 32 + 3 KB = 79 KB;
//   * one block barrier per step (24 MFMAs per wave) instead of per phase (72): a wave that waits leaves its SIMD to the other
//     block's wave, which is the point;
//   * the weight stream from L2 doubles per MFMA (8-row items): 14 B/clk per CU, inside the L2s' rate.
// DMA protocol (global_load_lds_dwordx4 from inline asm, completion counted by hand, as in vae_conv_rec.hip): the chunk of step
// t+3 is requested right behind the barrier of step t (its slot held step t-1, which every wave has finished reading by then)
// and has to have landed at the barrier of step t+2; the input stage of K-step k+1 goes out one piece per wave and step during
// the first six steps of K-step k.  Every barrier is preceded by a COUNTED vmcnt: the pieces a wave has requested after the chunk
// the barrier publishes may stay in flight (N(s) below; waves that requested an extra piece -- the ragged sixth input piece, the
// epilogue constants -- merely wait for it too).  The stream of chunks / input stages runs on across item boundaries: the last
// K-step of an item requests the first operands of the block's next item.
//
// Upstream call sites replaced: the same as vae_conv_rec.hip (scripts/tilevae.py:115-195 conv1 / conv2 / upsample.conv tasks,
// :218-245 custom_group_norm, :102-104 SiLU, :614-616 add_res).
#include "common.h"

#include <mutex>

using namespace mdt;

#include "conv_rec_common.h"

namespace {

constexpr int NWV = 4;            // waves per block: one per SIMD; the CU's other four wave slots belong to the second block
constexpr int EC2 = 3 * 32;       // records of one constants buffer: [bias | a | s] x 512 B (requested by 32 lanes each)

#define MDT_WAITV(n) __builtin_amdgcn_s_waitcnt(0x0F70 | (n))      // s_waitcnt vmcnt(n), n <= 15 (expcnt / lgkmcnt untouched)
#define MDT_BARRIER()                    \
    do {                                 \
        asm volatile("" ::: "memory");   \
        __builtin_amdgcn_s_barrier();    \
        asm volatile("" ::: "memory");   \
    } while (0)

struct Item2 {
    int b, cb, y0, x0;
};

// The block that arrives second on its CU waits `skew_ticks` before its first item (see the file header).  "Second" is decided
// by an arrival counter per hardware CU (XCC_ID, and SE / SH / CU id of HW_ID); without a counter buffer by the block index
// (blocks >= grid / 2 are dispatched after every CU got its first block).  Wave 0 only: the others wait at the item's first barrier.
__device__ __forceinline__ void startup_skew(const ConvRParams& P, int wave, int lane) {
    if (wave != 0) return;                                                   // (wave-uniform: the waits below are scalar loops)
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);           // HW_REG_HW_ID: [11:8] CU, [12] SH, [15:13] SE
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u;    // HW_REG_XCC_ID[3:0]
    const unsigned key = (xcc << 8) | ((hw >> 8) & 255u);
    unsigned second = blockIdx.x >= gridDim.x / 2 ? 1u : 0u;
    if (P.cu_ctr) {
        // arrival number of this block on its CU IN THIS LAUNCH: the counter word carries the launch epoch, so a launch that left an odd
        // number of blocks on some CUs (grid < 2 CUs is common for this family) cannot flip the parity of every later launch there
        unsigned n = 0;
        if (lane == 0) {
            unsigned* c = P.cu_ctr + key;
            unsigned seen = *reinterpret_cast<volatile unsigned*>(c);
            while (true) {
                const unsigned cnt = (seen >> 8) == P.epoch ? (seen & 255u) : 0u;
                const unsigned prev = atomicCAS(c, seen, (P.epoch << 8) | ((cnt + 1u) & 255u));
                if (prev == seen) { n = cnt; break; }
                seen = prev;
            }
        }
        second = (unsigned)__builtin_amdgcn_readfirstlane((int)n) & 1u;
    }
    if (P.census && lane == 0) P.census[blockIdx.x] = key | (second << 31);
    if (second && P.skew_ticks) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__builtin_amdgcn_s_memrealtime() - t0 < P.skew_ticks) __builtin_amdgcn_s_sleep(32);
    }
}

// =====================================================================================================================
// direct 3x3.  MW = 32-cout tiles per wave (2), WM = waves along cout (2), NROW = pixel rows per wave (4: two half-steps of 2).
// Step t = (k, dy, dx) of an item, 9 NK steps; chunk(t) sits in ring slot (r0 + t) & 3, r0 = the item's ring origin (the ring
// runs on across items: r0' = (r0 + 9 NK) & 3); K-step k uses input stage k & 1 (NK is even: every item starts in stage 0).
// One step of a wave:   fx(t, h=1) <- LDS | 12 MFMAs (rows 0-1) | vmcnt(N) + barrier | DMA requests |
//                       fw(t+1), fx(t+1, h=0) <- LDS | 12 MFMAs (rows 2-3)
#define MDT_OPERAND_F16 0      // mfma_operand.h: bf16 fragments
#define MDT_REC_OUT16 0        // epilogue_item<.., R16>: the record output is a bf16 (hi, lo) split
#define MDT_REC2_TERMS 3
#define MDT_REC2_KERNEL k_conv3x3_rec2
#include "vae_conv_rec2_direct_body.h"
#undef MDT_REC2_KERNEL
#undef MDT_REC2_TERMS
#define MDT_REC2_TERMS 1
#define MDT_REC2_KERNEL k_conv3x3_rec2_1t
#include "vae_conv_rec2_direct_body.h"
#undef MDT_REC2_KERNEL
#undef MDT_REC2_TERMS
// fp16 forms (MDTILE_PRECISION_F16, see vae_conv_rec.hip): fp16 input record + fp16 weight plane; record output fp16 (_f16) or a bf16 split / none (_f16s)
#undef MDT_OPERAND_F16
#define MDT_OPERAND_F16 1
#define MDT_REC2_TERMS 1
#undef MDT_REC_OUT16
#define MDT_REC_OUT16 1
#define MDT_REC2_KERNEL k_conv3x3_rec2_f16
#include "vae_conv_rec2_direct_body.h"
#undef MDT_REC2_KERNEL
#undef MDT_REC_OUT16
#define MDT_REC_OUT16 0
#define MDT_REC2_KERNEL k_conv3x3_rec2_f16s
#include "vae_conv_rec2_direct_body.h"
#undef MDT_REC2_KERNEL
#undef MDT_REC2_TERMS
#undef MDT_OPERAND_F16
#define MDT_OPERAND_F16 0

// =====================================================================================================================
// nearest-2x upsample + 3x3 conv in sub-pixel form (vae_conv_rec.hip: k_upconv_rec; derivation in vae_conv_bf16x3.hip), two blocks
// per CU.  Item = 128 couts x (4 x 32 INPUT px) of ONE output-row parity a and both column parities bb (wave tile 64 couts x 2
// input rows x 2 bb = 8 accumulator tiles).  Step t = (k, u, c): tap row u, combo-step c
//     c:  0 (shift s 0, bb 0)   1 (s 1, bb 0)   2 (s 1, bb 1)   3 (s 2, bb 1)        tap column v = s - bb
// 12 MFMAs per wave and step, 8 steps per K-step.  Step chunk = [hl][mt][lane] of (k, u, bb, v), 8 KB; the ring has SIX slots
// (the steps are half as long as the direct kernel's, so the same time in flight needs twice the chunks): the chunk of step t+5
// is requested behind the barrier of step t and has to have landed at the barrier of step t+4.  Input stage [hl][kg][6][34]
// records, double-buffered, 3-4 pieces per wave requested at the first steps of the previous K-step (before that step's chunk:
// the stage must be older than the chunk whose barrier publishes it).  28 + 48 + 3 KB = 79 KB.
// One step of a wave:   4 MFMAs (term 0) | vmcnt(N) + barrier | DMA requests | fw(t+1), fx(t+1) <- LDS | 8 MFMAs (terms 1, 2)
__device__ __forceinline__ int wrap6(int x) { return x >= 6 ? x - 6 : x; }

#define MDT_REC2_TERMS 3
#define MDT_REC2_KERNEL k_upconv_rec2
#include "vae_conv_rec2_upconv_body.h"
#undef MDT_REC2_KERNEL
#undef MDT_REC2_TERMS
#define MDT_REC2_TERMS 1
#define MDT_REC2_KERNEL k_upconv_rec2_1t
#include "vae_conv_rec2_upconv_body.h"
#undef MDT_REC2_KERNEL
#undef MDT_REC2_TERMS
// MDTILE_PRECISION_F16: the three-term upsample conv (raw-stream operand) with its activated record output in the fp16 form
#undef MDT_REC_OUT16
#define MDT_REC_OUT16 1
#define MDT_REC2_TERMS 3
#define MDT_REC2_KERNEL k_upconv_rec2_o16
#include "vae_conv_rec2_upconv_body.h"
#undef MDT_REC2_KERNEL
#undef MDT_REC2_TERMS
#undef MDT_REC_OUT16
#define MDT_REC_OUT16 0

}  // namespace

// arrival counters of startup_skew: one buffer per device, allocated on first use (under a lock: launches may come from several host
// threads), zeroed once; every launch takes a fresh epoch (see startup_skew), so nothing is ever reset.  The counter words are per
// DEVICE, not per stream: two rec2 launches in flight on one device at once (different streams) re-stamp each other's arrival counts,
// so "second block on this CU" can be decided wrongly for either -- that moves a block's START by half an item, never a result (the
// plugin and the bench run one stream per device; the heuristic assumes that).
static unsigned* cu_counters(unsigned* epoch) {
    static std::mutex mu;
    static unsigned* buf[64] = {};
    static unsigned next_epoch[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!buf[dev]) {
        unsigned* p = nullptr;
        if (hipMalloc(&p, 16 * 256 * sizeof(unsigned)) != hipSuccess) return nullptr;
        if (hipMemset(p, 0, 16 * 256 * sizeof(unsigned)) != hipSuccess) {
            (void)hipFree(p);      // (no counters: this launch runs without the skew; the next one tries again)
            return nullptr;
        }
        buf[dev] = p;
    }
    next_epoch[dev] = (next_epoch[dev] + 1u) & 0xFFFFFFu;
    if (next_epoch[dev] == 0u) next_epoch[dev] = 1u;      // (0 = the zeroed buffer's epoch)
    *epoch = next_epoch[dev];
    return buf[dev];
}

// The two-blocks-per-CU kernel of a launch, from the facts conv_rec_launch hands over (vae_conv_rec.hip: rec_kernel; no statistics, no narrow cout here)
static RecKernel rec2_kernel(int up, bool one, int x16, int y16) {
    if (up) return y16 ? k_upconv_rec2_o16 : one ? k_upconv_rec2_1t : k_upconv_rec2;
    if (x16) return y16 ? k_conv3x3_rec2_f16<2, 2, 4> : k_conv3x3_rec2_f16s<2, 2, 4>;
    return one ? k_conv3x3_rec2_1t<2, 2, 4> : k_conv3x3_rec2<2, 2, 4>;
}

// Probing switches (PROBES build of the library only -- common.h: probe_env; read per launch so that a probe can flip them in-process):
//   MDTILE_REC2_SKEW    0 = no start-up delay, 1 = by block index (>= grid / 2), 2 = by the per-CU arrival counter (default)
//   MDTILE_REC2_SKEW_PCT  the delay as a percentage of an item's K loop at one block per CU-half (default 100)
//   MDTILE_REC2_CENSUS  device address (hex) of a [grid] unsigned buffer that receives every block's hardware CU id
int mdt::conv_rec2_launch(ConvRParams P, int B, int up, hipStream_t s, int cus, bool one, int x16, int y16) {
    int skew = 2, pct = 100;
    if (const char* e = probe_env("MDTILE_REC2_SKEW")) skew = atoi(e);
    if (const char* e = probe_env("MDTILE_REC2_SKEW_PCT")) pct = atoi(e);
    P.census = nullptr;
    if (const char* e = probe_env("MDTILE_REC2_CENSUS")) P.census = reinterpret_cast<unsigned*>((uintptr_t)strtoull(e, nullptr, 16));
    P.epoch = 0;
    P.cu_ctr = skew == 2 ? cu_counters(&P.epoch) : nullptr;
    int per_cu = 2;                                   // two blocks per CU
    if (const char* e = probe_env("MDTILE_REC2_PER_CU")) per_cu = atoi(e) == 1 ? 1 : 2;      // probing: a 4-wave block alone on its CU
    const int grid_max = per_cu * (cus / 8 * 8);
    // K loop of one item with the SIMDs to itself, in 10 ns ticks.  up: NK x 8 steps x 12 MFMAs x 32 clk at ~2 GHz = NK x 1.5 us; direct: NK x 9 steps
    // x 24 MFMAs x 32 clk = NK x 3.5 us
    P.skew_ticks = skew ? (unsigned)((long long)P.NK * (up ? 154 : 346) * pct / (one ? 300 : 100)) : 0u;
    P.PX = ((up ? P.Win : P.W) + 31) / 32;
    P.ptiles = P.PX * (up ? (P.Hin + 3) / 4 : (P.H + 7) / 8);
    const long long items = (long long)((P.ptiles + 7) / 8) * 8 * P.NCB * (up ? 2 : 1) * B;
    dim3 grid((unsigned)(items < grid_max ? items : grid_max)), block(256);
    hipLaunchKernelGGL(rec2_kernel(up, one, x16, y16), grid, block, 0, s, P);
    MDT_LAUNCH_CHECK();
    return MDTILE_OK;
}

