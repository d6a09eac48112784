// Per-tile single-head self-attention of the VAE mid block on the bf16 matrix cores with SPLIT-fp32 operands ("bf16x3"),
// flash style (the T x T score matrix never exists).  Same arithmetic contract as vae_conv_bf16x3.hip: every fp32 factor
// is split x = hi + lo (two bf16, 16 significand bits), a product is x_lo*y_hi + x_hi*y_lo + x_hi*y_hi with fp32
// accumulation inside the MFMA; softmax statistics and the exponentials stay fp32.
// Upstream: tile_utils/attn.py:55-70 (bmm -> softmax -> bmm between the 1x1 convs).
//
// Two kernels:
//   k_attn_prep_*   fp32 q, k ([B,C,T] channel-major) and v ([B,T,C] token-major)  ->  bf16 hi/lo FRAGMENT-ORDER records in
//                   the workspace, padded with zeros to a multiple of 128 tokens, so that the main kernel's LDS stages
//                   are straight 16-byte copies and every MFMA operand is one conflict-free ds_read_b128:
//        Qrec / Krec [B][T128/32 token tiles][C/16 k-steps][hl][lane 64] x 8 bf16 :  token = 32*tile + (lane & 31),
//                                                                                  channel = 16*ks + 8*(lane >> 5) + i
//        Vrec        [B][T128/16 key groups ][C/32 m-tiles][hl][lane 64] x 8 bf16 :  channel = 32*mt + (lane & 31),
//                                                       key = 16*group + (i & 3) + 8*(i >> 2) + 4*(lane >> 5)
//                   The V key order is the order in which a lane of the TRANSPOSED score accumulator holds its keys, so
//                   the probabilities go from the score MFMAs to the output MFMAs without any cross-lane movement.
//   k_attn_bf16x3<C>  block = 512 threads (8 waves), 128 queries; per 128-key block:
//        scores  St[key][query] = sum_c K[key][c] Q[query][c]   A = K (M = keys), B = Q (N = queries), K-dim = channels;
//                wave w owns key tile w >> 1 and the two query tiles of half w & 1; channels stream in 64-channel slabs
//        softmax a lane holds one query column (16 keys of its tile): max / sum in-lane + one 32-lane swap, the 4 key
//                tiles of a query are combined through a few hundred bytes of LDS; P -> bf16 hi/lo records in LDS
//        output  Ot[c][query] += sum_key V[key][c] P[key][query]   A = V^T (M = channels), B = P^T, K-dim = keys;
//                the 128 x C output block lives in registers (8 waves x 8 accumulator tiles for C = 512); the V^T fragments
//                of a wave are its own (nobody shares them) and come straight from global memory
//   LDS: two 64 KB slab stages (K + Q slabs by DMA; the P records of a key block overlay the stage that is free) + statistics.
#include "launchers.h"

using namespace mdt;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int BQ = 128, BK = 128;        // queries per block, keys per iteration
constexpr int P_REC = 8 * 4 * 2 * 64;    // [key k-step 8][query tile 4][hl][lane]
constexpr int STAT_FLOATS = 4 * BQ + 4 * BQ + BQ;   // smax[4][128], ssum[4][128], alpha[128]

__device__ __forceinline__ void split8v(const float (&v)[8], u32x4& hi, u32x4& lo) {
    bf16x8 h, l;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        h[i] = (__bf16)v[i];
        l[i] = (__bf16)(v[i] - (float)h[i]);
    }
    hi = __builtin_bit_cast(u32x4, h);
    lo = __builtin_bit_cast(u32x4, l);
}

// ---- prep: q / k  [C][T] fp32 -> records [tile][ks][hl][lane]
__global__ __launch_bounds__(256) void k_attn_prep_qk(const float* __restrict__ src, u32x4* __restrict__ dst, int C, int T, int tiles) {
    const int NKS = C / 16;
    const size_t n = (size_t)tiles * NKS * 64;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int lane = (int)(idx & 63);
    const int ks = (int)((idx >> 6) % NKS);
    const int tile = (int)((idx >> 6) / NKS);
    const int b = blockIdx.y;
    const int tok = tile * 32 + (lane & 31);
    const float* s = src + (size_t)b * C * T;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int c = ks * 16 + (lane >> 5) * 8 + i;
        v[i] = tok < T ? s[(size_t)c * T + tok] : 0.0f;
    }
    u32x4 hi, lo;
    split8v(v, hi, lo);
    u32x4* d = dst + ((size_t)b * tiles * NKS + (size_t)tile * NKS + ks) * 128;
    d[lane] = hi;
    d[64 + lane] = lo;
}

// ---- prep: v  [T][C] fp32 token-major -> records [group16][mt][hl][lane]
__global__ __launch_bounds__(256) void k_attn_prep_v(const float* __restrict__ src, u32x4* __restrict__ dst, int C, int T, int groups) {
    const int NMT = C / 32;
    const size_t n = (size_t)groups * NMT * 64;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int lane = (int)(idx & 63);
    const int mt = (int)((idx >> 6) % NMT);
    const int g = (int)((idx >> 6) / NMT);
    const int b = blockIdx.y;
    const int c = mt * 32 + (lane & 31);
    const float* s = src + (size_t)b * T * C;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int key = g * 16 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
        v[i] = key < T ? s[(size_t)key * C + c] : 0.0f;
    }
    u32x4 hi, lo;
    split8v(v, hi, lo);
    u32x4* d = dst + ((size_t)b * groups * NMT + (size_t)g * NMT + mt) * 128;
    d[lane] = hi;
    d[64 + lane] = lo;
}

// ---- prep: v  [C][T] fp32 CHANNEL-major (the layout every other 1x1 conv of the queue writes) -> the same records.  A lane owns one
// channel and two runs of 4 consecutive keys: two 16-byte loads when T % 4 == 0 (rows then start 16-byte aligned).
__global__ __launch_bounds__(256) void k_attn_prep_v_cm(const float* __restrict__ src, u32x4* __restrict__ dst, int C, int T, int groups) {
    const int NMT = C / 32;
    const size_t n = (size_t)groups * NMT * 64;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int lane = (int)(idx & 63);
    const int mt = (int)((idx >> 6) % NMT);
    const int g = (int)((idx >> 6) / NMT);
    const int b = blockIdx.y;
    const int c = mt * 32 + (lane & 31);
    const float* s = src + ((size_t)b * C + c) * T;
    float v[8];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int k0 = g * 16 + 8 * h + 4 * (lane >> 5);        // keys k0 .. k0 + 3 = record elements 4 h .. 4 h + 3
        if ((T & 3) == 0) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
            if (k0 < T) t = *reinterpret_cast<const float4*>(s + k0);
            v[4 * h] = t.x; v[4 * h + 1] = t.y; v[4 * h + 2] = t.z; v[4 * h + 3] = t.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) v[4 * h + i] = k0 + i < T ? s[k0 + i] : 0.0f;
        }
    }
    u32x4 hi, lo;
    split8v(v, hi, lo);
    u32x4* d = dst + ((size_t)b * groups * NMT + (size_t)g * NMT + mt) * 128;
    d[lane] = hi;
    d[64 + lane] = lo;
}

// LDS-DMA of one 16-byte record per lane (global scalar base + 32-bit lane offset -> LDS wave-uniform base + 16 * lane), issued
// through inline asm: hipcc books __builtin_amdgcn_global_load_lds as a pending FLAT access and then turns every later
// `s_waitcnt lgkmcnt(N)` into lgkmcnt(0), which would serialise the fragment prefetch below (same finding as vae_conv_rec.hip).
// Completion is counted by hand: vmcnt(0) + barrier before any ds_read of the data.
__device__ __forceinline__ void dma16a(const void* base, unsigned voff, const u32x4* lds_dst) {
    const unsigned l = (unsigned)(__UINTPTR_TYPE__)(const __attribute__((address_space(3))) u32x4*)lds_dst;
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 2\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep)
                 : "v"(voff), "s"(base), "s"(l)
                 : "memory");
}

#define MDT_PIN() __builtin_amdgcn_sched_barrier(0)

// One 128-query block against its key range, per 128-key block:
//   scores   channels stream through LDS in 64-channel slabs [K | Q][tile 4][ks 4][hl][lane] (64 KB) by DMA, two stages; the
//            fragments of k-step ks+1 are read while the MFMAs of ks run (two register sets); ONE barrier per slab (24 MFMAs / wave)
//   softmax  as before; the P records (64 KB) are written INTO the slab stage that is free at that point (no LDS of their own)
//   output   V^T fragments are private to a wave (it owns MT_W channel tiles): they go global -> registers directly, two 16-key
//            steps ahead, never through LDS; P fragments are read one half-step ahead.  No barrier inside the output phase.
// 10 barriers per key block (8 slabs + 2 in the softmax) against 26 of the slab-per-32-channels / V-through-LDS schedule.
#define MDT_AT_TERMS 3
#define MDT_AT_KERNEL k_attn_bf16x3
#include "vae_attn_bf16x3_body.h"
#undef MDT_AT_KERNEL
#undef MDT_AT_TERMS
#define MDT_AT_TERMS 1
#define MDT_AT_KERNEL k_attn_bf16x1
#include "vae_attn_bf16x3_body.h"
#undef MDT_AT_KERNEL
#undef MDT_AT_TERMS

// merge the key-range parts of a query: out = sum_s O_s e^(m_s - m) / sum_s l_s e^(m_s - m), m = max_s m_s
__global__ __launch_bounds__(256) void k_attn_combine(const float* __restrict__ part, const float* __restrict__ pstat, float* __restrict__ out,
                                                      int B, int C, int T, int T128, int nsplit) {
    const int q = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
    if (q >= T) return;
    float w[4], m = -INFINITY;
    for (int s = 0; s < nsplit; ++s) m = fmaxf(m, pstat[((size_t)(s * B + b) * 2) * T128 + q]);
    float den = 0.0f;
    for (int s = 0; s < nsplit; ++s) {
        const float* ps = pstat + ((size_t)(s * B + b) * 2) * T128 + q;
        w[s] = exp2f(ps[0] - m);                     // the parts' maxima are kept in the log2 domain (see the softmax above)
        den += ps[T128] * w[s];
    }
    const float inv = 1.0f / den;
    for (int c = blockIdx.y; c < C; c += gridDim.y) {
        float o = 0.0f;
        for (int s = 0; s < nsplit; ++s) o += part[((size_t)(s * B + b) * C + c) * T + q] * w[s];
        out[((size_t)b * C + c) * T + q] = o * inv;
    }
}

}  // namespace

bool mdt::attn_bf16x3_eligible(int C) { return C == 128 || C == 256 || C == 512; }

// The main kernel of a launch from (one-term arithmetic, C); C is one of attn_bf16x3_eligible (the C entry points have checked it)
using AttnKernel = void (*)(const u32x4*, const u32x4*, const u32x4*, float*, int, int, int, int, float, int, float*, float*);
static AttnKernel attn_kernel(bool one, int C) {
    if (one) return C == 512 ? k_attn_bf16x1<512> : C == 256 ? k_attn_bf16x1<256> : k_attn_bf16x1<128>;
    return C == 512 ? k_attn_bf16x3<512> : C == 256 ? k_attn_bf16x3<256> : k_attn_bf16x3<128>;
}

// Key-range split factor: 1 block per CU (133 KB LDS), so the launch runs in ceil(blocks / CUs) rounds; pick the smallest
// nsplit <= 4 whose round occupancy is within 3 % of the best.  MDTILE_ATTN_SPLIT=n forces it.
static int attn_nsplit(int B, int Tq, int Tk) {
    static const int forced = [] { const char* e = probe_env("MDTILE_ATTN_SPLIT"); return e ? atoi(e) : 0; }();
    const int nkb = (Tk + 127) / 128;
    if (forced >= 1 && forced <= 4) return forced <= nkb ? forced : 1;
    // The split is chosen for ONE image of the batch, whatever B is: the key ranges fix the order in which a query's partial sums are
    // combined, and a tile's result must not depend on which other tiles it is stacked with (scripts/tilevae.py stacks tiles of one
    // shape along the batch axis; the live-window sweep and the whole-tile sweep stack differently and are compared bit for bit).
    // More images only add blocks to a launch whose split already fills the chip.
    (void)B;
    const long long blocks = (Tq + 127) / 128;
    // launches that fill the chip several times over: 4 key ranges per query block keep the Q working set of an XCD
    // (32 / nsplit query blocks x C x 512 B) inside its L2 -- see the block mapping in k_attn_bf16x3
    const int cus = device_cus();
    if (blocks >= 2 * cus && nkb >= 32) return 4;
    double eff[5], best = 0.0;
    for (int s = 1; s <= 4; ++s) {
        const long long rounds = (blocks * s + cus - 1) / cus;
        eff[s] = s <= nkb ? (double)(blocks * s) / (double)(rounds * cus) : 0.0;
        if (eff[s] > best) best = eff[s];
    }
    for (int s = 1; s <= 4; ++s)
        if (eff[s] >= best - 0.03) return s;
    return 1;
}

// workspace: Qrec (B * Tq128 * C * 4 bytes: hi + lo bf16 per element), Krec, Vrec (B * Tk128 * C * 4 bytes each)
// [+ nsplit un-normalised parts B*C*Tq fp32 and their (max, sum) rows 2*B*Tq128 fp32 when the key range is split]
size_t mdt::attn_bf16x3_ws_bytes(int B, int C, int Tq, int Tk) {
    const size_t Tq128 = ((size_t)Tq + 127) / 128 * 128, Tk128 = ((size_t)Tk + 127) / 128 * 128;
    const int ns = attn_nsplit(B, Tq, Tk);
    size_t bytes = (size_t)B * (Tq128 + 2 * Tk128) * C * 4;
    if (ns > 1) bytes += (size_t)ns * ((size_t)B * C * Tq + 2 * (size_t)B * Tq128) * 4;
    return bytes;
}

int mdt::attn_bf16x3_launch(const float* d_q, const float* d_k, const float* d_v_tok, float* d_out, int B, int C, int Tq, int Tk, float scale,
                       void* d_ws, hipStream_t s, bool v_channel_major) {
    const int Tq128 = (Tq + 127) / 128 * 128, Tk128 = (Tk + 127) / 128 * 128;
    const size_t perq = (size_t)B * Tq128 * C * 4 / 16, perk = (size_t)B * Tk128 * C * 4 / 16;   // records per operand
    u32x4* Qr = (u32x4*)d_ws;
    u32x4* Kr = Qr + perq;
    u32x4* Vr = Kr + perk;
    const int ns = attn_nsplit(B, Tq, Tk);
    float* part = (float*)(Vr + perk);
    float* pstat = part + (size_t)ns * B * C * Tq;
    {
        const int qtiles = Tq128 / 32, ktiles = Tk128 / 32;
        const size_t nq = (size_t)qtiles * (C / 16) * 64, nk = (size_t)ktiles * (C / 16) * 64;
        hipLaunchKernelGGL(k_attn_prep_qk, dim3(cdiv((long long)nq, 256), B), dim3(256), 0, s, d_q, Qr, C, Tq, qtiles);
        hipLaunchKernelGGL(k_attn_prep_qk, dim3(cdiv((long long)nk, 256), B), dim3(256), 0, s, d_k, Kr, C, Tk, ktiles);
    }
    {
        const int groups = Tk128 / 16;
        const size_t n = (size_t)groups * (C / 32) * 64;
        dim3 grid(cdiv((long long)n, 256), B);
        if (v_channel_major) hipLaunchKernelGGL(k_attn_prep_v_cm, grid, dim3(256), 0, s, d_v_tok, Vr, C, Tk, groups);
        else hipLaunchKernelGGL(k_attn_prep_v, grid, dim3(256), 0, s, d_v_tok, Vr, C, Tk, groups);
    }
    MDT_LAUNCH_CHECK();
    const int nq8 = (Tq128 / BQ + 7) / 8 * 8;
    dim3 grid(nq8 * ns, B), block(512);
    // MDTILE_PRECISION_BF16, and the attention of MDTILE_PRECISION_F16: one bf16 MFMA per product
    hipLaunchKernelGGL(attn_kernel(mfma_single_term() || mode_f16(), C), grid, block, 0, s, Qr, Kr, Vr, d_out, Tq, Tq128, Tk, Tk128, scale, ns, part, pstat);
    MDT_LAUNCH_CHECK();
    if (ns > 1) {
        dim3 cgrid(cdiv(Tq, 256), C < 64 ? C : 64, B);
        hipLaunchKernelGGL(k_attn_combine, cgrid, dim3(256), 0, s, part, pstat, d_out, B, C, Tq, Tq128, ns);
        MDT_LAUNCH_CHECK();
    }
    return MDTILE_OK;
}
