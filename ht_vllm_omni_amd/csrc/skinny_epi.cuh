// The launch-path skinny GEMM in front of and behind its MFMA loop: gemm_skinny_kernel (gemm.hip) and gemm_w8_kernel (gemm_w8.hip) differ
// only in how W reaches the MFMA, so the prologue (sum(r^2) slab gather, old-residual fetch) and everything from the combine on are written
// here once, on the value helpers of gemm_frag.cuh (which chain_gemm.cuh uses with its own coherent loads and stores).
#pragma once
#include "common.cuh"
#include "gemm_frag.cuh"

#define SKINNY_THREADS (SKINNY_WAVES * 64)

// what both kernels' prologue and epilogue read (GemmArgs and W8Args extend it with their operands)
struct SkinnyArgs {
    const uint16_t* bias; void* out;
    int M, N, K;
    const uint8_t* mask;       // fp32 epilogues: logit n is `mask_fill` where mask[n] == 0
    float mask_fill;           // (-inf; the Omni talker writes -1e9)
    const uint16_t* resid;     // EPI_RESID: the stream to add into (NULL: start a new one)
    float eps;                 // PRO_XNORM
    int oshuf;                 // fragment-major out (OMNI_LAYOUT_OUT_FRAG), see common.cuh frag_off
    // PRO_XNORM / EPI_RESID: per-row sum-of-squares slabs [np][pstride rows] fp32 (deterministic: one slab per producer workgroup)
    const float* part_in; int np_in; float* part_out;
    int pstride;               // rows per slab (64; 128 for the code predictor's two-position pass)
};

// LDS of a workgroup: [WAVES][NT*MT][64] f32x4 combine slots, then (norm-fused) [WAVES][64] slab partials
template <int MT, int NT>
__device__ __forceinline__ float* skinny_red(float* lds) { return lds + SKINNY_WAVES * NT * MT * 4 * 64; }

// ---- prologue: the loads that go out BEFORE the W ring so that they return first (loads complete in order)
template <int MT, bool NORM, int EPI>
struct SkinnyPro {
    static constexpr int XROWS = MT * 16, NCH = SKINNY_THREADS / XROWS;
    typedef SlabOrder<XROWS> SO;             // canonical slab order (gemm_frag.cuh): SO::PE slabs per thread cover np <= 128
    float pv[SO::PE];
    float psum;
    u32x2 r_old;

    __device__ __forceinline__ void load(const SkinnyArgs& a, int m_base, int Mloc) {
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        // PRO_XNORM, part 1: this thread's share of the sum(r^2) slabs of the workgroup's OWN rows (row = t % rows, every NCH-th slab; slabs
        // are [n group][pstride rows], so a wave-level load is contiguous); the reduction then overlaps the W latency
        psum = 0.f;
        if (NORM) {
            const int row = lane % XROWS, sub = lane / XROWS, ch = threadIdx.x / XROWS;
            const float* pp = a.part_in + m_base + row;
            SO::gather(pv, wave, sub, a.np_in, [&](int p) { return pp[(size_t)p * a.pstride]; });
            for (int p = ch + 128; p < a.np_in; p += NCH) psum += pp[(size_t)p * a.pstride];      // hidden > 2048 only (no chain there)
        }
        // EPI_RESID: the old residual values this thread will add into (one epilogue item per thread), fetched up front
        r_old = (u32x2){0u, 0u};
        if (EPI == OMNI_EPI_RESID && a.resid && threadIdx.x < MT * 64) {
            const int ml = (threadIdx.x >> 6) * 16 + (lane & 15);
            if (ml < Mloc)
                r_old = *reinterpret_cast<const u32x2*>(a.resid + frag_off(m_base + ml, blockIdx.x * 16 + 4 * (lane >> 4), a.N));
        }
    }

    // PRO_XNORM, part 2 (after the W ring is in flight; PRO 3: behind the MFMA loop): fixed-order reduction -> this wave's partial of the
    // row sums into red[wave][64].  row = lane % XROWS: the channels that share a wave fold by shuffles, the 8 waves through LDS
    __device__ __forceinline__ void reduce_to(const SkinnyArgs& a, float* red) {
        float s_ = SO::reduce(pv);
        if (a.np_in > 128) {                                   // the slabs past the canonical 128: folded over the row's channels as before
            if (XROWS <= 32) psum = xor32_sum(psum);
            if (XROWS <= 16) psum = xor16_sum(psum);
            s_ += psum;
        }
        red[threadIdx.x] = s_;
    }
};

// ---- finish: [PRO 3: the slab reduction,] the LDS combine of the 8 K-partials and the epilogue, with plain stores.
// `stage` (debug library: leave after stage N, launch-cost attribution; product callers pass a constant 0): 3 = + main loop, 4 = + LDS
// write of the K partials + barrier.
template <int MT, int NT, int PRO, int EPI>
__device__ __forceinline__ void skinny_finish(const SkinnyArgs& a, float* lds, const f32x4 (&acc)[NT][MT], SkinnyPro<MT, PRO == 2 || PRO == 3, EPI>& pro,
                                              int m_base, int Mloc, int stage) {
    constexpr bool DEFER = PRO == 3;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int K = a.K, N = a.N;
    float* red = skinny_red<MT, NT>(lds);
    if (DEFER) pro.reduce_to(a, red);      // its loads returned ahead of the operands'; read behind the combine barrier, below
    if (stage == 3) return;

    // (GEMM stage attribution, scripts/ab_knobs.py gemm_stage: the combine + epilogue were 0.42 ms of a 3.93 ms step)
    f32x4* lds4 = reinterpret_cast<f32x4*>(lds);
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i) lds4[(wave * (NT * MT) + j * MT + i) * 64 + lane] = acc[j][i];
    __syncthreads();
    if (stage == 4) return;

    // item = (m-tile i, [n-tile j], lane l): 4 consecutive n (reg 0..3) of one row m
    // OMNI_EPI_SILU_MUL_GU8: every 16-row W tile = 8 gate rows (D lanes 0..31) + the 8 matching up rows (lanes 32..63)
    constexpr bool GU8 = EPI == OMNI_EPI_SILU_MUL_GU8;
    constexpr bool SILU = EPI == OMNI_EPI_SILU_MUL || GU8;
    constexpr int NTO = (EPI == OMNI_EPI_SILU_MUL) ? NT / 2 : NT;
    constexpr int LN = GU8 ? 32 : 64;
    constexpr int ITEMS = NTO * MT * LN;
    for (int it = threadIdx.x; it < ITEMS; it += SKINNY_THREADS) {
        const int l = it % LN;
        const int t = it / LN;
        const int i = t % MT, j = t / MT;
        const int ml = i * 16 + (l & 15);
        if (ml >= Mloc) continue;
        const int m = m_base + ml;
        f32x4 sum = combine_waves(lds4, NT * MT, j * MT + i, l), sum2 = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (EPI == OMNI_EPI_SILU_MUL) sum2 = combine_waves(lds4, NT * MT, (NT / 2 + j) * MT + i, l);
        if (GU8) sum2 = combine_waves(lds4, NT * MT, j * MT + i, l + 32);
        if (DEFER) {
            const float rl = row_rstd(red, ml, K, a.eps);      // (the combine barrier covered the wave partials)
            sum *= rl;
            if (SILU) sum2 *= rl;
        }
        if (SILU) {
            const int n = GU8 ? (blockIdx.x * NT + j) * 8 + 4 * (l >> 4) : blockIdx.x * 16 * (NT / 2) + j * 16 + 4 * (l >> 4);
            float o[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) o[g] = silu_mul_bf16(sum[g], sum2[g]);
            *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(a.out) + (a.oshuf ? frag_off(m, n, N) : (size_t)m * N + n)) =
                make_uint2(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]));
        } else {
            const int n = blockIdx.x * 16 * NT + j * 16 + 4 * (l >> 4);
            float v[4] = {sum[0], sum[1], sum[2], sum[3]};
            if (a.bias) {
#pragma unroll
                for (int g = 0; g < 4; ++g) v[g] += bf2f(a.bias[n + g]);
            }
            if (EPI == OMNI_EPI_RESID) {
                // r = bf16(r + bf16(acc)) in place on the fragment-major residual stream (every element has exactly one
                // owner thread), plus this workgroup's 16-column share of sum(r^2) per row for the consumer's RMSNorm
                static_assert(EPI != OMNI_EPI_RESID || NT == 1, "EPI_RESID: one n-tile per workgroup");
                // item == thread (ITEMS = MT * 64 <= 256): r_old was fetched for exactly this (m, n)
                const ResidOut ro = resid_values(v, pro.r_old, a.resid != nullptr);
                *reinterpret_cast<u32x2*>(reinterpret_cast<uint16_t*>(a.out) + frag_off(m, n, N)) = ro.r;
                if (l < 16) a.part_out[blockIdx.x * a.pstride + m] = ro.ss;   // slabs [n group][pstride rows]
            } else if (EPI == OMNI_EPI_BF16) {
                *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(a.out) + (a.oshuf ? frag_off(m, n, N) : (size_t)m * N + n)) =
                    make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
            } else {
                float4 o;
                float* po = reinterpret_cast<float*>(&o);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    float y = (EPI == OMNI_EPI_F32_BF16RND) ? bfround(v[g]) : v[g];
                    if (a.mask && !a.mask[n + g]) y = a.mask_fill;
                    po[g] = y;
                }
                *reinterpret_cast<float4*>(reinterpret_cast<float*>(a.out) + (size_t)m * N + n) = o;
            }
        }
    }
}
