// Skinny-M (M <= 64) weight-streaming GEMM on fp8 e4m3fn weights: out[M,N] = x[M,K] . W_eff[N,K]^T with
// W_eff = bf16(fp8 * row scale) rebuilt in registers -- the dense backbone's decode GEMMs at one byte per weight.
//
// Contract: every entry point here returns bit for bit what the bf16 entry point of gemm.hip returns on W_eff.  That fixes
// the arithmetic, not the data movement: wave w of 8 accumulates k-steps w, w + 8, w + 16, ... of 32 in ascending order on
// v_mfma_f32_16x16x32_bf16, the 8 partials are summed in wave order through LDS, the deferred rstd (PRO 3) multiplies the
// fp32 sums, the sum(r^2) slabs are one per 16-column group.  Everything in front of and behind the MFMA loop IS gemm.hip's code
// (skinny_epi.cuh); this file holds the layout, the ring and the dequantisation.
//
// W8 fragment layout (include/omni_talker.h OMNI W8 layout): per 16-row tile, K bytes x 16 rows contiguous.  k-steps come in
// groups of 16 (512 k): the group's 8 KB are eight 1-KB blocks, block w = the two k-steps s = 16 g + w and s + 8 -- the two
// CONSECUTIVE steps of their owning wave -- as 16 B per lane: lane (r = l & 15, q = l >> 4) holds W[r][32 s + 8 q .. + 8) then
// W[r][32 (s + 8) + 8 q .. + 8).  One wave-level 16-B load = 1 KB contiguous = that wave's next two MFMA groups, in 4 VGPRs where
// bf16 needs 8.  The k-steps past the last whole group (K % 512 != 0: no talker shape, the `tiny` preset and tests) follow as
// 512-B blocks of 8 B per lane in step order: the file is a permutation of the [N, K] bytes, nothing is padded, and a wave owns
// at most two such steps.
//
// Schedule: a ring of D pairs (D KB per n-tile per wave: the bytes the bf16 kernel keeps in flight, covering twice the k-steps)
// of W AND the x fragments of both steps; nothing in the counted loop is predicated, so every MFMA group waits for exactly the
// loads issued D pairs earlier.  Pair counts that are no multiple of D run their first (pairs % D) pairs as one unpipelined
// batch through the same registers.  Lane (r, q) owns row r of a tile: one scale register per tile; per 8 weights the
// dequantisation is 4 cvt_pk_f32_fp8 + 8 multiplies + 4 cvt_pk_bf16_f32, issued per k-step so that the second step's conversion
// sits under the first step's MFMAs (NT x MT independent MFMAs per converted fragment set).
#include "common.cuh"
#include "kernels.h"
#include "gemm_frag.cuh"
#include "skinny_epi.cuh"
#include "gemm_tile_policy.h"

#define W8_WAVES SKINNY_WAVES
#define W8_THREADS SKINNY_THREADS

struct W8Args : SkinnyArgs {          // (pstride = 64: the slabs are [np][64] here)
    const uint16_t* x; int ldx;
    const uint8_t* W; const float* scale;
    const uint16_t* norm_w;           // PRO 3: norm weight
    int xshuf;                        // fragment-major x
};

template <int MT, int NT, int PRO, int EPI, bool NTL>
__global__ __launch_bounds__(W8_THREADS) void gemm_w8_kernel(const W8Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];   // [WAVES][NT*MT][64] f32x4 (+ [WAVES][64] slab partials)
    static_assert(PRO == 0 || PRO == 3, "W8: plain or deferred-rstd prologue");
    static_assert(EPI == OMNI_EPI_BF16 || EPI == OMNI_EPI_RESID || EPI == OMNI_EPI_SILU_MUL_GU8, "W8: bf16 epilogues");
    static_assert(EPI != OMNI_EPI_RESID || NT == 1, "EPI_RESID: one n-tile per workgroup");
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int K = a.K;
    const int m_base = blockIdx.y * (MT * 16);
    const int Mloc = min(a.M - m_base, MT * 16);                  // valid rows of this workgroup (>= 1)
    const int nsteps = K >> 5;                                    // k-steps of 32
    const int npairs = nsteps >> 4;                               // pairs of this wave = whole 16-step groups
    const int tail0 = npairs << 4;                                // first k-step of the 8-B-per-lane remainder
    const int xstep = a.xshuf ? 512 : 32;

    const uint8_t* wtile[NT];
    float sc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int row0 = (blockIdx.x * NT + j) * 16;              // (GU8: rows of the interleaved [2 * inter, K] matrix)
        wtile[j] = a.W + (size_t)row0 * K;
        sc[j] = a.scale[row0 + r];
    }
    const uint16_t* xrow[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        int m = i * 16 + r;
        m = m_base + (m < Mloc ? m : Mloc - 1);                   // rows past M: valid address, result discarded
        const int xt = min((m_base >> 4) + i, ((a.M + 15) >> 4) - 1);      // fragment-major x holds ceil(M / 16) row tiles
        xrow[i] = a.xshuf ? a.x + ((size_t)xt * nsteps) * 512 + lane * 8 : a.x + (size_t)m * a.ldx + 8 * q;
    }

    f32x4 acc[NT][MT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[j][i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // PRO 3: this thread's share of the sum(r^2) slabs of the workgroup's rows, issued before the W ring (gemm.hip, PRO_XNORM part 1)
    // and EPI_RESID's old residual values
    constexpr bool NORM = PRO == 3;
    SkinnyPro<MT, NORM, EPI> pro;
    pro.load(a, m_base, Mloc);

    // ring depth in pairs: 2 KB per n-tile in flight per wave, 4 KB for the residual-epilogue tiles (one 16-column tile, long K,
    // every byte cold) where the x fragments of 8 k-steps still fit the register file
    constexpr int D = (EPI == OMNI_EPI_RESID && MT <= 2) ? 4 : 2;
    u32x4 Wq[D][NT], Xa[D][MT], Xb[D][MT], NWa[D], NWb[D];
    auto load_pair = [&](int d, int p) {
        const int sa = 16 * p + wave, sb = sa + 8;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const uint16_t* wp = reinterpret_cast<const uint16_t*>(wtile[j] + ((size_t)(p * 8 + wave) << 10) + lane * 16);
            Wq[d][j] = NTL ? ld16_nt(wp) : ld16(wp);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) Xa[d][i] = ld16(xrow[i] + sa * xstep);
        if (NORM) NWa[d] = ld16(a.norm_w + sa * 32 + 8 * q);
#pragma unroll
        for (int i = 0; i < MT; ++i) Xb[d][i] = ld16(xrow[i] + sb * xstep);
        if (NORM) NWb[d] = ld16(a.norm_w + sb * 32 + 8 * q);
    };
    auto mma_step = [&](const u32x4 (&A)[NT], u32x4 (&X)[MT], const u32x4& nw) {
        if (NORM) {
#pragma unroll
            for (int i = 0; i < MT; ++i) X[i] = xw_frag(X[i], nw);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int i = 0; i < MT; ++i) acc[j][i] = mfma16(A[j], X[i], acc[j][i]);
    };
    auto mma_pair = [&](int d) {
        u32x4 A[NT], B[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) A[j] = deq_fp8x8((u32x2){Wq[d][j][0], Wq[d][j][1]}, sc[j]);
        mma_step(A, Xa[d], NWa[d]);
#pragma unroll
        for (int j = 0; j < NT; ++j) B[j] = deq_fp8x8((u32x2){Wq[d][j][2], Wq[d][j][3]}, sc[j]);      // under the MFMAs of the first step
        mma_step(B, Xb[d], NWb[d]);
    };

    // the first (npairs % D) pairs: all loaded at once, then multiplied (talker shapes with K % (512 D) != 0; never the 1.7B backbone)
    const int rem = npairs % D;
#pragma unroll
    for (int d = 0; d < D - 1; ++d)
        if (d < rem) load_pair(d, d);
#pragma unroll
    for (int d = 0; d < D - 1; ++d)
        if (d < rem) mma_pair(d);
    // counted schedule over the other pairs (a multiple of D)
    const int G = npairs / D;
    if (G > 0) {
#pragma unroll
        for (int d = 0; d < D; ++d) load_pair(d, rem + d);
        for (int g = 0; g + 1 < G; ++g) {
#pragma unroll
            for (int d = 0; d < D; ++d) {
                mma_pair(d);
                load_pair(d, rem + (g + 1) * D + d);
            }
        }
#pragma unroll
        for (int d = 0; d < D; ++d) mma_pair(d);
    }
    // the k-steps past the last whole group: steps tail0 + wave and tail0 + wave + 8 where they exist, 8 B of W per lane each
    if (tail0 < nsteps) {
        u32x2 Wt[2][NT];
        u32x4 Xt[2][MT], NWt[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int s = tail0 + wave + 8 * h;
            if (s < nsteps) {
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    Wt[h][j] = *reinterpret_cast<const u32x2*>(wtile[j] + ((size_t)tail0 << 9) + ((size_t)(s - tail0) << 9) + lane * 8);
#pragma unroll
                for (int i = 0; i < MT; ++i) Xt[h][i] = ld16(xrow[i] + s * xstep);
                if (NORM) NWt[h] = ld16(a.norm_w + s * 32 + 8 * q);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (tail0 + wave + 8 * h < nsteps) {
                u32x4 A[NT];
#pragma unroll
                for (int j = 0; j < NT; ++j) A[j] = deq_fp8x8(Wt[h][j], sc[j]);
                mma_step(A, Xt[h], NWt[h]);
            }
        }
    }

    // ---- PRO 3: the slab reduction behind the MFMA loop; the combine of the 8 K-partials in wave order; the epilogue
    skinny_finish<MT, NT, PRO, EPI>(a, lds, acc, pro, m_base, Mloc, 0);
}

template <int MT, int NT, int PRO, int EPI>
static int launch_w8(const W8Args& a, int m_splits, hipStream_t st) {
    const int groups = EPI == OMNI_EPI_SILU_MUL_GU8 ? a.N / (8 * NT) : a.N / (16 * NT);
    const size_t lds = (size_t)W8_WAVES * NT * MT * 4 * 64 * sizeof(float) + (PRO == 3 ? W8_WAVES * 64 * sizeof(float) : 0);
    if (lds > 65536) {   // 8+ accumulator tiles: up to 98 KB of the CU's 160 KB (one workgroup per CU)
        static bool done = false;
        if (!done) {
            (void)hipFuncSetAttribute((const void*)gemm_w8_kernel<MT, NT, PRO, EPI, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
            (void)hipFuncSetAttribute((const void*)gemm_w8_kernel<MT, NT, PRO, EPI, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
            done = true;
        }
    }
    // non-temporal W loads only when each W byte is read by exactly one workgroup (no m-split)
    if (m_splits == 1)
        hipLaunchKernelGGL((gemm_w8_kernel<MT, NT, PRO, EPI, true>), dim3(groups, m_splits), dim3(W8_THREADS), lds, st, a);
    else
        hipLaunchKernelGGL((gemm_w8_kernel<MT, NT, PRO, EPI, false>), dim3(groups, m_splits), dim3(W8_THREADS), lds, st, a);
    OMNI_CHECK_LAUNCH("omni_gemm_w8");
    return OMNI_OK;
}

template <int PRO, int EPI>
static int dispatch_w8(const W8Args& a, hipStream_t st) {
    // the bf16 kernel's tile policy at its 256-workgroup target (the bits do not depend on it; the starting point for a W8 sweep)
    int mt, splits;
    const int nt = skinny_tile_nt(PRO == 3, EPI, a.M, a.N, a.K);
    skinny_tile_mt(PRO == 3, EPI, a.M, a.N, nt, 256, &mt, &splits);
    if (nt == 4 && mt == 4) {        // 16 accumulator tiles + the ring of a pair per slot do not fit 256 registers: two m-splits
        mt = 2;
        splits = skinny_tile_splits(a.M, &mt);
    }
#define TILE(N_, M_) if (nt == N_ && mt == M_) return launch_w8<M_, N_, PRO, EPI>(a, splits, st);
#define TILE_M(N_) TILE(N_, 1) TILE(N_, 2) TILE(N_, 4)
    if constexpr (EPI == OMNI_EPI_SILU_MUL_GU8) { TILE_M(2) TILE_M(3) TILE(4, 1) TILE(4, 2) }
    else if constexpr (PRO == 0) { TILE_M(1) }
    else { TILE_M(1) TILE_M(2) TILE(4, 1) TILE(4, 2) }
#undef TILE_M
#undef TILE
    omni_set_error("omni_gemm_w8: no kernel for tile NT=%d MT=%d (epilogue %d)", nt, mt, EPI);
    return OMNI_EINVAL;
}

static int check_w8(const W8Args& a, const char* who) {
    OMNI_CHECK_ARG(a.x && a.W && a.out, "%s: null pointer", who);
    OMNI_CHECK_ARG(a.scale, "%s: null scales (fp32 per output row)", who);
    OMNI_CHECK_ARG(a.M >= 1 && a.M <= 64, "%s: M=%d outside 1..64", who, a.M);
    OMNI_CHECK_ARG(a.N > 0 && a.N % 16 == 0, "%s: N=%d not a multiple of 16", who, a.N);
    OMNI_CHECK_ARG(a.K > 0 && a.K % 32 == 0, "%s: K=%d not a multiple of 32", who, a.K);
    return OMNI_OK;
}

extern "C" int omni_gemm_w8(const void* x, int ldx, const void* w8, const float* w_scale, const void* bias, void* out, int M, int N,
                            int K, int layout, void* stream) {
    W8Args a{};
    a.pstride = 64;
    a.xshuf = (layout & OMNI_LAYOUT_X_FRAG) != 0;
    a.oshuf = (layout & OMNI_LAYOUT_OUT_FRAG) != 0;
    a.x = (const uint16_t*)x; a.ldx = ldx; a.W = (const uint8_t*)w8; a.scale = w_scale; a.bias = (const uint16_t*)bias; a.out = out;
    a.M = M; a.N = N; a.K = K;
    int rc = check_w8(a, "omni_gemm_w8");
    if (rc != OMNI_OK) return rc;
    OMNI_CHECK_ARG(a.xshuf || (ldx >= K && ldx % 8 == 0), "omni_gemm_w8: ldx=%d (need >= K, multiple of 8)", ldx);
    OMNI_CHECK_ARG(!a.oshuf || N % 32 == 0, "omni_gemm_w8: fragment-major output needs N %% 32 == 0");
    return dispatch_w8<0, OMNI_EPI_BF16>(a, (hipStream_t)stream);
}

extern "C" int omni_gemm_resid_w8(const void* x_frag, const void* w8, const float* w_scale, void* r_io, int accumulate, float* partials,
                                  int M, int N, int K, void* stream) {
    W8Args a{};
    a.pstride = 64;
    a.xshuf = 1; a.oshuf = 1;
    a.x = (const uint16_t*)x_frag; a.ldx = K; a.W = (const uint8_t*)w8; a.scale = w_scale; a.out = r_io;
    a.resid = accumulate ? (const uint16_t*)r_io : nullptr;
    a.part_out = partials;
    a.M = M; a.N = N; a.K = K;
    int rc = check_w8(a, "omni_gemm_resid_w8");
    if (rc != OMNI_OK) return rc;
    OMNI_CHECK_ARG(partials, "omni_gemm_resid_w8: null partials");
    OMNI_CHECK_ARG(N % 32 == 0, "omni_gemm_resid_w8: N=%d not a multiple of 32 (fragment-major residual stream)", N);
    return dispatch_w8<0, OMNI_EPI_RESID>(a, (hipStream_t)stream);
}

extern "C" int omni_gemm_xnorm_w8(const void* r, const float* partials, int nparts, const void* norm_w, float eps, const void* w8,
                                  const float* w_scale, void* out, int M, int N, int K, int epilogue, int out_frag, void* stream) {
    W8Args a{};
    a.pstride = 64;
    a.xshuf = 1; a.oshuf = out_frag != 0;
    a.x = (const uint16_t*)r; a.ldx = K; a.W = (const uint8_t*)w8; a.scale = w_scale; a.out = out;
    a.M = M; a.N = N; a.K = K;
    a.norm_w = (const uint16_t*)norm_w; a.eps = eps;
    a.part_in = partials; a.np_in = nparts;
    int rc = check_w8(a, "omni_gemm_xnorm_w8");
    if (rc != OMNI_OK) return rc;
    OMNI_CHECK_ARG(partials && norm_w && nparts >= 1, "omni_gemm_xnorm_w8: null pointer / nparts=%d", nparts);
    OMNI_CHECK_ARG(epilogue == OMNI_EPI_BF16 || epilogue == OMNI_EPI_SILU_MUL_GU8, "omni_gemm_xnorm_w8: epilogue %d unsupported", epilogue);
    OMNI_CHECK_ARG(!a.oshuf || N % 32 == 0, "omni_gemm_xnorm_w8: fragment-major output needs N %% 32 == 0");
    if (epilogue == OMNI_EPI_SILU_MUL_GU8) return dispatch_w8<3, OMNI_EPI_SILU_MUL_GU8>(a, (hipStream_t)stream);
    return dispatch_w8<3, OMNI_EPI_BF16>(a, (hipStream_t)stream);
}
