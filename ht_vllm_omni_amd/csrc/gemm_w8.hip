// Skinny-M (M <= 64) weight-streaming GEMM on fp8 e4m3fn weights: out[M,N] = x[M,K] . W_eff[N,K]^T with
// W_eff = bf16(fp8 * row scale) rebuilt in registers -- the dense backbone's decode GEMMs at one byte per weight.
//
// Contract: every entry point here returns bit for bit what the bf16 entry point of gemm.hip returns on W_eff.  That fixes
// the arithmetic, not the data movement: wave w of 8 accumulates k-steps w, w + 8, w + 16, ... of 32 in ascending order on
// v_mfma_f32_16x16x32_bf16, the 8 partials are summed in wave order through LDS, the deferred rstd (PRO 3) multiplies the
// fp32 sums, the sum(r^2) slabs are one per 16-column group.  The epilogues below repeat gemm.hip's statements for that reason.
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

#define W8_WAVES 8
#define W8_THREADS (W8_WAVES * 64)

struct W8Args {
    const uint16_t* x; int ldx;
    const uint8_t* W; const float* scale; const uint16_t* bias; void* out;
    int M, N, K;
    const uint16_t* resid; const uint16_t* norm_w; float eps;     // EPI_RESID: the stream to add into (NULL: start one); PRO 3: norm weight
    int xshuf, oshuf;                                             // fragment-major x / out
    const float* part_in; int np_in; float* part_out;             // sum(r^2) slabs [np][64] in (PRO 3) / out (EPI_RESID)
};

// 8 fp8 bytes of one row -> the MFMA A fragment of bf16(fp8 * scale)
__device__ __forceinline__ u32x4 w8_deq(uint32_t lo, uint32_t hi, float s) {
    float f[8];
    unpack_fp8x4(lo, f);
    unpack_fp8x4(hi, f + 4);
    u32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = pack_bf2(f[2 * j] * s, f[2 * j + 1] * s);
    return o;
}

template <int MT, int NT, int PRO, int EPI, bool NTL>
__global__ __launch_bounds__(W8_THREADS) void gemm_w8_kernel(const W8Args a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];   // [WAVES][NT*MT][64] f32x4 (+ [WAVES][64] slab partials)
    static_assert(PRO == 0 || PRO == 3, "W8: plain or deferred-rstd prologue");
    static_assert(EPI == OMNI_EPI_BF16 || EPI == OMNI_EPI_RESID || EPI == OMNI_EPI_SILU_MUL_GU8, "W8: bf16 epilogues");
    static_assert(EPI != OMNI_EPI_RESID || NT == 1, "EPI_RESID: one n-tile per workgroup");
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int K = a.K, N = a.N;
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
    constexpr bool NORM = PRO == 3;
    constexpr int XROWS = MT * 16, NCH = W8_THREADS / XROWS;
    typedef SlabOrder<XROWS> SO;
    float pv[SO::PE];
    float psum = 0.f;
    if (NORM) {
        const int row = lane % XROWS, sub = lane / XROWS, ch = threadIdx.x / XROWS;
        const float* pp = a.part_in + m_base + row;
#pragma unroll
        for (int e = 0; e < SO::PE; ++e) {
            const int p = SO::index(wave, sub, e);
            pv[e] = pp[(size_t)min(p, a.np_in - 1) * 64];
            if (p >= a.np_in) pv[e] = 0.f;
        }
        for (int p = ch + 128; p < a.np_in; p += NCH) psum += pp[(size_t)p * 64];
    }
    uint2 r_old = make_uint2(0, 0);                               // EPI_RESID: the old residual values of this thread's epilogue item
    if (EPI == OMNI_EPI_RESID && a.resid && threadIdx.x < MT * 64) {
        const int ml = (threadIdx.x >> 6) * 16 + (lane & 15);
        if (ml < Mloc)
            r_old = *reinterpret_cast<const uint2*>(a.resid + frag_off(m_base + ml, blockIdx.x * 16 + 4 * (lane >> 4), N));
    }

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
        for (int j = 0; j < NT; ++j) A[j] = w8_deq(Wq[d][j][0], Wq[d][j][1], sc[j]);
        mma_step(A, Xa[d], NWa[d]);
#pragma unroll
        for (int j = 0; j < NT; ++j) B[j] = w8_deq(Wq[d][j][2], Wq[d][j][3], sc[j]);      // under the MFMAs of the first step
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
                for (int j = 0; j < NT; ++j) A[j] = w8_deq(Wt[h][j][0], Wt[h][j][1], sc[j]);
                mma_step(A, Xt[h], NWt[h]);
            }
        }
    }

    // PRO 3: the slab reduction behind the MFMA loop -> one partial per wave and row, read by the epilogue (gemm.hip xnorm_rstd, DEFER)
    if (NORM) {
        float s_ = SO::reduce(pv);
        if (a.np_in > 128) {
            if (XROWS <= 32) psum = xor32_sum(psum);
            if (XROWS <= 16) psum = xor16_sum(psum);
            s_ += psum;
        }
        lds[W8_WAVES * NT * MT * 4 * 64 + wave * 64 + lane] = s_;
    }

    // ---- combine the 8 K-partials through LDS in wave order, then the epilogue: gemm.hip's statements
    f32x4* lds4 = reinterpret_cast<f32x4*>(lds);
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < MT; ++i) lds4[(wave * (NT * MT) + j * MT + i) * 64 + lane] = acc[j][i];
    __syncthreads();

    constexpr bool GU8 = EPI == OMNI_EPI_SILU_MUL_GU8;
    constexpr int LN = GU8 ? 32 : 64;
    constexpr int ITEMS = NT * MT * LN;
    for (int it = threadIdx.x; it < ITEMS; it += W8_THREADS) {
        const int l = it % LN;
        const int t = it / LN;
        const int i = t % MT, j = t / MT;
        const int ml = i * 16 + (l & 15);
        if (ml >= Mloc) continue;
        const int m = m_base + ml;
        f32x4 sum = (f32x4){0.f, 0.f, 0.f, 0.f}, sum2 = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int w = 0; w < W8_WAVES; ++w) {
            sum += lds4[(w * (NT * MT) + j * MT + i) * 64 + l];
            if (GU8) sum2 += lds4[(w * (NT * MT) + j * MT + i) * 64 + l + 32];
        }
        if (NORM) {
            const float* red = lds + W8_WAVES * NT * MT * 4 * 64;
            float tsum = 0.f;
#pragma unroll
            for (int w = 0; w < W8_WAVES; ++w) tsum += red[w * 64 + ml];
            const float rl = 1.0f / sqrtf(tsum / (float)K + a.eps);
            sum *= rl;
            if (GU8) sum2 *= rl;
        }
        float v[4], v2[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) { v[g] = sum[g]; v2[g] = sum2[g]; }
        if (GU8) {
            const int n = (blockIdx.x * NT + j) * 8 + 4 * (l >> 4);
            float o[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float gt = bfround(v[g]);
                const float up = bfround(v2[g]);
                const float sl = bfround(gt / (1.0f + expf(-gt)));
                o[g] = sl * up;
            }
            *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(a.out) + (a.oshuf ? frag_off(m, n, N) : (size_t)m * N + n)) =
                make_uint2(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]));
        } else {
            const int n = blockIdx.x * 16 * NT + j * 16 + 4 * (l >> 4);
            if (a.bias) {
#pragma unroll
                for (int g = 0; g < 4; ++g) v[g] += bf2f(a.bias[n + g]);
            }
            if (EPI == OMNI_EPI_RESID) {
                uint16_t* rp = reinterpret_cast<uint16_t*>(a.out) + frag_off(m, n, N);
                float rv[4];
#pragma unroll
                for (int g = 0; g < 4; ++g) rv[g] = bfround(v[g]);
                if (a.resid) {     // item == thread (ITEMS = MT * 64 <= 256): r_old was fetched for exactly this (m, n)
                    rv[0] = bfround(bf_lo(r_old.x) + rv[0]); rv[1] = bfround(bf_hi(r_old.x) + rv[1]);
                    rv[2] = bfround(bf_lo(r_old.y) + rv[2]); rv[3] = bfround(bf_hi(r_old.y) + rv[3]);
                }
                *reinterpret_cast<uint2*>(rp) = make_uint2(pack_bf2(rv[0], rv[1]), pack_bf2(rv[2], rv[3]));
                float ss = sq4_sum(rv[0], rv[1], rv[2], rv[3]);
                ss = xor32_sum(xor16_sum(ss));       // the 4 lanes (l & 15) + 16 * {0..3} hold the 16 columns of row m
                if (l < 16) a.part_out[blockIdx.x * 64 + m] = ss;
            } else {
                *reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(a.out) + (a.oshuf ? frag_off(m, n, N) : (size_t)m * N + n)) =
                    make_uint2(pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]));
            }
        }
    }
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

// Tile policy: gemm.hip's pick_tile for the forms that exist here (the bits do not depend on it; the starting point for a W8 sweep).
// Plain / residual GEMMs: NT = 1, M split over grid.y until ~256 workgroups.  Norm-fused: wide n groups where there are enough columns,
// since every n group rebuilds the normalised rows it multiplies.
static void pick_tile_w8(bool norm, bool gu8, const W8Args& a, int* nt_out, int* mt_out, int* splits_out) {
    const int mt_total = (a.M + 15) / 16;
    const int cols = gu8 ? a.N / 8 : a.N / 16;
    int nt = gu8 ? 2 : 1;
    if (norm) {
        nt = (cols % 4 == 0 && cols / 4 >= 64) ? 4 : ((cols % 2 == 0 && cols / 2 >= 32) ? 2 : nt);
        if (!gu8 && nt == 4 && cols / 4 == 64 && a.K >= 2048 && mt_total >= 3) nt = 2;      // the backbone's qkv: 128 groups x 2 m-splits
        if (gu8 && cols % 3 == 0 && cols / 3 >= 128) nt = 3;                                // 256 workgroups at the backbone's gate_up
    }
    const int groups = gu8 ? a.N / (8 * nt) : a.N / (16 * nt);
    int splits = groups >= 160 ? 1 : (256 + groups - 1) / groups;
    if (norm && gu8 && nt == 3 && groups == 128 && mt_total == 3) splits = 3;
    if (splits > mt_total) splits = mt_total;
    int mt = (mt_total + splits - 1) / splits;       // 1..4
    if (mt == 3) mt = 4;
    if (nt == 4 && mt == 4) mt = 2;                  // 16 accumulator tiles + the ring of a pair per slot do not fit 256 registers: two m-splits
    *nt_out = nt; *mt_out = mt; *splits_out = (mt_total + mt - 1) / mt;
}

template <int PRO, int EPI>
static int dispatch_w8(const W8Args& a, hipStream_t st) {
    int nt, mt, splits;
    pick_tile_w8(PRO == 3, EPI == OMNI_EPI_SILU_MUL_GU8, a, &nt, &mt, &splits);
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
