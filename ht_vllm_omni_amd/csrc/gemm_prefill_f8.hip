// W8A8 prefill GEMM on the fp8 matrix path of gfx950: out[M, N] = epilogue((q_x . q_w^T) * s_x[m] * s_w[n]) with both operands e4m3fn
// bytes, v_mfma_f32_16x16x128_f8f6f4 (128 k per instruction from 32 B per lane, fp32 accumulate: twice the bf16 MFMA's rate), and the
// row quantiser that produces q_x.  The arithmetic of `quantization: fp8` as vLLM runs it: dynamic per-token activation scales against
// per-channel weight scales.
//
// Arithmetic contract (include/omni_talker.h, omni_quant_rows_fp8 / omni_gemm_tile_fp8):
//   quantiser  s_x[m] = max(max_k |a[m, k]|, 1e-12) / 448 (fp32);  q_x[m, k] = e4m3fn(a[m, k] / s_x[m]) -- IEEE fp32 division, round to
//              nearest even, saturating at +-448: engine.fp8_quant_rows.  With the norm prologue a = omni_rmsnorm's output row, computed
//              by the same code (norm_row.cuh) and never stored.
//   GEMM       acc[m, n] = sum_k q_x[m, k] q_w[n, k] (the products are exact, fp32 accumulation inside the MFMA, one MFMA per 128 k in
//              ascending order);  y = (acc * s_x[m]) * s_w[n] in fp32;  out = bf16(y), or for the GU8 row order
//              bf16(bf16(SiLU(bf16 gate)) * bf16 up) (omni_silu_mul's rounding points, tile_epi.cuh).
//
// No second copy of the weights.  W is the decode step's W8 matrix (gemm_w8.hip; the W8 fragment layout of include/omni_talker.h).  A dot
// product does not care about the order of k as long as both operands use the same one, and in the W8 layout lane (k % 32) / 8 * 16 +
// row % 16 of the two consecutive 1-KB blocks 2 j, 2 j + 1 of a 16-step group holds 32 bytes: 8 k of each of the k-steps {2 j, 2 j + 8,
// 2 j + 1, 2 j + 9} -- precisely one operand of the 16x16x128 MFMA (lane = row + 16 * k-group, 8 VGPRs, 128 distinct k over the four
// lane groups).  The K % 512 remainder lives in 512-B blocks of 8 B per lane; four consecutive ones give an operand the same way.  So a
// 16-row tile is K / 128 CHUNKS of 2 KB, chunk c = the operand of MFMA c, and the quantiser writes the activations in the same layout
// with tokens in place of output rows (pad rows of the last 16-row tile zero).
//
// Data movement.  Both operands are linear runs in HBM: a workgroup's slice (128 k) of an n-tile or m-tile is one 2-KB chunk, staged by
// LDS-DMA as a straight copy (buffer_load_dwordx4 ... lds, two 1-KB wave instructions per chunk, no VGPR staging); tiles past N or past
// the last live 16-row tile of x are out of the descriptor's range and read as zero.  The per-lane picking happens on the way out of
// LDS: two ds_read_b128 (lane * 16 in each KB of a main chunk) or four ds_read_b64 (lane * 8 in each 512-B block of a remainder
// chunk), all lane-linear and conflict-free.  Ring of NBUF slices: slice t + NBUF - 1 is staged at the top of slice t, behind the ONE
// barrier of the slice, whose counted wait (vmcnt = the NBUF - 2 younger slices still in flight, lgkmcnt(0) for this wave's reads of the
// buffer about to be overwritten) makes slice t visible.  A 128-deep slice of a 256 x 256 tile is 64 KB -- two fit, and each has a whole
// slice of MFMAs (32 per wave, 2 048 cycles per SIMD) to land; the 128 x 64 tile keeps four.  A wave holds its WM x fragments (8 VGPRs
// each) for the slice and streams its WN W fragments past them: WN * WM MFMAs per WN + WM fragment reads.
// W is the MFMA's A operand: D[n][m], lane holds m = l & 15, n = 4 (l >> 4) + reg -- s_w belongs to the accumulator REGISTER, s_x to the
// LANE; both are applied once, behind the loop, and the bf16 kernels' epilogue (tile_epi.cuh) stores the tile.
// Every geometry adds k in the same order (one MFMA per chunk, chunks ascending): bit-identical outputs.
// Shared with the bf16 kernels and written once in tile_epi.cuh: geometry (F8Geom), tile order, launcher, the MoE gate / up pairing and
// finishes, the epilogue.  Which geometry a launch takes: tile_choice_fp8, gemm_tile_policy.h.
//
// MoE prefill on fp8 expert weights (MOE != 0 instantiations; entry point omni_moe_prefill_experts_fp8 in moe_prefill.hip): the grouped
// gate_up and down GEMMs over the compact expert-sorted batch of omni_moe_align (one m block = 64 or 256 rows of ONE expert), on the bytes
// and row scales the decode step's omni_moe_experts_ex reads -- no copy of the expert weights.
//   W  An expert matrix is frag_shuffle(q8): one byte per weight in the bf16 fragment order (frag_off, common.cuh), i.e. a 16-row tile is
//      K / 32 consecutive 512-B blocks of 8 B per lane (q * 16 + r) -- w8_off8 with P = 0: EVERY chunk is a remainder chunk, whatever K is
//      (no main part is derived from K >> 9).  Chunk c = k-steps 4 c .. 4 c + 3, a straight 2-KB LDS-DMA copy, read back with four
//      ds_read_b64: register pair e of lane (q, r) holds k = 128 c + 32 e + 8 q + j.  Expert base = expert * N * K bytes, scales [E, N].
//   x  LDS-DMA moves 16 B per lane, not 8, so the activations are quantised into a layout of their own (quant_rows_f8_kernel<.., TOK>):
//      token-major [rows, K] with k permuted inside every 128-k chunk -- byte 32 q + 8 e + j of the chunk holds k = 32 e + 8 q + j.  Lane
//      (c, q) fetches the two 16-B pieces at byte 32 q of its SOURCE row (gate_up: row_token[batch row], the gather; down: the act row as
//      it lies); the two instructions leave the image f8_frag<true> reads, registers [e0 e1 | e2 e3]: the same k as W's, pair for pair.
//      Rows with row_token < 0 and rows past the descriptor read as zero.  No VGPR staging on either operand.
//   Arithmetic contract (include/omni_talker.h, omni_moe_prefill_experts_fp8):
//      gate_up  g = (acc * s_x[token]) * s_w[n] in fp32 for gate and for up, act = bf16(bf16(SiLU(bf16 g_gate)) * bf16 g_up)
//               (omni_silu_mul's three roundings), gate and up paired as in the bf16 kernel (tile_src_ntile, tile_moe_finish: tile_epi.cuh);
//      down     y = bf16(bf16((acc * s_a[row]) * s_w[n]) * row_weight[row]) (MOE_DOWN's two roundings, tile_moe_finish);
//      k order  one MFMA per chunk, ascending, in both geometries (128 x 64 for 64-row blocks, 256 x 256 for 256-row blocks).
//   The act quantiser skips the rows of blocks without an expert (never written by gate_up; the down GEMM leaves those blocks at once);
//   pad rows inside an expert's block are zeros: zero bytes, scale 1e-12 / 448.
#include <type_traits>

#include "common.cuh"
#include "gemm_frag.cuh"
#include "gemm_tile_policy.h"
#include "kernels.h"
#include "norm_row.cuh"
#include "tile_epi.cuh"

typedef int i32x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------------------------- row quantiser
#define QR_ROWS_PER_BLOCK 4

// byte offset of the 8 bytes (row, k0 .. k0 + 7), k0 % 8 == 0, in the W8 fragment layout of a [rows, K] matrix
__device__ __forceinline__ size_t w8_off8(int row, int k0, int K) {
    const int s = k0 >> 5, q = (k0 & 31) >> 3, r = row & 15, P = K >> 9;
    const size_t tile = (size_t)(row >> 4) * 16 * K;
    if (s < 16 * P) return tile + ((s >> 4) * 8 + (s & 7)) * 1024 + (q * 16 + r) * 16 + ((s >> 3) & 1) * 8;
    return tile + (size_t)P * 8192 + (s - 16 * P) * 512 + (q * 16 + r) * 8;
}

// One wave per row, the row in registers (lane l: the 8-element vectors l, l + 64, ...): [norm ->] max |a| -> scale -> 8 bytes per vector.
// Rows [M, ceil16(M)) are written as zeros (the GEMM's pad rows).
// TOK: the MoE prefill's token-major layout (file header) instead -- no pad rows, and with block_expert the rows of blocks (`block` rows
// each) that no expert owns are left alone.
template <int MAXV, bool NORM, bool TOK = false>
__global__ __launch_bounds__(64 * QR_ROWS_PER_BLOCK) void quant_rows_f8_kernel(const uint16_t* __restrict__ x, int ldx, const uint16_t* __restrict__ delta,
                                                                               uint16_t* residual, const uint16_t* __restrict__ norm_w, float eps,
                                                                               uint8_t* __restrict__ q, float* __restrict__ scale, int M, int K,
                                                                               const int32_t* __restrict__ block_expert = nullptr, int block = 1) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * QR_ROWS_PER_BLOCK + (threadIdx.x >> 6);
    if (row >= (TOK ? M : ((M + 15) & ~15))) return;
    if constexpr (TOK)
        if (block_expert && block_expert[row / block] < 0) return;
    const int nvec = K >> 3;
    uint4 pk[MAXV];                       // the row as packed bf16
#pragma unroll
    for (int i = 0; i < MAXV; ++i) pk[i] = make_uint4(0, 0, 0, 0);
    if (row < M) {
        if constexpr (NORM) {
            const size_t ro = (size_t)row * K;
            NormRow<MAXV> nr;
            const float rstd = nr.load(residual ? residual + ro : x + (size_t)row * ldx, delta ? delta + ro : nullptr, residual ? residual + ro : nullptr,
                                       false, norm_w, K, eps, lane);
#pragma unroll
            for (int i = 0; i < MAXV; ++i)
                if (lane + i * 64 < nvec) pk[i] = nr.normed(i, rstd);
        } else {
#pragma unroll
            for (int i = 0; i < MAXV; ++i)
                if (lane + i * 64 < nvec) pk[i] = *reinterpret_cast<const uint4*>(x + (size_t)row * ldx + (lane + i * 64) * 8);
        }
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const uint32_t* w = reinterpret_cast<const uint32_t*>(&pk[i]);
#pragma unroll
        for (int j = 0; j < 4; ++j) amax = fmaxf(amax, fmaxf(fabsf(bf_lo(w[j])), fabsf(bf_hi(w[j]))));
    }
    amax = wave_max(amax);
    const float s = fmaxf(amax, 1e-12f) / OMNI_FP8_MAX;
    if (row < M && lane == 0) scale[row] = s;
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int vi = lane + i * 64;
        if (vi < nvec) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(&pk[i]);
            u32x2 o;
            o[0] = pack_fp8x4(bf_lo(w[0]) / s, bf_hi(w[0]) / s, bf_lo(w[1]) / s, bf_hi(w[1]) / s);
            o[1] = pack_fp8x4(bf_lo(w[2]) / s, bf_hi(w[2]) / s, bf_lo(w[3]) / s, bf_hi(w[3]) / s);
            // TOK: vector vi = k 8 vi .. + 7 = (chunk vi >> 4, e = (vi >> 2) & 3, q = vi & 3) -> byte 32 q + 8 e of the row's chunk
            const size_t off = TOK ? (size_t)row * K + (vi >> 4) * 128 + (vi & 3) * 32 + ((vi >> 2) & 3) * 8 : w8_off8(row, vi * 8, K);
            *reinterpret_cast<u32x2*>(q + off) = o;
        }
    }
}

// the launch: MAXV = the smallest instantiation that holds the row's K / 8 vectors, 64 lanes x MAXV (the norm prologue stops at 8: K <= 4096);
// grid over the rows the kernel writes (pad rows included, TOK has none)
template <bool NORM, bool TOK>
static void quant_rows_launch(const void* x, int ldx, const void* delta, void* residual, const void* norm_w, float eps, void* q, float* scale, int M,
                              int K, const int32_t* block_expert, int block, hipStream_t st) {
    const dim3 grid(((TOK ? M : (M + 15) & ~15) + QR_ROWS_PER_BLOCK - 1) / QR_ROWS_PER_BLOCK);
    const int nvec = K / 8;
#define QR_LAUNCH(V)                                                                                                                          \
    hipLaunchKernelGGL((quant_rows_f8_kernel<V, NORM, TOK>), grid, dim3(64 * QR_ROWS_PER_BLOCK), 0, st, (const uint16_t*)x, ldx, (const uint16_t*)delta, \
                       (uint16_t*)residual, (const uint16_t*)norm_w, eps, (uint8_t*)q, scale, M, K, block_expert, block)
    if (nvec <= 64 * 2) QR_LAUNCH(2);
    else if (nvec <= 64 * 4) QR_LAUNCH(4);
    else if (NORM || nvec <= 64 * 8) QR_LAUNCH(8);
    else if constexpr (!NORM) QR_LAUNCH(16);
#undef QR_LAUNCH
}

extern "C" int omni_quant_rows_fp8(const void* x, int ldx, const void* delta, void* residual, const void* norm_w, float eps, void* q_frag,
                                   float* x_scale, int M, int K, void* stream) {
    OMNI_CHECK_ARG(q_frag && x_scale && (x || residual), "omni_quant_rows_fp8: null pointer");
    OMNI_CHECK_ARG(M >= 1 && K > 0 && K % 128 == 0, "omni_quant_rows_fp8: M=%d K=%d (M >= 1, K %% 128 == 0)", M, K);
    OMNI_CHECK_ARG(norm_w || (!delta && !residual), "omni_quant_rows_fp8: delta / residual belong to the norm prologue (norm_w is null)");
    OMNI_CHECK_ARG(!delta || residual, "omni_quant_rows_fp8: delta needs residual");
    OMNI_CHECK_ARG(residual || (ldx >= K && ldx % 8 == 0), "omni_quant_rows_fp8: ldx=%d (>= K, multiple of 8)", ldx);
    OMNI_CHECK_ARG(K <= (norm_w ? 4096 : 8192), "omni_quant_rows_fp8: K=%d too wide for a row in registers (norm prologue: 4096, plain: 8192)", K);
    if (norm_w) quant_rows_launch<true, false>(x, ldx, delta, residual, norm_w, eps, q_frag, x_scale, M, K, nullptr, 1, (hipStream_t)stream);
    else quant_rows_launch<false, false>(x, ldx, delta, residual, norm_w, eps, q_frag, x_scale, M, K, nullptr, 1, (hipStream_t)stream);
    OMNI_CHECK_LAUNCH("omni_quant_rows_fp8");
    return OMNI_OK;
}

int k_quant_rows_f8_tok(const void* x, int ldx, void* q, float* scale, int M, int K, const int32_t* block_expert, int block, void* stream) {
    OMNI_CHECK_ARG(x && q && scale && M >= 1 && K > 0 && K % 128 == 0 && K <= 8192 && ldx >= K && ldx % 8 == 0 && block >= 1,
                   "omni_moe_prefill_experts_fp8: quantiser M=%d K=%d ldx=%d (K %% 128 == 0, K <= 8192)", M, K, ldx);
    quant_rows_launch<false, true>(x, ldx, nullptr, nullptr, nullptr, 0.f, q, scale, M, K, block_expert, block, (hipStream_t)stream);
    OMNI_CHECK_LAUNCH("omni_moe_prefill_experts_fp8(quantiser)");
    return OMNI_OK;
}

// ---------------------------------------------------------------------------------------------------------------- tile GEMM
struct F8Args {
    const uint8_t* x8; const float* xs;
    const uint8_t* W; const float* ws;
    uint16_t* out; int ldo;
    int M, N, K;
    int mblocks, nblocks, band;
    // MOE != 0 (file header): x8 = x_rows token-major rows, xs per source row; W / ws per expert ([E, N, K] bytes, [E, N] scales); the maps of
    // omni_moe_align -- m block b belongs to expert block_expert[b] (< 0: none, the workgroup leaves), batch row r reads token row_token[r]
    // (gate_up; < 0: zeros) and carries the routing weight row_weight[r] (down)
    int x_rows;
    const int32_t* block_expert; const int32_t* row_token; const uint16_t* row_weight;
};

// Geometry F8Geom<WAVES_N, WN, WM> (tile_epi.cuh): one slice = a 128-deep 2-KB chunk of every tile of both operands, two LDS-DMA
// instructions per chunk.

// one MFMA operand out of a 2-KB chunk image: a main chunk (two 1-KB blocks of 16 B per lane) or a remainder chunk (four 512-B blocks
// of 8 B per lane); W and x chunks of one slice are of the same kind, so register e of both operands holds the same k
template <bool MAIN>
__device__ __forceinline__ i32x8 f8_frag(const uint8_t* chunk, int lane) {
    if constexpr (MAIN) {
        const u32x4 lo = *reinterpret_cast<const u32x4*>(chunk + lane * 16), hi = *reinterpret_cast<const u32x4*>(chunk + 1024 + lane * 16);
        return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
    } else {
        u32x2 b[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) b[e] = *reinterpret_cast<const u32x2*>(chunk + e * 512 + lane * 8);
        return i32x8{(int)b[0][0], (int)b[0][1], (int)b[1][0], (int)b[1][1], (int)b[2][0], (int)b[2][1], (int)b[3][0], (int)b[3][1]};
    }
}

// (scale operands 0 / 0 with cbsz = blgp = 0 select the unscaled fp8 x fp8 instruction)
__device__ __forceinline__ f32x4 f8_mfma(i32x8 a, i32x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0, 0, 0, 0);
}

template <int WAVES_N, int WN, int WM, bool GU8, int MOE = 0>
__global__ __launch_bounds__(TG_THREADS) void gemm_tile_f8_kernel(const F8Args a) {
    using G = F8Geom<WAVES_N, WN, WM>;
    constexpr int NTILES = G::NTILES, MTILES = G::MTILES, SLICE = G::SLICE, NLW = G::NLW, NLX = G::NLX, NBUF = G::NBUF;
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wn = wave % WAVES_N, wm = wave / WAVES_N;
    const int c = lane & 15, q = lane >> 4;
    int n_blk, m_blk;
    tile_block(a.band, a.mblocks, a.nblocks, n_blk, m_blk);
    const int m0 = m_blk * G::BM, n0 = n_blk * G::BN;
    const uint8_t* W = a.W;
    const float* ws = a.ws;
    if constexpr (MOE != 0) {
        const int expert = a.block_expert[m_blk];                             // uniform: one expert per m block
        if (expert < 0) return;                                               // past the last expert's rows
        W += (size_t)expert * a.N * a.K;
        ws += (size_t)expert * a.N;
    }
    const int nsteps = a.K >> 7;                                              // chunks = slices = MFMAs per output tile
    const int nmain = (a.K >> 9) << 2;                                        // ... of which the whole 16-step groups (MOE: unused, none)
    const size_t tile_bytes = (size_t)16 * a.K;

    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)W, 0, (int)((size_t)a.N * a.K), 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x8, 0, (int)((size_t)(MOE != 0 ? a.x_rows : ((a.M + 15) & ~15)) * a.K), 0x00020000);

    // ---- staging.  Slice image: W tile f at 2 f KB, x tile g at 2 (NTILES + g) KB.  Wave w copies W tiles w + 8 i and x tiles w + 8 i; a
    // wave without an i-th tile loads zeros into its spare KB so that every wave has the same count in flight
    unsigned wbase[NLW], xbase[NLX];
#pragma unroll
    for (int i = 0; i < NLW; ++i) {
        const int f = wave + TG_WAVES * i;
        bool in_n;
        const int n16 = tile_src_ntile<MOE, WN, NTILES>(f, n_blk, a.N, in_n);
        wbase[i] = (f < NTILES && in_n) ? (unsigned)(n16 * tile_bytes + lane * 16) : TG_OOB;
    }
#pragma unroll
    for (int i = 0; i < NLX; ++i) {
        const int g = wave + TG_WAVES * i, m16 = (m0 >> 4) + g;
        xbase[i] = (g < MTILES && m16 * 16 < a.M) ? (unsigned)(m16 * tile_bytes + lane * 16) : TG_OOB;      // 16-row tiles with a live row
        if constexpr (MOE != 0) {                                             // per-lane source row: lane (c, q) fetches bytes [32 q, + 32) of its chunk
            int src = g < MTILES ? m0 + g * 16 + c : -1;
            if constexpr (MOE == MOE_GU_FUSED)
                if (src >= 0) src = a.row_token[src];                         // the gather; < 0: a padding row
            xbase[i] = (src >= 0 && src < a.x_rows) ? (unsigned)((size_t)src * a.K + 32 * q) : TG_OOB;
        }
    }
    // the second 1-KB piece of a chunk lies `second` bytes behind the first in the source: 1 KB in a fragment layout, 16 B in a token-major row
    auto copy_chunk = [&](const __amdgpu_buffer_rsrc_t& r, unsigned base, bool live, bool mine, uint8_t* img, unsigned second = 1024u) {
        const unsigned off = (live && base != TG_OOB) ? base : TG_OOB;
        uint8_t* d0 = mine ? img : lds + NBUF * SLICE + wave * 1024;
        uint8_t* d1 = mine ? img + 1024 : d0;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_t*)d0, 16, off, 0, 0, 0);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_void_t*)d1, 16, off == TG_OOB ? TG_OOB : off + second, 0, 0, 0);
    };
    auto stage = [&](int slice, int buf) {                // slices are staged in order, one call each; past the last one: zeros
        const bool live = slice < nsteps;
        uint8_t* img = lds + buf * SLICE;
#pragma unroll
        for (int i = 0; i < NLW; ++i) {
            const int f = wave + TG_WAVES * i;
            copy_chunk(rw, wbase[i] + (unsigned)slice * 2048u, live && wbase[i] != TG_OOB, f < NTILES, img + f * 2048);
        }
#pragma unroll
        for (int i = 0; i < NLX; ++i) {
            const int g = wave + TG_WAVES * i;
            if constexpr (MOE != 0) copy_chunk(rx, xbase[i] + (unsigned)slice * 128u, live && xbase[i] != TG_OOB, g < MTILES, img + (NTILES + g) * 2048, 16u);
            else copy_chunk(rx, xbase[i] + (unsigned)slice * 2048u, live && xbase[i] != TG_OOB, g < MTILES, img + (NTILES + g) * 2048);
        }
    };

    f32x4 acc[WN][WM];
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
        for (int i = 0; i < WM; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // one slice: the wave's WM x fragments stay in registers, its W fragments stream past them one ahead of the MFMAs that use them (the
    // scheduling fences keep hipcc from reading all WN fragments first: 8 VGPRs each beside WN * WM * 4 accumulators)
    auto mma_slice = [&](const uint8_t* img, auto main) {
        constexpr bool MAIN = decltype(main)::value;
        constexpr bool XMAIN = MOE != 0 || MAIN, WMAIN = MOE == 0 && MAIN;   // MOE: x images of two 16-B pieces against W remainder chunks
        i32x8 xf[WM];
#pragma unroll
        for (int i = 0; i < WM; ++i) xf[i] = f8_frag<XMAIN>(img + (NTILES + wm * WM + i) * 2048, lane);
        i32x8 wf = f8_frag<WMAIN>(img + (wn * WN) * 2048, lane);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < WN; ++j) {
            i32x8 wnext = wf;
            if (j + 1 < WN) wnext = f8_frag<WMAIN>(img + (wn * WN + j + 1) * 2048, lane);
#pragma unroll
            for (int i = 0; i < WM; ++i) acc[j][i] = f8_mfma(wf, xf[i], acc[j][i]);
            __builtin_amdgcn_sched_barrier(0);
            wf = wnext;
        }
        __builtin_amdgcn_s_setprio(0);
    };

    // ---- main loop: one barrier per slice.  Behind it slice t is visible to every wave and every wave is done with slice t - 1, whose buffer
    // the staging of slice t + NBUF - 1 overwrites at once.  The chunks of the whole 16-step groups first, then those of the K % 512 remainder
    int buf = 0, sbuf = NBUF - 1;
#pragma unroll
    for (int s = 0; s < NBUF - 1; ++s) stage(s, s);
    auto run = [&](int t0, int t1, auto main) {
        for (int t = t0; t < t1; ++t) {
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"((NBUF - 2) * G::LOADS) : "memory");
            stage(t + NBUF - 1, sbuf);
            mma_slice(lds + buf * SLICE, main);
            buf = buf + 1 == NBUF ? 0 : buf + 1;
            sbuf = sbuf + 1 == NBUF ? 0 : sbuf + 1;
        }
    };
    if constexpr (MOE != 0) {
        run(0, nsteps, std::false_type{});
    } else {
        run(0, nmain, std::true_type{});
        run(nmain, nsteps, std::false_type{});
    }
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the ring is dead: its tail loads (zeros) landed

    // ---- y = (acc * s_x[m]) * s_w[n]: the lane's m per m-tile, the register's n per n-tile.  Rows past M and columns past N are not stored
    // (MOE: s_x belongs to the SOURCE row -- the token of a gathered row; s_w to the row of W that n-tile j of the wave is: tile_src_ntile)
    const int mw0 = m0 + wm * WM * 16, nw0 = MOE == MOE_GU_FUSED ? n_blk * (G::BN / 2) + wn * (WN / 2) * 16 : n0 + wn * WN * 16;
    float sx[WM];
#pragma unroll
    for (int i = 0; i < WM; ++i) {
        int m = mw0 + i * 16 + c;
        if constexpr (MOE == MOE_GU_FUSED) m = a.row_token[m];
        sx[i] = (m >= 0 && m < (MOE != 0 ? a.x_rows : a.M)) ? a.xs[m] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        bool in_n;
        const int n = tile_src_ntile<MOE, WN, NTILES>(wn * WN + j, n_blk, a.N, in_n) * 16 + 4 * q;
        const f32x4 sw = in_n ? *reinterpret_cast<const f32x4*>(ws + n) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j][i][e] = (acc[j][i][e] * sx[i]) * sw[e];
    }
    TileArgs ta{};
    ta.out = a.out; ta.ldo = a.ldo; ta.M = a.M; ta.N = a.N; ta.row_weight = a.row_weight;
    if constexpr (MOE != 0) tile_moe_finish<MOE>(ta, acc, lds, wave, lane, mw0, nw0);
    else tile_epilogue<WN, WM, GU8, true>(ta, acc, lds, wave, lane, mw0, nw0);
}

template <int WAVES_N, int WN, int WM, bool GU8, int MOE = 0>
static int launch_f8(const F8Args& a, hipStream_t st) {
    return tile_launch_geom<gemm_tile_f8_kernel<WAVES_N, WN, WM, GU8, MOE>, F8Geom<WAVES_N, WN, WM>>(
        a, st, MOE ? "omni_moe_prefill_experts_fp8" : "omni_gemm_tile_fp8");
}

// the instantiation a TileChoice (gemm_tile_policy.h) names
template <bool GU8>
static int launch_choice_f8(const TileChoice& t, const F8Args& a, hipStream_t st) {
    switch (t.waves_n * 100 + t.wn * 10 + t.wm) {
    case 422: return launch_f8<4, 2, 2, GU8>(a, st);
    case 284: return launch_f8<2, 8, 4, GU8>(a, st);
    case 447: return launch_f8<4, 4, 7, GU8>(a, st);
    case 446: return launch_f8<4, 4, 6, GU8>(a, st);
    }
    omni_set_error("omni_gemm_tile_fp8: no kernel for tile <%d, %d, %d>", t.waves_n, t.wn, t.wm);
    return OMNI_EINVAL;
}

extern "C" int omni_gemm_tile_fp8(const omni_tile_gemm_fp8* g, void* stream) {
    OMNI_CHECK_ARG(g && g->x8 && g->x_scale && g->w8 && g->w_scale && g->out, "omni_gemm_tile_fp8: null argument");
    OMNI_CHECK_ARG(g->M >= 1 && g->N > 0 && g->N % 16 == 0 && g->K > 0 && g->K % 128 == 0, "omni_gemm_tile_fp8: M=%d N=%d K=%d (M >= 1, N %% 16, K %% 128)",
                   g->M, g->N, g->K);
    OMNI_CHECK_ARG((int64_t)g->N * g->K < (int64_t)TG_OOB && (int64_t)(g->M + 15) * g->K < (int64_t)TG_OOB, "omni_gemm_tile_fp8: an operand exceeds the 2 GB descriptor");
    const bool gu8 = g->act == OMNI_TILE_ACT_SILU_MUL_GU8;
    OMNI_CHECK_ARG(g->act == OMNI_TILE_ACT_NONE || gu8, "omni_gemm_tile_fp8: act=%d (none or SiLU-mul on the GU8 row order)", g->act);
    OMNI_CHECK_ARG(g->ldo >= (gu8 ? g->N / 2 : g->N) && g->ldo % 8 == 0, "omni_gemm_tile_fp8: ldo=%d (>= output width, multiple of 8)", g->ldo);
    OMNI_CHECK_ARG(g->tile_hint >= 0 && g->tile_hint <= 4, "omni_gemm_tile_fp8: tile_hint=%d", g->tile_hint);
    OMNI_CHECK_ARG(g->tile_hint == 0 || g->tile_hint == 2 || g->N % 256 == 0, "omni_gemm_tile_fp8: tile_hint=%d needs N %% 256 == 0", g->tile_hint);
    F8Args a{};
    a.x8 = (const uint8_t*)g->x8; a.xs = g->x_scale; a.W = (const uint8_t*)g->w8; a.ws = g->w_scale;
    a.out = (uint16_t*)g->out; a.ldo = g->ldo; a.M = g->M; a.N = g->N; a.K = g->K;
    const TileChoice t = tile_choice_fp8(g->M, g->N, g->tile_hint);
    return gu8 ? launch_choice_f8<true>(t, a, (hipStream_t)stream) : launch_choice_f8<false>(t, a, (hipStream_t)stream);
}

// ---- the MoE prefill's expert GEMMs on fp8 weights over the compact batch (entry point: moe_prefill.hip), in the two block heights of
// TILE_MOE_BLOCK (tile_epi.cuh), the same k order in both.
int k_moe_tile_gemm_f8(int mode, int block, const void* x8, const float* x_scale, int x_rows, const void* w8, const float* w_scale, int experts,
                       const int32_t* block_expert, const int32_t* row_token, const void* row_weight, void* out, int ldo, int rows, int N, int K,
                       void* stream) {
    OMNI_CHECK_ARG(x8 && x_scale && w8 && w_scale && block_expert && out && (mode == MOE_DOWN ? row_weight != nullptr : row_token != nullptr),
                   "omni_moe_prefill_experts_fp8: null argument");
    OMNI_CHECK_ARG(mode == MOE_GU_FUSED || mode == MOE_DOWN, "omni_moe_prefill_experts_fp8: mode=%d", mode);
    OMNI_CHECK_ARG((block == 64 || block == 256) && rows > 0 && rows % block == 0, "omni_moe_prefill_experts_fp8: block=%d rows=%d", block, rows);
    OMNI_CHECK_ARG(N > 0 && N % 128 == 0 && (mode != MOE_GU_FUSED || N % 256 == 0) && K > 0 && K % 128 == 0 && ldo % 8 == 0 && experts >= 1,
                   "omni_moe_prefill_experts_fp8: N=%d K=%d ldo=%d", N, K, ldo);
    OMNI_CHECK_ARG(x_rows > 0 && (int64_t)x_rows * K < (int64_t)TG_OOB && (int64_t)N * K < (int64_t)TG_OOB, "omni_moe_prefill_experts_fp8: an operand exceeds the 2 GB descriptor");
    OMNI_CHECK_ARG(mode != MOE_DOWN || x_rows >= rows, "omni_moe_prefill_experts_fp8: act rows");
    F8Args a{};
    a.x8 = (const uint8_t*)x8; a.xs = x_scale; a.x_rows = x_rows; a.W = (const uint8_t*)w8; a.ws = w_scale;
    a.out = (uint16_t*)out; a.ldo = ldo; a.M = rows; a.N = N; a.K = K;
    a.block_expert = block_expert; a.row_token = row_token; a.row_weight = (const uint16_t*)row_weight;
    hipStream_t st = (hipStream_t)stream;
    if (mode == MOE_GU_FUSED) return TILE_MOE_BLOCK(block, launch_f8, MOE_GU_FUSED, a, st);
    return TILE_MOE_BLOCK(block, launch_f8, MOE_DOWN, a, st);
}
