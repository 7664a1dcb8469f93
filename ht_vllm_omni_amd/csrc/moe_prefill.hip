// Sparse-MoE MLP of the Qwen3-Omni talker over PROMPT rows (T from 1 to many thousands): expert grouping on the device, expert GEMMs on
// the tile kernel over a compact expert-sorted batch, combine -- no host read between the router and the block's output, so the prefill
// can be captured in a graph.  Arithmetic and rounding points = moe.hip (oracle/talker_oracle.py moe_block): per expert gate_up,
// SiLU * up, down, * routing weight, each rounded to bf16; per token a bf16 accumulation in ascending expert index; + the sigmoid-gated
// shared expert.
//
// Alignment (omni_moe_align).  The tile kernel wants every m block to belong to ONE expert, so expert e's rows start at a multiple of the
// block height and the batch has r_max = T k + E (block - 1) rows (rounded up) whatever the routing is: sizes never depend on data.
// The split is moe.hip's own scheme scaled up -- one workgroup per expert finds its slots itself by ballot over the routing list (<= 256 KB
// at 8 k tokens, L2-resident across the 128 workgroups), no atomics, positions decided by slot order alone:
//   launch A  wave w of workgroup e counts the slots of expert e in ITS contiguous segment of the list -> counts[e][w] (and marks the slots
//             of experts outside the window);
//   launch B  every workgroup rebuilds the prefix of the <= 256 padded expert counts in LDS (so no third launch and no grid-wide wait), then
//             wave w compacts its segment again from base = expert start + the counts of waves < w: rows in ascending slot (= token) order.
//             It also writes the padding rows of its last block, its blocks' owner, and a share of the rows / blocks past the last expert.
// Wave segments instead of a workgroup-wide scan: no barrier inside the loops, a wave keeps several loads in flight; the price is reading the
// list twice, from L2.
// Two launches because an expert's start needs every other expert's count.
//
// Expert GEMMs: the MOE instantiations of the tile kernels of gemm_prefill.hip (bf16 experts) and gemm_prefill_f8.hip (fp8 experts); what
// the two share -- the gate / up pairing, the finishes, the block heights -- is in tile_epi.cuh.  Combine: one workgroup per token reads its
// k rows of y through slot_row, 8 columns per thread.
#include "common.cuh"
#include "kernels.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

#define MA_WAVES 8
#define MA_THREADS (MA_WAVES * 64)
#define MP_MAXK 8
#define MP_MAXE 256

struct AlignArgs {
    const int32_t* idx; const uint16_t* wts;
    int n, top_k, e0, E_local, blk, r_max;
    int32_t* counts; int32_t* row_start; int32_t* block_expert; int32_t* row_token; uint16_t* row_weight; int32_t* slot_row;
};

// wave w scans slots [w * seg, (w + 1) * seg) of the list, seg a multiple of 64
__device__ __forceinline__ int align_seg(int n) { return (n + MA_THREADS - 1) / MA_THREADS * 64; }

__global__ __launch_bounds__(MA_THREADS) void moe_align_count_kernel(const AlignArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x, target = a.e0 + e;
    const int seg = align_seg(a.n), lo = wave * seg, hi = min(lo + seg, a.n);
    int cnt = 0;
    for (int base = lo; base < hi; base += 64) {                  // uniform trip count: the ballot sees the whole wave
        const int i = base + lane;
        const int v = i < hi ? a.idx[i] : 0;
        cnt += __builtin_popcountll(__ballot(i < hi && v == target));
        // a slot of an expert another rank holds has no owner workgroup here: workgroup (i mod E_local) marks it
        if (i < hi && (v < a.e0 || v >= a.e0 + a.E_local) && i % a.E_local == e) a.slot_row[i] = -1;
    }
    if (lane == 0) a.counts[e * MA_WAVES + wave] = cnt;
}

__global__ __launch_bounds__(MA_THREADS) void moe_align_place_kernel(const AlignArgs a) {
    __shared__ int s_pad[MP_MAXE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int e = blockIdx.x, target = a.e0 + e, blk = a.blk;
    for (int j = threadIdx.x; j < a.E_local; j += MA_THREADS) {
        int c = 0;
#pragma unroll
        for (int w = 0; w < MA_WAVES; ++w) c += a.counts[j * MA_WAVES + w];
        s_pad[j] = (c + blk - 1) / blk * blk;
    }
    __syncthreads();
    int start = 0, total = 0;
    for (int j = 0; j < a.E_local; ++j) {                         // LDS broadcast reads
        const int p = s_pad[j];
        if (j < e) start += p;
        total += p;
    }
    int wbase = 0, mine = 0;
#pragma unroll
    for (int w = 0; w < MA_WAVES; ++w) {
        const int c = a.counts[e * MA_WAVES + w];
        if (w < wave) wbase += c;
        mine += c;
    }
    const int seg = align_seg(a.n), lo = wave * seg, hi = min(lo + seg, a.n);
    int run = start + wbase;
    for (int base = lo; base < hi; base += 64) {
        const int i = base + lane;
        const bool m = i < hi && a.idx[i] == target;
        const uint64_t bal = __ballot(m);
        if (m) {
            const int r = run + __builtin_popcountll(bal & ((1ull << lane) - 1ull));
            a.row_token[r] = i / a.top_k;
            a.row_weight[r] = a.wts[i];
            a.slot_row[i] = r;
        }
        run += __builtin_popcountll(bal);
    }
    const int pad_end = start + s_pad[e];
    for (int r = start + mine + threadIdx.x; r < pad_end; r += MA_THREADS) { a.row_token[r] = -1; a.row_weight[r] = 0; }
    for (int b = start / blk + threadIdx.x; b < pad_end / blk; b += MA_THREADS) a.block_expert[b] = e;
    if (threadIdx.x == 0) a.row_start[e] = start;
    if (threadIdx.x == 0 && e == 0) a.row_start[a.E_local] = total;
    // rows and blocks past the last expert: dealt over the workgroups
    for (int r = total + e * MA_THREADS + threadIdx.x; r < a.r_max; r += a.E_local * MA_THREADS) { a.row_token[r] = -1; a.row_weight[r] = 0; }
    for (int b = total / blk + e * MA_THREADS + threadIdx.x; b < a.r_max / blk; b += a.E_local * MA_THREADS) a.block_expert[b] = -1;
}

// ---------------------------------------------------------------- combine: one workgroup per token, 8 columns per thread
// out[t] = sum over the token's experts in ascending expert index of y[slot_row] (bf16 round after every add; rows < 0 are zero)
//          + bf16(bf16(sigmoid(gate_logit[t])) * shared[t])
__global__ __launch_bounds__(128) void moe_prefill_combine_kernel(const uint16_t* __restrict__ y, const int32_t* __restrict__ topk_idx,
                                                                  const int32_t* __restrict__ slot_row, const uint16_t* __restrict__ shared,
                                                                  const uint16_t* __restrict__ gate_logit, int ld_gate,
                                                                  uint16_t* __restrict__ out, int top_k, int H) {
    const int t = blockIdx.x;
    __shared__ int s_row[MP_MAXK];
    if (threadIdx.x < MP_MAXK) s_row[threadIdx.x] = -1;
    __syncthreads();
    if (threadIdx.x < (unsigned)top_k) {                  // thread j: rank of expert j among the token's experts (moe_combine_kernel)
        const int mine = topk_idx[(size_t)t * top_k + threadIdx.x];
        int rank = 0;
        for (int j = 0; j < top_k; ++j) rank += topk_idx[(size_t)t * top_k + j] < mine ? 1 : 0;
        s_row[rank] = slot_row[(size_t)t * top_k + threadIdx.x];
    }
    __syncthreads();
    int rows[MP_MAXK];
#pragma unroll
    for (int k = 0; k < MP_MAXK; ++k) rows[k] = s_row[k];
    float gate = 0.f;
    if (shared) {
        const float lg = bf2f(gate_logit[(size_t)t * ld_gate]);
        gate = bfround(1.0f / (1.0f + expf(-lg)));
    }
    for (int h = threadIdx.x * 8; h < H; h += 128 * 8) {
        u32x4 yv[MP_MAXK];
#pragma unroll
        for (int k = 0; k < MP_MAXK; ++k)
            yv[k] = rows[k] >= 0 ? *reinterpret_cast<const u32x4*>(y + (size_t)rows[k] * H + h) : u32x4{0u, 0u, 0u, 0u};
        float lo[4] = {0.f, 0.f, 0.f, 0.f}, hi[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < MP_MAXK; ++k)
            if (rows[k] >= 0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { lo[j] = bfround(lo[j] + bf_lo(yv[k][j])); hi[j] = bfround(hi[j] + bf_hi(yv[k][j])); }
            }
        if (shared) {
            const u32x4 sv = *reinterpret_cast<const u32x4*>(shared + (size_t)t * H + h);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                lo[j] = bfround(lo[j] + bfround(gate * bf_lo(sv[j])));
                hi[j] = bfround(hi[j] + bfround(gate * bf_hi(sv[j])));
            }
        }
        u32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = pack_bf2(lo[j], hi[j]);
        *reinterpret_cast<u32x4*>(out + (size_t)t * H + h) = o;
    }
}

// ---------------------------------------------------------------- C entry points
static int64_t moe_r_max(int T, int top_k, int E_local, int block) {
    return ((int64_t)T * top_k + (int64_t)E_local * (block - 1) + block - 1) / block * block;
}

extern "C" int omni_moe_align(const omni_moe_align_args* g, void* stream) {
    OMNI_CHECK_ARG(g && g->topk_idx && g->topk_w && g->counts_ws && g->row_start && g->block_expert && g->row_token && g->row_weight && g->slot_row,
                   "omni_moe_align: null argument");
    OMNI_CHECK_ARG(g->T >= 1 && g->top_k >= 1 && g->top_k <= MP_MAXK && g->E_local >= 1 && g->E_local <= MP_MAXE && g->e0 >= 0,
                   "omni_moe_align: T=%d top_k=%d E_local=%d e0=%d (top_k <= %d, E_local <= %d)", g->T, g->top_k, g->E_local, g->e0, MP_MAXK, MP_MAXE);
    OMNI_CHECK_ARG(g->block == 64 || g->block == 256, "omni_moe_align: block=%d (64 | 256)", g->block);
    const int64_t need = moe_r_max(g->T, g->top_k, g->E_local, g->block);
    OMNI_CHECK_ARG(need < ((int64_t)1 << 30) && g->r_max == need, "omni_moe_align: r_max=%d, the maps of these sizes hold %lld rows", g->r_max, (long long)need);
    AlignArgs a;
    a.idx = g->topk_idx; a.wts = (const uint16_t*)g->topk_w;
    a.n = g->T * g->top_k; a.top_k = g->top_k; a.e0 = g->e0; a.E_local = g->E_local; a.blk = g->block; a.r_max = g->r_max;
    a.counts = g->counts_ws; a.row_start = g->row_start; a.block_expert = g->block_expert; a.row_token = g->row_token;
    a.row_weight = (uint16_t*)g->row_weight; a.slot_row = g->slot_row;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(moe_align_count_kernel, dim3(g->E_local), dim3(MA_THREADS), 0, st, a);
    OMNI_CHECK_LAUNCH("omni_moe_align(count)");
    hipLaunchKernelGGL(moe_align_place_kernel, dim3(g->E_local), dim3(MA_THREADS), 0, st, a);
    OMNI_CHECK_LAUNCH("omni_moe_align(place)");
    return OMNI_OK;
}

// What the two entry points have in common (G = omni_moe_prefill_args | omni_moe_prefill_fp8_args): the checks on the fields both structs hold ...
template <typename G>
static int moe_prefill_check(const G* g, const char* name) {
    OMNI_CHECK_ARG(g && g->x && g->topk_idx && g->block_expert && g->row_token && g->row_weight && g->slot_row && g->w_gate_up && g->w_down &&
                   g->act_ws && g->y_ws && g->out, "%s: null argument", name);
    OMNI_CHECK_ARG(g->T >= 1 && g->top_k >= 1 && g->top_k <= MP_MAXK && g->E_local >= 1 && g->E_local <= MP_MAXE,
                   "%s: T=%d top_k=%d E_local=%d", name, g->T, g->top_k, g->E_local);
    OMNI_CHECK_ARG(g->block == 64 || g->block == 256, "%s: block=%d (64 | 256)", name, g->block);
    OMNI_CHECK_ARG(g->r_max == moe_r_max(g->T, g->top_k, g->E_local, g->block), "%s: r_max=%d does not belong to these sizes", name, g->r_max);
    OMNI_CHECK_ARG(!g->shared || (g->gate_logit && g->ld_gate >= 1), "%s: shared expert output without its gate logits", name);
    return OMNI_OK;
}

// ... and the combine behind the down GEMM
template <typename G>
static int launch_combine(const G* g, void* stream, const char* name) {
    hipLaunchKernelGGL(moe_prefill_combine_kernel, dim3(g->T), dim3(128), 0, (hipStream_t)stream, (const uint16_t*)g->y_ws, g->topk_idx,
                       g->slot_row, (const uint16_t*)g->shared, (const uint16_t*)g->gate_logit, g->ld_gate, (uint16_t*)g->out, g->top_k, g->H);
    OMNI_CHECK_LAUNCH(name);
    return OMNI_OK;
}

extern "C" int omni_moe_prefill_experts(const omni_moe_prefill_args* g, void* stream) {
    int rc = moe_prefill_check(g, "omni_moe_prefill_experts");
    if (rc != OMNI_OK) return rc;
    OMNI_CHECK_ARG(g->H > 0 && g->H % 64 == 0 && g->I > 0 && g->I % 32 == 0, "omni_moe_prefill_experts: H=%d I=%d (H %% 64, I %% 32)", g->H, g->I);
    const int H = g->H, I = g->I, R = g->r_max;
    const bool fused = k_moe_tile_fused_ok(g->block, I);
    OMNI_CHECK_ARG(fused || g->gu_ws, "omni_moe_prefill_experts: I=%d takes the unfused gate_up path, which needs gu_ws", I);
    if (fused) {
        rc = k_moe_tile_gemm(MOE_GU_FUSED, g->block, g->x, g->T, H, g->w_gate_up, (int64_t)2 * I * H, g->E_local, g->block_expert, g->row_token,
                             nullptr, g->act_ws, I, R, 2 * I, H, stream);
        if (rc != OMNI_OK) return rc;
    } else {
        rc = k_moe_tile_gemm(MOE_GU_PLAIN, g->block, g->x, g->T, H, g->w_gate_up, (int64_t)2 * I * H, g->E_local, g->block_expert, g->row_token,
                             nullptr, g->gu_ws, 2 * I, R, 2 * I, H, stream);
        if (rc != OMNI_OK) return rc;
        rc = omni_silu_mul(g->gu_ws, g->act_ws, R, I, stream);      // rows of blocks without an expert: never read again
        if (rc != OMNI_OK) return rc;
    }
    rc = k_moe_tile_gemm(MOE_DOWN, g->block, g->act_ws, R, I, g->w_down, (int64_t)H * I, g->E_local, g->block_expert, nullptr, g->row_weight,
                         g->y_ws, H, R, H, I, stream);
    if (rc != OMNI_OK) return rc;
    return launch_combine(g, stream, "omni_moe_prefill_experts(combine)");
}

// The same block on the decode step's fp8 expert bytes (gemm_prefill_f8.hip: the fp8 MFMA, W8A8): quantise the token rows once, gathered
// gate_up GEMM, quantise the act rows of the blocks an expert owns, down GEMM, the unchanged combine.  No host read.
extern "C" int omni_moe_prefill_experts_fp8(const omni_moe_prefill_fp8_args* g, void* stream) {
    int rc = moe_prefill_check(g, "omni_moe_prefill_experts_fp8");
    if (rc != OMNI_OK) return rc;
    OMNI_CHECK_ARG(g->s_gate_up && g->s_down && g->x8_ws && g->xs_ws && g->a8_ws && g->as_ws, "omni_moe_prefill_experts_fp8: null argument");
    OMNI_CHECK_ARG(g->H > 0 && g->H % 128 == 0 && g->I > 0 && g->I % 128 == 0, "omni_moe_prefill_experts_fp8: H=%d I=%d (H %% 128, I %% 128)", g->H, g->I);
    const int H = g->H, I = g->I, R = g->r_max;
    rc = k_quant_rows_f8_tok(g->x, H, g->x8_ws, g->xs_ws, g->T, H, nullptr, 1, stream);
    if (rc != OMNI_OK) return rc;
    rc = k_moe_tile_gemm_f8(MOE_GU_FUSED, g->block, g->x8_ws, g->xs_ws, g->T, g->w_gate_up, g->s_gate_up, g->E_local, g->block_expert, g->row_token,
                            nullptr, g->act_ws, I, R, 2 * I, H, stream);
    if (rc != OMNI_OK) return rc;
    rc = k_quant_rows_f8_tok(g->act_ws, I, g->a8_ws, g->as_ws, R, I, g->block_expert, g->block, stream);
    if (rc != OMNI_OK) return rc;
    rc = k_moe_tile_gemm_f8(MOE_DOWN, g->block, g->a8_ws, g->as_ws, R, g->w_down, g->s_down, g->E_local, g->block_expert, nullptr, g->row_weight,
                            g->y_ws, H, R, H, I, stream);
    if (rc != OMNI_OK) return rc;
    return launch_combine(g, stream, "omni_moe_prefill_experts_fp8(combine)");
}
