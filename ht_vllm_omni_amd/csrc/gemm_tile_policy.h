// Tile policies of the GEMMs, as pure host arithmetic with no HIP dependency, each held to a table on the CPU (tests/test_gemm_tile_policy.py,
// tests/test_gemm_tile_choice.py): a tile changes time, never bits (or bits in a way the kernels' own tests pin), so no GPU test sees it drift.
//   skinny_tile_*   the skinny (decode) GEMM: which workgroup tile (NT 16-row n-tiles x MT 16-row m-tiles) and how many M splits a launch takes,
//                   on (norm, epilogue, M, N, K).  gemm.hip and gemm_w8.hip both call it (the bf16 kernel's bits depend on the row tile only
//                   through SlabOrder, the W8 kernel's not at all -- its time does); the persistent chains are built for the tiles it gives
//                   at 64 rows.
//   tile_choice_*   the tile (prefill) GEMM: which geometry and kernel form omni_gemm_tile (gemm_prefill.hip) and omni_gemm_tile_fp8
//                   (gemm_prefill_f8.hip) run; at the end of this file.
//
// Plain GEMMs: narrow n groups (NT = 1, SiLU 16 + 16 columns), M split over grid.y until the grid has ~`wgs` workgroups.  Norm-fused
// (PRO_XNORM, and its deferred-rstd form): wide n groups (NT = 4) and as many M splits as that allows -- the normalisation work of a
// workgroup is proportional to the rows it owns, and is repeated once per n group.
#pragma once
#include "../../include/omni_talker.h"

// 1. NT, the n-tiles per workgroup
static inline int skinny_tile_nt(bool norm, int epi, int M, int N, int K) {
    const int mt_total = (M + 15) / 16;
    const bool gu8 = epi == OMNI_EPI_SILU_MUL_GU8;
    const bool silu = epi == OMNI_EPI_SILU_MUL || gu8;
    const int cols = silu ? N / 8 : N / 16;                   // n groups at the narrowest tile
    int nt = silu ? 2 : 1;
    if (norm) {
        // measured at M = 64 (scripts/bench_tiles.py): 64+ groups of NT = 4, else NT = 2
        nt = (cols % 4 == 0 && cols / 4 >= 64) ? 4 : ((cols % 2 == 0 && cols / 2 >= 32) ? 2 : nt);
        // 4096 columns over K >= 2048 (the backbone's qkv): 128 groups x 2 m-splits beat 64 x 4 (10.4 vs 10.8 us; the code
        // predictor's K = 1024 shape does not: same-box A/B of the step)
        // (33-48 rows -- three 16-row tiles -- take the 64-row choice too since round 5: 128 groups x 2 m-splits of 32 rows, the tile set of
        //  the persistent backbone launch, which now runs from 33 rows on: bb_chain.hip)
        if (!silu && nt == 4 && cols / 4 == 64 && K >= 2048 && mt_total >= 3) nt = 2;
        if (silu && nt < 2) nt = 2;
        if (gu8 && cols % 3 == 0 && cols / 3 >= 128) nt = 3;  // 256 workgroups (backbone), 128 x 2 m-splits (code predictor)
    } else if (silu && cols % 4 == 0 && cols / 4 >= 160 && mt_total == 4) {
        nt = 4;                                               // backbone gate_up at full batch: 32 + 32 columns, no M split
        if (gu8 && cols % 3 == 0 && cols / 3 >= 256) nt = 3;  // 24 columns x 256 workgroups: 14.8 vs 16.1 us
    }
    return nt;
}

// MT as the kernels exist (1, 2 or 4 m-tiles per workgroup) and the M splits (grid.y) that then cover M rows; a caller that overrides
// MT (gemm.hip's debug knob, gemm_w8.hip's register-budget clamp) comes back through here
static inline int skinny_tile_splits(int M, int* mt) {
    if (*mt == 3) *mt = 4;
    if (*mt > 4) *mt = 4;
    return ((M + 15) / 16 + *mt - 1) / *mt;
}

// 2. given NT and the workgroup target: MT and the M splits
static inline void skinny_tile_mt(bool norm, int epi, int M, int N, int nt, int wgs, int* mt_out, int* splits_out) {
    const int mt_total = (M + 15) / 16;
    const bool gu8 = epi == OMNI_EPI_SILU_MUL_GU8;
    const bool silu = epi == OMNI_EPI_SILU_MUL || gu8;
    const int groups = silu ? N / (8 * nt) : N / (16 * nt);
    int splits = groups >= 160 ? 1 : (wgs + groups - 1) / groups;
    // the 1024-wide gate_up (code predictor, 0.6B backbone: 128 groups of 24 columns) at 33-48 rows: three 16-row tiles, not a 32-row pair
    // with a half-empty partner (round 5) -- the tile set of the persistent chains there, whose fourth row group then has no work in ANY
    // stage and leaves at once instead of idling through four stages per layer to wake up for this one (B = 40: the predictor phase cost
    // 0.25 ms MORE than at 64 rows; cp_chain.hip k_cp_chain, bb_chain.hip)
    if (norm && gu8 && nt == 3 && groups == 128 && mt_total == 3) splits = 3;
    if (splits > mt_total) splits = mt_total;
    if (splits < 1) splits = 1;
    *mt_out = (mt_total + splits - 1) / splits;
    *splits_out = skinny_tile_splits(M, mt_out);
}

// ---- the tile GEMM.  A choice is a geometry <waves along n, n-tiles per wave, m-tiles per wave> of the lock-step kernel: 256 x 256 <2, 8, 4> |
// 256 x 224 <4, 4, 7> | 256 x 192 <4, 4, 6> | 192 x 256 <2, 6, 4> | 128 x 512 <1, 8, 4> | 96 x 512 <1, 6, 4> (columns x rows) and the small
// 128 x 64 <4, 2, 2>; or, mw != 0, the two-group form of the 256-column tile with 32 mw rows (gemm_tile_pp_kernel<MW>; bf16 only).  Every
// geometry adds k in the same order: the choice never changes a bit of the output.
struct TileChoice { int waves_n, wn, wm, mw; };
#define TILE_CUS 256              // workgroups of one round: one per CU (the ring takes most of the LDS)
#define TILE_FEW 96               // fewer big tiles than this leave most CUs idle: the K loop's latency is the cost, not MFMA throughput

static inline long long tile_count(int M, int N, int bm, int bn) { return (long long)((N + bn - 1) / bn) * ((M + bm - 1) / bm); }

// 256-column tiles come in three heights.  A grid runs in rounds of TILE_CUS tiles and a round costs ~ the tile's rows: 6.4 k prompt tokens
// x 2048 columns are 208 tiles of 256 rows (one round, 48 CUs idle) or 232 tiles of 224 rows (one round, 12.5 % shorter)
static inline int tile_rows_by_rounds(int M, int N) {
    long long best = -1;
    int bm = 256;
    for (int cand = 256; cand >= 192; cand -= 32) {           // ties go to the taller tile
        const long long cost = ((tile_count(M, N, cand, 256) + TILE_CUS - 1) / TILE_CUS) * (cand + 16);
        if (best < 0 || cost < best) { best = cost; bm = cand; }
    }
    return bm;
}

// rows of the 256-column tile: tile_hint 3 / 4 name 224 / 192, else by rounds where `by_rounds`, else 256
static inline int tile_rows_256(int M, int N, int hint, bool by_rounds) {
    if (hint == 3) return 224;
    if (hint == 4) return 192;
    return by_rounds ? tile_rows_by_rounds(M, N) : 256;
}

static inline TileChoice tile_lockstep_256(int bm) { return bm == 224 ? TileChoice{4, 4, 7, 0} : (bm == 192 ? TileChoice{4, 4, 6, 0} : TileChoice{2, 8, 4, 0}); }

// omni_gemm_tile.  `plain` = no conv window, no groups, no group_rows: what the two-group form takes (5 - 8 % faster at every height).
// tile_hint: 0 auto | 1 big lock-step | 2 small | 3 / 4 lock-step 224 / 192 rows | 5 / 6 / 7 two-group 256 / 224 / 192 rows.
static inline TileChoice tile_choice_bf16(int M, int N, int groups, bool plain, bool gu8, int hint) {
    // the small tile for problems whose big-tile grid would leave most CUs idle (the Code2Wav transformer / ConvNeXt at a few hundred frames,
    // streaming chunks); the big tile is the widest that divides N
    const int big_n = N % 256 == 0 ? 256 : (N % 192 == 0 ? 192 : (N % 128 == 0 ? 128 : (N % 96 == 0 ? 96 : (N > 128 ? 256 : 128))));
    const int big_m = big_n >= 192 ? 256 : 512;
    if (hint == 2 || (hint == 0 && tile_count(M, N, big_m, big_n) * groups < TILE_FEW && N >= 64)) return {4, 2, 2, 0};
    if (N % 256 == 0) {
        const int h = hint == 5 ? 1 : (hint > 5 ? hint - 3 : hint);       // 5 / 6 / 7 name the heights of 1 / 3 / 4
        const int bm = tile_rows_256(M, N, h, hint == 0 && groups == 1);
        if (hint >= 5 || (hint == 0 && plain)) return {4, 4, 0, bm / 32};
        return tile_lockstep_256(bm);
    }
    if (gu8) return {1, 8, 4, 0};
    if (N % 192 == 0) return {2, 6, 4, 0};
    if (N % 128 == 0) return {1, 8, 4, 0};
    if (N % 96 == 0) return {1, 6, 4, 0};
    return N > 128 ? TileChoice{2, 8, 4, 0} : TileChoice{1, 8, 4, 0};
}

// omni_gemm_tile_fp8.  The small tile where 256-column tiles do not divide N or would leave most CUs idle; tile_hint: 0 auto | 1 256 rows |
// 2 small | 3 / 4 224 / 192 rows.
static inline TileChoice tile_choice_fp8(int M, int N, int hint) {
    if (hint == 2 || N % 256 != 0 || (hint == 0 && tile_count(M, N, 256, 256) < TILE_FEW)) return {4, 2, 2, 0};
    return tile_lockstep_256(tile_rows_256(M, N, hint, hint == 0));
}
