// Tile policy of the skinny GEMM: which workgroup tile (NT 16-row n-tiles x MT 16-row m-tiles) and how many M splits a launch takes.
// Pure host arithmetic on (norm, epilogue, M, N, K) with no HIP dependency: gemm.hip and gemm_w8.hip both call it (the bf16 kernel's bits
// depend on the row tile only through SlabOrder, the W8 kernel's not at all -- its time does), the persistent chains are built for the tiles
// it gives at 64 rows, and tests/test_gemm_tile_policy.py holds it to a table on the CPU.
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
