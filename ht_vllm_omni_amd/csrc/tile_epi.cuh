// What the tile GEMMs share: gemm_tile_kernel / gemm_tile_pp_kernel (gemm_prefill.hip, bf16 operands) and gemm_tile_f8_kernel
// (gemm_prefill_f8.hip, fp8 operands).  All of them end with D[n][m] accumulator fragments of v_mfma_*_16x16x*.  Here, once each:
//   TileArgs, tile_launch                 the launch arguments and "set the LDS attribute once, launch, check";
//   TileGeomT (TileGeom / F8Geom)         waves x tiles -> block, slice, ring and LDS sizes, pinned per instantiated geometry;
//   tile_block / tile_band                the order in which workgroups take output tiles;
//   tile_src_ntile                        which 16 rows of W an n-tile of the block is (the MoE fused gate_up pairing);
//   tile_moe_finish                       the MoE prefill's two finishes (SiLU(gate) * up; bf16(acc) * routing weight);
//   tile_epilogue                         the transposed store through LDS with the GU8 SiLU * up pairing.
// What differs for real between the operand widths -- staging, rings, counted waits, MFMA loops -- stays in the two .hip files; which
// geometry a launch takes is host arithmetic in gemm_tile_policy.h.
#pragma once
#include "common.cuh"
#include "gemm_frag.cuh"
#include "kernels.h"

#define TG_WAVES 8
#define TG_THREADS (TG_WAVES * 64)
#define TG_OOB 0x80000000u           // byte offset beyond any descriptor (num_records < 2^31): reads as zero
#define TG_LDS_MAX (160 * 1024)

typedef __attribute__((address_space(3))) void lds_void_t;

struct TileArgs {
    const uint16_t* x; int64_t x_rows; int ldx;
    int seg_len, seg_rows, row_off;
    const uint16_t* W; const float* bias; const float* scale;
    const float* resid; int ldr;
    float* out_f32; int ldf;
    uint16_t* out; int ldo;
    uint16_t* out2; int ldo2; const float* snake_alpha; const float* snake_inv_beta;
    int M, N, K;
    int act;                         // OMNI_TILE_ACT_*
    int mblocks, nblocks, band;
    // grouped (batched) launch: blockIdx.y = group; group g reads x rows [g * gx_rows, + its row count), the matrix
    // W + g * gw_elems, and writes output rows from g * gout_rows.  group_rows (device, optional) = live rows per group:
    // tiles past it leave at once, rows past it read as zero and are not stored
    long long gx_rows, gw_elems, gout_rows;
    const int32_t* group_rows;
    // MoE prefill over the expert-sorted compact batch (moe_prefill.hip, MOE != 0 instantiations): m block b belongs to expert
    // block_expert[b] (< 0: no rows, the workgroup leaves) and reads W + expert * gw_elems; batch row r is token row row_token[r] of x
    // (< 0: a padding row, reads as zero) and carries the routing weight row_weight[r] (bf16)
    const int32_t* block_expert; const int32_t* row_token; const uint16_t* row_weight;
};

// Geometry of one instantiation: 8 waves (two per SIMD: while one issues its LDS-DMA pieces -- 60 - 180 cycles each -- or waits for
// fragments, the other feeds the matrix pipe) as WAVES_N x (8 / WAVES_N); a wave owns WN n-tiles x WM m-tiles of 16 x 16 (acc = WN * WM * 4
// of its 256 registers); BN = WAVES_N * WN * 16, BM = (8 / WAVES_N) * WM * 16.  A slice holds one CHUNK (bytes of a 16-row tile per MFMA
// depth: 1 KB = 32 k of bf16, 2 KB = 128 k of fp8) of every tile of both operands, staged by DMA LDS-DMA instructions per chunk.
template <int CHUNK, int DMA, int WAVES_N, int WN, int WM>
struct TileGeomT {
    static constexpr int WAVES_M = TG_WAVES / WAVES_N;
    static constexpr int NTILES = WAVES_N * WN, MTILES = WAVES_M * WM;
    static constexpr int BN = NTILES * 16, BM = MTILES * 16;
    static constexpr int SLICE = (NTILES + MTILES) * CHUNK;
    static constexpr int NLW = (NTILES + TG_WAVES - 1) / TG_WAVES, NLX = (MTILES + TG_WAVES - 1) / TG_WAVES;   // chunks per wave and slice
    static constexpr int LOADS = DMA * (NLW + NLX);                          // LDS-DMA instructions per wave and slice (uniform: counted waits)
    static constexpr bool W_RAGGED = NTILES % TG_WAVES != 0;                 // some waves issue a dummy W load into a spare KB (uniform counts)
    static constexpr bool X_RAGGED = MTILES % TG_WAVES != 0;                 // likewise for x
    static constexpr int SPARE = W_RAGGED || X_RAGGED ? TG_WAVES * 1024 : 0;
    static constexpr int FLOOR = (TG_LDS_MAX - SPARE) / SLICE;               // slices that fit
    static constexpr int NBUF = FLOOR >= 4 ? 4 : FLOOR;                      // the ring: min(4, floor), at least 2
    static constexpr int EPI_BYTES = TG_WAVES * 16 * (WN * 64 + 16);         // fp32 image of one m-tile x the wave's columns
    static constexpr int RING_BYTES = NBUF * SLICE + SPARE;
    static constexpr int LDS_BYTES = RING_BYTES > EPI_BYTES ? RING_BYTES : EPI_BYTES;
    static_assert(WN % 2 == 0 && NBUF >= 2 && (NBUF - 2) * LOADS < 64 && LDS_BYTES <= TG_LDS_MAX, "geometry");
};
template <int WAVES_N, int WN, int WM> using TileGeom = TileGeomT<1024, 1, WAVES_N, WN, WM>;      // bf16: gemm_tile_kernel
template <int WAVES_N, int WN, int WM> using F8Geom = TileGeomT<2048, 2, WAVES_N, WN, WM>;        // fp8: gemm_tile_f8_kernel
// Every instantiated geometry, pinned to the figures of the two structs this template replaced: a ring that outgrows them is an LDS
// overrun, a load count that drifts is a counted wait that lets a slice be read before it landed.  (SLICE, NBUF, LOADS, LDS_BYTES)
#define TG_PIN(GEOM, A, B, C, slice, nbuf, loads, lds)                                                                                 \
    static_assert(GEOM<A, B, C>::SLICE == slice && GEOM<A, B, C>::NBUF == nbuf && GEOM<A, B, C>::LOADS == loads && GEOM<A, B, C>::LDS_BYTES == lds, \
                  "tile geometry moved: " #GEOM "<" #A ", " #B ", " #C ">")
TG_PIN(TileGeom, 2, 8, 4, 32768, 4, 4, 131072);
TG_PIN(TileGeom, 4, 4, 7, 30720, 4, 4, 131072);
TG_PIN(TileGeom, 4, 4, 6, 28672, 4, 4, 122880);
TG_PIN(TileGeom, 4, 2, 2, 12288, 4, 2, 57344);
TG_PIN(TileGeom, 1, 8, 4, 40960, 4, 5, 163840);
TG_PIN(TileGeom, 2, 6, 4, 28672, 4, 4, 122880);
TG_PIN(TileGeom, 1, 6, 4, 38912, 4, 5, 163840);
TG_PIN(F8Geom, 2, 8, 4, 65536, 2, 8, 131072);
TG_PIN(F8Geom, 4, 4, 7, 61440, 2, 8, 131072);
TG_PIN(F8Geom, 4, 4, 6, 57344, 2, 8, 122880);
TG_PIN(F8Geom, 4, 2, 2, 24576, 4, 4, 106496);
#undef TG_PIN

// The (n block, m block) of this workgroup.  XCD-aware tile order (bijective for any grid size): the hardware deals workgroup ids
// round-robin over the 8 XCDs, so id -> a contiguous chunk of the tile order per XCD.  Tile order: bands of `band` m blocks, n-major inside
// a band, so that an XCD's contiguous chunk of ~nwg / 8 tiles is a compact 2-D block (~sqrt x sqrt) of the tile grid: it touches the
// fewest distinct W and x panels (L2 misses go to the MALL / HBM)
__device__ __forceinline__ void tile_block(int band, int mblocks, int nblocks, int& n_blk, int& m_blk) {
    const int nwg = gridDim.x, id = blockIdx.x;
    const int xcd = id & 7, slot = id >> 3, per = nwg >> 3, rem = nwg & 7;
    const int tile = (xcd < rem ? xcd * (per + 1) : rem * (per + 1) + (xcd - rem) * per) + slot;
    const int per_band = band * nblocks;
    const int b = tile / per_band, r = tile - b * per_band;
    const int h = min(band, mblocks - b * band);                  // rows of this (possibly last, shorter) band
    n_blk = r / h;
    m_blk = b * band + (r - n_blk * h);
}

// the band rule: ~sqrt(tiles per XCD) m blocks
static inline int tile_band(int mblocks, int nblocks) {
    const int per_xcd = (mblocks * nblocks + 7) / 8;
    int band = 1;
    while (band * band < per_xcd) ++band;
    return band > mblocks ? mblocks : band;
}

// One launch of tile kernel KERNEL (Args = TileArgs | F8Args): the dynamic-LDS attribute once per kernel, the launch, its check.
template <auto KERNEL, typename Args>
static int tile_launch(dim3 grid, int lds_bytes, const Args& a, hipStream_t st, const char* name) {
    static bool attr_set = false;
    if (!attr_set) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) { omni_set_error("%s: LDS attribute: %s", name, hipGetErrorString(e)); return OMNI_EHIP; }
        attr_set = true;
    }
    hipLaunchKernelGGL(KERNEL, grid, dim3(TG_THREADS), lds_bytes, st, a);
    OMNI_CHECK_LAUNCH(name);
    return OMNI_OK;
}

// ... of a lock-step kernel of geometry G over a.M rows x a.N rows of W (the MoE fused gate_up: N / 2 output columns in blocks of BN / 2,
// which divide them -- the same count), `groups` of them along grid.y
template <auto KERNEL, typename G, typename Args>
static int tile_launch_geom(Args a, hipStream_t st, const char* name, int groups = 1) {
    a.mblocks = (a.M + G::BM - 1) / G::BM;
    a.nblocks = (a.N + G::BN - 1) / G::BN;
    a.band = tile_band(a.mblocks, a.nblocks);
    return tile_launch<KERNEL>(dim3(a.mblocks * a.nblocks, groups), G::LDS_BYTES, a, st, name);
}

// The MoE prefill's two block heights, one m block = `block` rows of ONE expert: 64 rows = <4, 2, 2> (128 columns; fused: 64 gate + 64 up),
// 256 rows = <2, 8, 4> (256 columns; fused: 128 + 128).  LAUNCH<WAVES_N, WN, WM, GU8, MOE>(...) is the caller's launcher.
#define TILE_MOE_BLOCK(block, LAUNCH, MOE, ...) ((block) == 64 ? LAUNCH<4, 2, 2, false, MOE>(__VA_ARGS__) : LAUNCH<2, 8, 4, false, MOE>(__VA_ARGS__))

// Which 16 rows of W tile f of a workgroup's NTILES n-tiles is (f = wave column * WN + the wave's n-tile j), and whether it lies inside the
// N rows.  Plain: n block and tile in order.  MOE_GU_FUSED (W = [gate rows | up rows], N = 2 I): n block nb covers columns [nb BN/2, + BN/2)
// of gate AND of up, a wave's first WN / 2 n-tiles being gate and its second WN / 2 the SAME columns of up, so that gate and up of an output
// element meet in one lane.  W staging of both kernels and the fp8 kernel's row scales go through here.
template <int MOE, int WN, int NTILES>
__device__ __forceinline__ int tile_src_ntile(int f, int n_blk, int N, bool& in_n) {
    int n16 = n_blk * NTILES + f;
    in_n = n16 * 16 < N;
    if constexpr (MOE == MOE_GU_FUSED) {
        constexpr int HN = WN / 2;
        const int j = f % WN;
        const int col16 = n_blk * (NTILES / 2) + (f / WN) * HN + j % HN;      // 16-column tile of the [rows, I] output
        in_n = col16 * 32 < N;
        n16 = (j >= HN ? N >> 5 : 0) + col16;
    }
    return n16;
}

__device__ __forceinline__ float tg_gelu(float v) { return 0.5f * v * (1.0f + erff(v * 0.70710678118654752f)); }

__device__ __forceinline__ bool tile_plain(const TileArgs& a) {
    return !a.bias && !a.scale && a.act != OMNI_TILE_ACT_GELU && !a.resid && !a.out_f32 && !a.out2 && a.out;
}

// Epilogue of a tile kernel: `acc[j][i]` = this wave's WN n-tiles x WM m-tiles (D[n][m] fragments), first row mw0, first column nw0; `lds` is dead.
// PLAIN = no bias, scale, GELU, residual, fp32 or snake output (the talker prefill's four GEMMs): the same values (acc + 0 and * 1 change
// nothing) without ~20 wave-uniform branches per pass -- they, not the stores, were most of an 11 k-cycle epilogue (profiles/r05_gemm_pp_stamps.txt).
template <int WN, int WM, bool GU8, bool PLAIN>
__device__ __forceinline__ void tile_epilogue(const TileArgs& a, f32x4 (&acc)[WN][WM], uint8_t* lds, int wave, int lane, int mw0, int nw0) {
    const int c = lane & 15, q = lane >> 4;
    // ---- epilogue.  Register side: y = act(acc + bias) * scale in fp32, transposed through this wave's LDS image in fp32, ONE m-tile
    // (16 rows x the wave's WN * 16 columns) per pass.  Row side: 8 columns per lane, a row's lanes cover WN * 64 contiguous bytes
    // of an fp32 output (whole 128-byte lines); + fp32 residual (the pass's residual loads are issued before its image is written:
    // the epilogue of a residual GEMM is an HBM phase, not a chain of load -> add -> store round trips), then up to three stores of
    // the SAME fp32 value: fp32 (the residual stream), bf16 (the next GEMM's operand), bf16(snake(y)) (the next conv's operand).
    // (Two images per wave, pass p + 1's written before pass p's is read back, measured SLOWER: 5.9 k -> 8.5 k cycles per epilogue.)
    constexpr int IPITCH = WN * 64 + 16;                  // bytes per image row
    constexpr int PER_ROW = GU8 ? WN : WN * 2;            // lane items per image row: a [8 gate | 8 up] tile, or 8 columns
    constexpr int RIT = (16 * PER_ROW + 63) / 64;         // row-side iterations per pass
    uint8_t* img = lds + wave * (16 * IPITCH);
    f32x4 bq[WN], sq[WN];
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int n = nw0 + j * 16 + 4 * q;
        bq[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        sq[j] = f32x4{1.f, 1.f, 1.f, 1.f};
        if (!PLAIN && n < a.N) {
            if (a.bias) bq[j] = *reinterpret_cast<const f32x4*>(a.bias + n);
            if (a.scale) sq[j] = *reinterpret_cast<const f32x4*>(a.scale + n);
        }
    }
    const bool gelu = !PLAIN && a.act == OMNI_TILE_ACT_GELU;
    auto write_image = [&](const int pass) {
        if (PLAIN) {
#pragma unroll
            for (int j = 0; j < WN; ++j) *reinterpret_cast<f32x4*>(img + c * IPITCH + (j * 16 + 4 * q) * 4) = acc[j][pass];
        } else if (gelu) {
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = tg_gelu(acc[j][pass][e] + bq[j][e]) * sq[j][e];
                *reinterpret_cast<f32x4*>(img + c * IPITCH + (j * 16 + 4 * q) * 4) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < WN; ++j) {
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = (acc[j][pass][e] + bq[j][e]) * sq[j][e];
                *reinterpret_cast<f32x4*>(img + c * IPITCH + (j * 16 + 4 * q) * 4) = v;
            }
        }
    };
    f32x4 rv[RIT][2];
#pragma unroll
    for (int pass = 0; pass < WM; ++pass) {
        const int mp0 = mw0 + pass * 16;
        if (!PLAIN && !GU8 && a.resid) {
#pragma unroll
            for (int it = 0; it < RIT; ++it) {
                const int idx = lane + 64 * it;
                const int row = idx / PER_ROW, ch = idx - row * PER_ROW;
                const int m = mp0 + row, n = nw0 + ch * 8;
                rv[it][0] = rv[it][1] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (idx < 16 * PER_ROW && m < a.M && n < a.N) {
                    const float* rp = a.resid + (size_t)m * a.ldr + n;
                    rv[it][0] = *reinterpret_cast<const f32x4*>(rp);
                    rv[it][1] = *reinterpret_cast<const f32x4*>(rp + 4);
                }
            }
        }
        write_image(pass);
        __builtin_amdgcn_wave_barrier();
        if (GU8) {
            // tile j of a row = [8 gate | 8 up] -> 8 act columns at n / 2: bf16(bf16(SiLU(bf16 gate)) * bf16 up), the rounding points of
            // torch's F.silu(g) * u on bf16 tensors (omni_silu_mul, oracle silu_mul)
#pragma unroll
            for (int it = 0; it < RIT; ++it) {
                const int idx = lane + 64 * it;
                const int row = idx / PER_ROW, j = idx - row * PER_ROW;
                const int m = mp0 + row, n = nw0 + j * 16;
                if (idx >= 16 * PER_ROW || m >= a.M || n >= a.N) continue;
                const float* gp = reinterpret_cast<const float*>(img + row * IPITCH + j * 64);
                u32x4 o;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float g0 = bfround(gp[2 * e]), g1 = bfround(gp[2 * e + 1]);
                    const float u0 = bfround(gp[8 + 2 * e]), u1 = bfround(gp[8 + 2 * e + 1]);
                    const float s0 = bfround(g0 / (1.0f + expf(-g0))), s1 = bfround(g1 / (1.0f + expf(-g1)));   // torch: F.silu(bf16) is bf16
                    o[e] = pack_bf2(s0 * u0, s1 * u1);
                }
                *reinterpret_cast<u32x4*>(a.out + (size_t)m * a.ldo + (n >> 1)) = o;
            }
        } else {
#pragma unroll
            for (int it = 0; it < RIT; ++it) {
                const int idx = lane + 64 * it;
                const int row = idx / PER_ROW, ch = idx - row * PER_ROW;
                const int m = mp0 + row, n = nw0 + ch * 8;
                if (idx >= 16 * PER_ROW || m >= a.M || n >= a.N) continue;
                f32x4 y0 = *reinterpret_cast<const f32x4*>(img + row * IPITCH + ch * 32);
                f32x4 y1 = *reinterpret_cast<const f32x4*>(img + row * IPITCH + ch * 32 + 16);
                if (PLAIN) {
                    u32x4 o;
                    o[0] = pack_bf2(y0[0], y0[1]); o[1] = pack_bf2(y0[2], y0[3]);
                    o[2] = pack_bf2(y1[0], y1[1]); o[3] = pack_bf2(y1[2], y1[3]);
                    *reinterpret_cast<u32x4*>(a.out + (size_t)m * a.ldo + n) = o;
                    continue;
                }
                if (a.resid) {
                    y0 += rv[it][0];
                    y1 += rv[it][1];
                }
                if (a.out_f32) {
                    float* op = a.out_f32 + (size_t)m * a.ldf + n;
                    *reinterpret_cast<f32x4*>(op) = y0;
                    *reinterpret_cast<f32x4*>(op + 4) = y1;
                }
                if (a.out) {
                    u32x4 o;
                    o[0] = pack_bf2(y0[0], y0[1]); o[1] = pack_bf2(y0[2], y0[3]);
                    o[2] = pack_bf2(y1[0], y1[1]); o[3] = pack_bf2(y1[2], y1[3]);
                    *reinterpret_cast<u32x4*>(a.out + (size_t)m * a.ldo + n) = o;
                }
                if (a.out2) {
                    const f32x4 al0 = *reinterpret_cast<const f32x4*>(a.snake_alpha + n), al1 = *reinterpret_cast<const f32x4*>(a.snake_alpha + n + 4);
                    const f32x4 ib0 = *reinterpret_cast<const f32x4*>(a.snake_inv_beta + n), ib1 = *reinterpret_cast<const f32x4*>(a.snake_inv_beta + n + 4);
                    f32x4 z0, z1;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float s0 = __sinf(y0[e] * al0[e]), s1 = __sinf(y1[e] * al1[e]);
                        z0[e] = y0[e] + ib0[e] * s0 * s0;
                        z1[e] = y1[e] + ib1[e] * s1 * s1;
                    }
                    u32x4 o;
                    o[0] = pack_bf2(z0[0], z0[1]); o[1] = pack_bf2(z0[2], z0[3]);
                    o[2] = pack_bf2(z1[0], z1[1]); o[3] = pack_bf2(z1[2], z1[3]);
                    *reinterpret_cast<u32x4*>(a.out2 + (size_t)m * a.ldo2 + n) = o;
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

// The finishes of the MoE prefill's expert GEMMs (MOE = MOE_GU_FUSED | MOE_GU_PLAIN | MOE_DOWN, kernels.h) on this wave's accumulators, whose
// row 16 i + (lane & 15) of the block's rows from mw0 the lane holds; a.N = the rows of W, nw0 = the wave's first OUTPUT column.
//   MOE_GU_FUSED  n-tile j is gate and HN + j up of the same columns: act = bf16(bf16(SiLU(bf16 gate)) * bf16 up) (silu_mul_bf16) [rows, N / 2];
//   MOE_DOWN      the two rounding points of y = bf16(acc) followed by y * weight on bf16 tensors, weight = a.row_weight[row];
//   MOE_GU_PLAIN  the accumulators as they are.
template <int MOE, int WN, int WM>
__device__ __forceinline__ void tile_moe_finish(TileArgs a, f32x4 (&acc)[WN][WM], uint8_t* lds, int wave, int lane, int mw0, int nw0) {
    if constexpr (MOE == MOE_GU_FUSED) {
        constexpr int HN = WN / 2;
        f32x4 o[HN][WM];
#pragma unroll
        for (int j = 0; j < HN; ++j)
#pragma unroll
            for (int i = 0; i < WM; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) o[j][i][e] = silu_mul_bf16(acc[j][i][e], acc[HN + j][i][e]);
        a.N >>= 1;                                                            // the output's width
        tile_epilogue<HN, WM, false, true>(a, o, lds, wave, lane, mw0, nw0);
    } else {
        if constexpr (MOE == MOE_DOWN) {
#pragma unroll
            for (int i = 0; i < WM; ++i) {
                const float wgt = bf2f(a.row_weight[mw0 + i * 16 + (lane & 15)]);
#pragma unroll
                for (int j = 0; j < WN; ++j)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[j][i][e] = bfround(acc[j][i][e]) * wgt;
            }
        }
        tile_epilogue<WN, WM, false, true>(a, acc, lds, wave, lane, mw0, nw0);
    }
}
