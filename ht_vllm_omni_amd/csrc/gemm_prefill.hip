// Large-M bf16 GEMM on the matrix cores: out[M, N] = epilogue(x[M, K] . W[N, K]^T), fp32 accumulate.
//
// The prefill-side counterpart of gemm.hip's weight-streaming skinny kernel: at M = 512 ... 600 k rows the op is MFMA-bound, so a
// workgroup owns a 256-row x BN-column output tile, stages 64-deep slices of both operands in LDS and reuses every fragment
// 4 - 8 times from registers.  Built for two callers:
//   * talker prefill (engine.prefill_native): the four per-layer GEMMs on the SAME fragment-major weights the decode step
//     streams (OMNI_LAYOUT_W_FRAG; gate_up in its 8-row interleave with SiLU(gate) * up fused) -- weights are stored once;
//   * Code2Wav decoder (codec.hip / code2wav.py): activations are TIME-major [T, C], so a causal dilated conv1d is this GEMM
//     over overlapping row windows of x -- K = taps x C_in split into `seg_len`-wide segments, segment s of output row m
//     reading x row m + row_off + s * seg_rows -- with no im2col buffer, and a transposed conv of stride s / kernel 2s is
//     the GEMM [T, 2 C_in] x [2 C_in, s * C_out] whose row-major output IS the up-sampled [T * s, C_out] signal.
//
// Data movement.  Both operands reach LDS by LDS-DMA (buffer_load_dwordx4 ... lds, 1 KB per wave instruction, no VGPR
// staging): W fragments are contiguous 1 KB runs of the fragment-major matrix; x fragments are gathered by the per-lane
// SOURCE address (lane (c, q) fetches 16 B of row c at k-offset 8q), which leaves the LDS image fragment-major too --
// every ds_read_b128 is lane-linear, conflict-free, no swizzle.  Rows outside [0, x_rows) (the causal left padding, the
// M tail) and k-steps past K are out of range of the buffer descriptor and read as zero.  Two LDS buffers; the loads of
// slice t + 1 are issued before the MFMAs of slice t, one counted wait + barrier per slice.
// MFMA v_mfma_f32_16x16x32_bf16 with W as the A operand: D[n][m], lane holds m = l & 15, n = 4 (l >> 4) + reg.
// Epilogue: y = (acc + bias) -> GELU -> * scale (+ fp32 residual) in fp32, transposed through LDS (one m-tile per pass) so that global
// stores are whole row pieces; on the way out SiLU(gate) * up for the interleaved gate_up layout, and up to three stores of y: fp32 (a residual
// STREAM kept in fp32: snake's sin(alpha x) turns a bf16 ulp of x ~ 16 into a phase error of 0.1 rad), bf16 (the next GEMM's
// operand) and bf16(snake(y)) = y + inv_beta * sin^2(alpha * y) -- the activation in front of the NEXT conv, so that no
// stand-alone activation pass runs over the 24 kHz-rate tensors.
// Workgroups are dealt to the 8 XCDs in contiguous chunks of the (n block, m block) order, m fastest: the workgroups that
// share an L2 share a W panel.
// This file holds what is bf16's own: the staging, the ring and its counted waits, the two kernels' MFMA schedules, and the entry point's
// argument checks.  Shared with the fp8 sibling (gemm_prefill_f8.hip) and written once in tile_epi.cuh: geometry, tile order, launcher,
// the MoE gate / up pairing and finishes, the epilogue.  Which geometry and form a launch takes: tile_choice_bf16, gemm_tile_policy.h.
#include "common.cuh"
#include "gemm_frag.cuh"
#include "gemm_tile_policy.h"
#include "kernels.h"
#include "tile_epi.cuh"

__device__ __forceinline__ f32x4 tg_mfma(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// Geometry TileGeom<WAVES_N, WN, WM> (tile_epi.cuh): one slice = a 32-deep 1-KB chunk of every tile of both operands.
// MOE != 0: the same staging, ring and slice order over the MoE prefill's compact batch (one m block = BM rows of ONE expert):
//   MOE_GU_FUSED  x rows gathered through row_token; W = the decode step's [gate rows | up rows] matrix (a.N = 2 I rows) in the gate / up
//                 pairing of tile_src_ntile, SiLU(gate) * up in registers, out = act [rows, I];
//   MOE_GU_PLAIN  x gathered, plain [rows, 2 I] output (widths the fused arrangement does not divide; omni_silu_mul follows);
//   MOE_DOWN      x = act rows as they lie, out = bf16(bf16(acc) * row_weight[row]).
// (the mode numbers: kernels.h; the finishes: tile_moe_finish)
template <int WAVES_N, int WN, int WM, bool GU8, int MOE = 0>
__global__ __launch_bounds__(TG_THREADS) void gemm_tile_kernel(const TileArgs a_in) {
    using G = TileGeom<WAVES_N, WN, WM>;
    TileArgs a = a_in;
    long long x_lo = 0, x_hi = a.x_rows;                                      // rows of x this launch may read
    if (gridDim.y > 1 || a.group_rows) {
        const int grp = blockIdx.y;
        if (a.group_rows) a.M = min(a.M, a.group_rows[grp]);
        x_lo = grp * a.gx_rows;
        x_hi = min(x_lo + a.M, a.x_rows);
        a.W += (size_t)grp * a.gw_elems;
        const size_t orow = (size_t)grp * a.gout_rows;
        if (a.out) a.out += orow * a.ldo;
        if (a.out2) a.out2 += orow * a.ldo2;
        if (a.out_f32) a.out_f32 += orow * a.ldf;
        if (a.resid) a.resid += orow * a.ldr;
    }
    constexpr int NTILES = G::NTILES, SLICE = G::SLICE, NLW = G::NLW, NLX = G::NLX, NBUF = G::NBUF;
    constexpr int INFLIGHT = NBUF - 2;                                        // slices still landing when slice t + 1 is awaited
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int wn = wave % WAVES_N, wm = wave / WAVES_N;
    const int c = lane & 15, q = lane >> 4;

    int n_blk, m_blk;
    tile_block(a.band, a.mblocks, a.nblocks, n_blk, m_blk);               // XCD-aware, banded (tile_epi.cuh)
    const int m0 = m_blk * G::BM, n0 = n_blk * G::BN;
    if (m0 >= a.M) return;                                                    // a group with fewer rows than the launch's M (uniform)
    if constexpr (MOE != 0) {
        const int expert = a.block_expert[m_blk];                             // uniform: one expert per m block
        if (expert < 0) return;                                               // past the last expert's rows
        a.W += (size_t)expert * a.gw_elems;
    }
    const int nsteps = a.K >> 5;                                              // 32-deep slices

    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.W, 0, (int)((size_t)a.N * a.K * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)(a.x_rows * a.ldx * 2), 0x00020000);

    // ---- staging.  Slice image: W tile f at f KB, x tile g at (NTILES + g) KB.  Wave w issues W tiles w + 8 i (i < NLW; a wave
    // without an i-th tile loads zeros into a spare KB so that every wave has the same count in flight) and x tiles w + 8 i.
    unsigned wbase[NLW];
    int xrow[NLX], xbyte[NLX];
#pragma unroll
    for (int i = 0; i < NLW; ++i) {
        const int f = wave + TG_WAVES * i;
        bool in_n;
        const int n16 = tile_src_ntile<MOE, WN, NTILES>(f, n_blk, a.N, in_n);
        wbase[i] = (f < NTILES && in_n) ? (unsigned)((size_t)n16 * nsteps * 1024 + lane * 16) : TG_OOB;
    }
#pragma unroll
    for (int i = 0; i < NLX; ++i) {
        const int g = wave + TG_WAVES * i;
        xrow[i] = (int)x_lo + m0 + g * 16 + c + a.row_off;
        if constexpr (MOE == MOE_GU_FUSED || MOE == MOE_GU_PLAIN)             // the gather: the lane's source row is the batch row's token
            xrow[i] = g < G::MTILES ? a.row_token[m0 + g * 16 + c] : -1;
        xbyte[i] = (xrow[i] * a.ldx + 8 * q) * 2;        // wraps out of the descriptor for rows < 0 (never used then)
    }
    int seg = 0, cs = 0;                                  // segment walk of the NEXT slice to stage: k = seg * seg_len + cs
    const int seg_row_bytes = a.seg_rows * a.ldx * 2;
    auto stage = [&](int slice) {                         // slices are staged in order, one call each
        const int buf = slice % NBUF;
        const bool live = slice < nsteps;
        const int shift = seg * a.seg_rows, add = seg * seg_row_bytes + cs * 2;
        uint8_t* base = lds + buf * SLICE + wave * 1024;
#pragma unroll
        for (int i = 0; i < NLW; ++i) {
            const bool mine = !G::W_RAGGED || wave + TG_WAVES * i < NTILES;
            const unsigned off = (live && mine && wbase[i] != TG_OOB) ? wbase[i] + (unsigned)slice * 1024u : TG_OOB;
            uint8_t* dst = mine ? base + i * (TG_WAVES * 1024) : lds + NBUF * SLICE + wave * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (lds_void_t*)dst, 16, off, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < NLX; ++i) {
            const bool mine = !G::X_RAGGED || wave + TG_WAVES * i < G::MTILES;
            const int r = xrow[i] + shift;
            const unsigned off = (live && mine && r >= (int)x_lo && r < (int)x_hi) ? (unsigned)(xbyte[i] + add) : TG_OOB;
            uint8_t* dst = mine ? base + (NTILES + i * TG_WAVES) * 1024 : lds + NBUF * SLICE + wave * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (lds_void_t*)dst, 16, off, 0, 0, 0);
        }
        cs += 32;
        if (cs >= a.seg_len) { cs = 0; ++seg; }
    };

    f32x4 acc[WN][WM];
#pragma unroll
    for (int j = 0; j < WN; ++j)
#pragma unroll
        for (int i = 0; i < WM; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- main loop.  Per slice a wave reads WM x fragments + WN W fragments and issues WN * WM MFMAs, in two halves of the W
    // tiles.  The wait for slice t + 1 and the workgroup barrier sit BETWEEN the halves of slice t; right after it the wave
    // reads the x fragments and the first W half of slice t + 1 into the other register set, so that LDS latency hides behind
    // the second half's MFMAs, and the second W half is read at the top of the next slice behind the first half's MFMAs.
    // NBUF-deep ring, slice t + NBUF - 1 staged at the top of slice t: NBUF - 2 slices stay in flight across every barrier
    // (counted vmcnt, never 0 inside the loop).  lgkmcnt(0) before the barrier retires this wave's reads of the buffer that
    // the next top-of-slice staging overwrites.
    constexpr int HW = WN / 2;
    auto lds_w = [&](int slice, int j) {
        return *reinterpret_cast<const u32x4*>(lds + (slice % NBUF) * SLICE + (wn * WN + j) * 1024 + lane * 16);
    };
    auto lds_x = [&](int slice, int i) {
        return *reinterpret_cast<const u32x4*>(lds + (slice % NBUF) * SLICE + (NTILES + wm * WM + i) * 1024 + lane * 16);
    };
    u32x4 xa[WM], xb[WM], w0[HW], w1[HW];
#pragma unroll
    for (int s = 0; s < NBUF - 1; ++s) stage(s);
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(INFLIGHT * G::LOADS) : "memory");
#pragma unroll
    for (int i = 0; i < WM; ++i) xa[i] = lds_x(0, i);
#pragma unroll
    for (int j = 0; j < HW; ++j) w0[j] = lds_w(0, j);

#define TG_SLICE(T, XCUR, XNEXT)                                                                             \
    {                                                                                                        \
        _Pragma("unroll") for (int j = 0; j < HW; ++j) w1[j] = lds_w((T), HW + j);                           \
        stage((T) + NBUF - 1);                                                                               \
        __builtin_amdgcn_s_setprio(1);                                                                       \
        _Pragma("unroll") for (int j = 0; j < HW; ++j)                                                       \
            _Pragma("unroll") for (int i = 0; i < WM; ++i) acc[j][i] = tg_mfma(w0[j], XCUR[i], acc[j][i]);   \
        __builtin_amdgcn_s_setprio(0);                                                                       \
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(INFLIGHT * G::LOADS) : "memory"); \
        _Pragma("unroll") for (int i = 0; i < WM; ++i) XNEXT[i] = lds_x((T) + 1, i);                         \
        _Pragma("unroll") for (int j = 0; j < HW; ++j) w0[j] = lds_w((T) + 1, j);                            \
        __builtin_amdgcn_s_setprio(1);                                                                       \
        _Pragma("unroll") for (int j = 0; j < HW; ++j)                                                       \
            _Pragma("unroll") for (int i = 0; i < WM; ++i) acc[HW + j][i] = tg_mfma(w1[j], XCUR[i], acc[HW + j][i]); \
        __builtin_amdgcn_s_setprio(0);                                                                       \
    }
    for (int t = 0; t < nsteps; t += 2) {                // an odd slice count runs one slice of zeros (staged out of range)
        TG_SLICE(t, xa, xb)
        TG_SLICE(t + 1, xb, xa)
    }
#undef TG_SLICE
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");   // the ring is dead: its tail loads (zeros) landed

    if constexpr (MOE != 0) {
        const int nw0 = MOE == MOE_GU_FUSED ? n_blk * (G::BN / 2) + wn * (WN / 2) * 16 : n0 + wn * WN * 16;
        tile_moe_finish<MOE>(a, acc, lds, wave, lane, m0 + wm * WM * 16, nw0);
    } else {
        if (tile_plain(a)) tile_epilogue<WN, WM, GU8, true>(a, acc, lds, wave, lane, m0 + wm * WM * 16, n0 + wn * WN * 16);
        else tile_epilogue<WN, WM, GU8, false>(a, acc, lds, wave, lane, m0 + wm * WM * 16, n0 + wn * WN * 16);
    }
}

// ---- the two-group ("ping-pong") form of the 256-column tile.  Same images, same MFMA, same accumulation order as gemm_tile_kernel
// (bit-identical output); what differs is WHEN a wave does what.  The eight waves are two groups of four, one wave of each group per SIMD:
// group g owns the tile's m-tiles [MW g, + MW) (16 rows each; BM = 32 MW), wave column wc = wave & 3 owns n-tiles [4 wc, + 4).  A K-tile
// (64 deep: two 32-deep steps) is two phases of [12 LDS reads + 4 LDS-DMA pieces | barrier | 24 - 32 MFMAs | barrier], and group 1 runs ONE
// barrier interval behind group 0: while one wave of a SIMD issues its loads (an LDS-DMA piece costs its issuer 60 - 180 cycles) and waits
// for its fragments, the other one owns the matrix pipe.  In gemm_tile_kernel both waves of a SIMD load at the same time and then want the
// pipe at the same time.  Phase 2 t: [x low (t), W high (t) | x low (t) x all four n-tiles]; phase 2 t + 1: [x high (t), W low (t + 1) |
// x high (t) x all four] (the low W fragments live in two register sets).
// Staging: a K-tile's image is four 16 KB half-tiles (x: the low m-tiles of both groups | W: n-tiles 0-1 of every wave column | W: n-tiles
// 2-3 | x: the high m-tiles; a wave without a real piece loads zeros into a spare KB: uniform vmcnt), two 64 KB buffers.  Each phase stages
// the two half-tiles that the phase after the next one reads, and waits -- vmcnt(4) behind its own four pieces, in front of its first
// barrier -- for the two that the NEXT phase reads.  Order of a region's life: read in phase p (the reads retire at that wave's lgkmcnt(0)
// behind the phase's first barrier) -> re-staged in phase p + 2 -> waited for in p + 3 -> read in p + 4.  With the groups one interval
// apart every one of these edges still has a barrier that BOTH parties passed in between.
// Measured (scripts/probes/gemm_pp_stamps.hip, profiles/r05_gemm_pp_stamps.txt): 2 400 - 2 600 cycles per K-tile against 2 048 of MFMA at
// full rate (gemm_tile_kernel: ~2 900); four phases of 12 - 16 MFMAs: +1.5 %; the closing barrier 4 or 8 MFMAs before a section's end
// (both groups on the pipe for a moment): +9 %; unequal groups (240 / 208 rows): slower than the next taller equal pair.
//
// -DPP_STAMPS (the probe only): 1 / 2 = the shader clock at the section boundaries of K-tiles 8 ... 23 of one workgroup (first wave of each
// group; 2 adds a stamp between the loads and the first barrier), kept in LDS behind the ring (a global store would count in vmcnt);
// 3 = shader clock and the 100 MHz clock at kernel entry, loop start, loop end, kernel end, nothing inside the loop.
#ifdef PP_STAMPS
__device__ unsigned long long g_pp_stamps[2][1024];
__device__ int g_pp_stamp_wg;
#if PP_STAMPS == 3
#define PP_T()
#define PP_C(k) do { if (st_wave) { g_pp_stamps[grp][1 + 2 * (k)] = __builtin_amdgcn_s_memtime(); g_pp_stamps[grp][2 + 2 * (k)] = __builtin_amdgcn_s_memrealtime(); } } while (0)
#else
#define PP_T() do { if (st_on) { st_buf[st_n] = __builtin_amdgcn_s_memtime(); ++st_n; } } while (0)
#define PP_C(k)
#endif
#if PP_STAMPS == 2
#define PP_T1() PP_T()
#else
#define PP_T1()
#endif
#else
#define PP_T()
#define PP_T1()
#define PP_C(k)
#endif

template <int MW, bool GU8>
__global__ __launch_bounds__(TG_THREADS) void gemm_tile_pp_kernel(const TileArgs a_in) {
    const TileArgs& a = a_in;
    constexpr int KT_BYTES = 64 * 1024, HALF = 16 * 1024, SPARE = 2 * KT_BYTES;
    constexpr int LO = (MW + 1) / 2, HI = MW - LO;            // low / high m-tiles of a wave
    static_assert(MW >= 2 && MW <= 8, "geometry");
    extern __shared__ __attribute__((aligned(1024))) uint8_t lds[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int grp = wave >> 2, wc = wave & 3;
    const int c = lane & 15, q = lane >> 4;
#ifdef PP_STAMPS
    const bool st_wave = (int)blockIdx.x == g_pp_stamp_wg && wc == 0 && lane == 0;
#endif
    PP_C(0);
    int n_blk, m_blk;
    tile_block(a.band, a.mblocks, a.nblocks, n_blk, m_blk);
    const int m0 = m_blk * (32 * MW), n0 = n_blk * 256;
    const int nsteps = a.K >> 5, nkt = (nsteps + 1) >> 1;
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc((void*)a.W, 0, (int)((size_t)a.N * a.K * 2), 0x00020000);
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc((void*)a.x, 0, (int)(a.x_rows * a.ldx * 2), 0x00020000);

    // staging: piece e (0 / 1) of a half-tile = fragment f = wave + 8 e of its 16 = (slot t = f >> 1, k-step f & 1).  Slot t of an x half is
    // the t-th m-tile of [group 0's half | group 1's half]; slot t of a W half is n-tile 4 (t >> 1) + (t & 1) (+ 2 in the high half).
    unsigned wofs[2][2], xofs[2][2];
    bool xreal[2][2];
#pragma unroll
    for (int hi = 0; hi < 2; ++hi)
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int f = wave + 8 * e, t = f >> 1, ks = f & 1;
            const int n16 = (n0 >> 4) + 4 * (t >> 1) + (t & 1) + 2 * hi;
            wofs[hi][e] = n16 * 16 < a.N ? (unsigned)(((size_t)n16 * nsteps + ks) * 1024 + lane * 16) : TG_OOB;
            const int cnt = hi ? HI : LO;                     // per group
            const int mt = (t < cnt ? 0 : MW) + (hi ? LO : 0) + (t < cnt ? t : t - cnt);
            const int row = m0 + mt * 16 + c;
            xreal[hi][e] = t < 2 * cnt;
            xofs[hi][e] = (t < 2 * cnt && row < a.M && row < a.x_rows) ? (unsigned)(((size_t)row * a.ldx + ks * 32 + 8 * q) * 2) : TG_OOB;
        }
    auto stage = [&](int kt, int h, int buf) {                // h: 0 x low, 1 W low, 2 W high, 3 x high
        const bool live = kt < nkt;
        const bool is_w = h == 1 || h == 2;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const unsigned base = is_w ? wofs[h == 2][e] : xofs[h == 3][e];
            // an odd count of 32-deep steps: the last K-tile's second step lies past the row's K (x: the next row's data; W: the next n-tile's)
            const bool tail = ((wave + 8 * e) & 1) && 2 * kt + 1 >= nsteps;
            const unsigned off = (live && !tail && base != TG_OOB) ? base + (unsigned)kt * (is_w ? 2048u : 128u) : TG_OOB;
            const bool real = is_w || xreal[h == 3][e];
            uint8_t* dst = real ? lds + buf * KT_BYTES + h * HALF + (wave + 8 * e) * 1024 : lds + SPARE + wave * 1024;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(is_w ? rw : rx, (lds_void_t*)dst, 16, off, 0, 0, 0);
        }
    };
    const int t_lo = grp ? LO : 0, t_hi = grp ? HI : 0;       // this group's first slot in the x halves
    auto lds_x = [&](int buf, int hi, int i, int ks) {
        return *reinterpret_cast<const u32x4*>(lds + buf * KT_BYTES + (hi ? 3 : 0) * HALF + ((((hi ? t_hi : t_lo) + i) * 2 + ks) * 1024) + lane * 16);
    };
    auto lds_w = [&](int buf, int hi, int j, int ks) {
        return *reinterpret_cast<const u32x4*>(lds + buf * KT_BYTES + (hi ? 2 : 1) * HALF + (((wc * 2 + j) * 2 + ks) * 1024) + lane * 16);
    };

    // prologue: K-tile 0 whole and K-tile 1's low W -- what phase 0 expects to be in flight behind what it reads
    stage(0, 1, 0); stage(0, 0, 0); stage(0, 2, 0); stage(0, 3, 0); stage(1, 1, 1);
    asm volatile("s_waitcnt vmcnt(4)\n\ts_barrier" ::: "memory");
    if (grp) asm volatile("s_barrier" ::: "memory");          // group 1 starts one interval late

    f32x4 acc[4][MW];
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < MW; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 xr[LO][2], wl[2][2], wl2[2][2], wh[2][2];
#ifdef PP_STAMPS
    unsigned long long* st_buf = reinterpret_cast<unsigned long long*>(lds + SPARE + 8192 + grp * 4096);
    int st_n = 0;
    bool st_on = false;
#endif

#define PP_MFMA(WL, XCNT, XHI)                                                                                           \
    PP_T1();                                                                                                             \
    asm volatile("s_barrier\n\ts_waitcnt lgkmcnt(0)" ::: "memory");                                                      \
    PP_T();                                                                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                                                   \
    __builtin_amdgcn_s_setprio(1);                                                                                       \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                     \
        _Pragma("unroll") for (int i = 0; i < (XCNT); ++i) {                                                             \
            _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                \
                acc[j][(XHI) * LO + i] = tg_mfma(WL[j][ks], xr[i][ks], acc[j][(XHI) * LO + i]);                          \
            _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                \
                acc[2 + j][(XHI) * LO + i] = tg_mfma(wh[j][ks], xr[i][ks], acc[2 + j][(XHI) * LO + i]);                  \
        }                                                                                                                \
    __builtin_amdgcn_s_setprio(0);                                                                                       \
    __builtin_amdgcn_sched_barrier(0);                                                                                   \
    PP_T();                                                                                                              \
    asm volatile("s_barrier" ::: "memory");                                                                              \
    PP_T();
#define PP_KTILE(KT, BUF, WL, WLNEXT)                                                                                    \
    {                                                                                                                    \
        _Pragma("unroll") for (int i = 0; i < LO; ++i)                                                                   \
            _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) xr[i][ks] = lds_x(BUF, 0, i, ks);                           \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                    \
            _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) wh[j][ks] = lds_w(BUF, 1, j, ks);                           \
        stage((KT) + 1, 0, (BUF) ^ 1);                                                                                   \
        stage((KT) + 1, 2, (BUF) ^ 1);                                                                                   \
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
        PP_MFMA(WL, LO, 0)                                                                                               \
        _Pragma("unroll") for (int i = 0; i < HI; ++i)                                                                   \
            _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) xr[i][ks] = lds_x(BUF, 1, i, ks);                           \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                    \
            _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) WLNEXT[j][ks] = lds_w((BUF) ^ 1, 0, j, ks);                 \
        stage((KT) + 1, 3, (BUF) ^ 1);                                                                                   \
        stage((KT) + 2, 1, BUF);                                                                                         \
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                                                               \
        PP_MFMA(WL, HI, 1)                                                                                               \
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) wl[j][ks] = lds_w(0, 0, j, ks);
    PP_C(1);
    for (int u = 0; u < nkt; u += 2) {                        // an odd K-tile count runs one K-tile of zeros (staged out of range)
#ifdef PP_STAMPS
        st_on = st_wave && u >= 8 && u < 24;
        if (u == 8) PP_T();
#endif
        PP_KTILE(u, 0, wl, wl2)
        PP_KTILE(u + 1, 1, wl2, wl)
    }
#undef PP_KTILE
#undef PP_MFMA
    PP_C(2);
    if (!grp) asm volatile("s_barrier" ::: "memory");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
#if defined(PP_STAMPS) && PP_STAMPS != 3
    if (st_wave)
        for (int i = 0; i < st_n && i < 1023; ++i) g_pp_stamps[grp][1 + i] = st_buf[i];
    if (st_wave) g_pp_stamps[grp][0] = st_n;
#endif
    if (tile_plain(a)) tile_epilogue<4, MW, GU8, true>(a, acc, lds, wave, lane, m0 + grp * MW * 16, n0 + wc * 64);
    else tile_epilogue<4, MW, GU8, false>(a, acc, lds, wave, lane, m0 + grp * MW * 16, n0 + wc * 64);
#if defined(PP_STAMPS) && PP_STAMPS == 3
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    PP_C(3);
#endif
}

template <int MW, bool GU8>
static int launch_tile_pp(TileArgs a, hipStream_t st) {
    constexpr int BM = 32 * MW;
    a.mblocks = (a.M + BM - 1) / BM;
    a.nblocks = a.N / 256;
    a.band = tile_band(a.mblocks, a.nblocks);
#ifdef PP_STAMPS
    constexpr int LDS_BYTES = 128 * 1024 + TG_WAVES * 1024 + 8192 + 8192;
#else
    constexpr int LDS_BYTES = 128 * 1024 + TG_WAVES * 1024;
#endif
    return tile_launch<gemm_tile_pp_kernel<MW, GU8>>(dim3(a.mblocks * a.nblocks), LDS_BYTES, a, st, "omni_gemm_tile");
}

template <int WAVES_N, int WN, int WM, bool GU8, int MOE = 0>
static int launch_tile(const TileArgs& a, hipStream_t st, int groups = 1) {
    return tile_launch_geom<gemm_tile_kernel<WAVES_N, WN, WM, GU8, MOE>, TileGeom<WAVES_N, WN, WM>>(
        a, st, MOE ? "omni_moe_prefill_experts" : "omni_gemm_tile", groups);
}

// the instantiation a TileChoice (gemm_tile_policy.h) names
template <bool GU8>
static int launch_choice(const TileChoice& t, const TileArgs& a, hipStream_t st, int groups) {
    if (t.mw) return t.mw == 8 ? launch_tile_pp<8, GU8>(a, st) : (t.mw == 7 ? launch_tile_pp<7, GU8>(a, st) : launch_tile_pp<6, GU8>(a, st));
    switch (t.waves_n * 100 + t.wn * 10 + t.wm) {
    case 422: return launch_tile<4, 2, 2, GU8>(a, st, groups);
    case 284: return launch_tile<2, 8, 4, GU8>(a, st, groups);
    case 447: return launch_tile<4, 4, 7, GU8>(a, st, groups);
    case 446: return launch_tile<4, 4, 6, GU8>(a, st, groups);
    case 184: return launch_tile<1, 8, 4, GU8>(a, st, groups);
    case 264: if constexpr (!GU8) return launch_tile<2, 6, 4, false>(a, st, groups);        // (widths SiLU-mul never takes)
    case 164: if constexpr (!GU8) return launch_tile<1, 6, 4, false>(a, st, groups);
    }
    omni_set_error("omni_gemm_tile: no kernel for tile <%d, %d, %d> mw=%d", t.waves_n, t.wn, t.wm, t.mw);
    return OMNI_EINVAL;
}

extern "C" int omni_gemm_tile(const omni_tile_gemm* g, void* stream) {
    OMNI_CHECK_ARG(g && g->x && g->w && (g->out || g->out2 || g->out_f32), "omni_gemm_tile: null argument");
    OMNI_CHECK_ARG(g->M > 0 && g->N > 0 && g->N % 16 == 0 && g->K > 0 && g->K % 32 == 0, "omni_gemm_tile: M=%d N=%d K=%d (N %% 16, K %% 32)", g->M, g->N, g->K);
    const int seg_len = g->seg_len > 0 ? g->seg_len : g->K;
    OMNI_CHECK_ARG(seg_len % 32 == 0 && g->K % seg_len == 0, "omni_gemm_tile: seg_len=%d must divide K=%d and be a multiple of 32", seg_len, g->K);
    OMNI_CHECK_ARG(g->ldx % 8 == 0 && g->ldx >= seg_len, "omni_gemm_tile: ldx=%d (>= seg_len, multiple of 8)", g->ldx);
    OMNI_CHECK_ARG(g->x_rows > 0 && g->x_rows * (int64_t)g->ldx * 2 < (int64_t)TG_OOB, "omni_gemm_tile: x of %lld rows x %d exceeds the 2 GB descriptor", (long long)g->x_rows, g->ldx);
    OMNI_CHECK_ARG((int64_t)g->N * g->K * 2 < (int64_t)TG_OOB, "omni_gemm_tile: W exceeds the 2 GB descriptor");
    const bool gu8 = g->act == OMNI_TILE_ACT_SILU_MUL_GU8;
    OMNI_CHECK_ARG(g->act == OMNI_TILE_ACT_NONE || g->act == OMNI_TILE_ACT_GELU || gu8, "omni_gemm_tile: act=%d", g->act);
    OMNI_CHECK_ARG(g->tile_hint >= 0 && g->tile_hint <= 7, "omni_gemm_tile: tile_hint=%d", g->tile_hint);
    OMNI_CHECK_ARG(g->tile_hint < 3 || g->N % 256 == 0, "omni_gemm_tile: tile_hint=%d needs N %% 256 == 0", g->tile_hint);
    OMNI_CHECK_ARG(!gu8 || (g->out && !g->resid && !g->out2 && !g->out_f32), "omni_gemm_tile: SiLU-mul takes out only");
    OMNI_CHECK_ARG(!g->out2 || (g->snake_alpha && g->snake_inv_beta), "omni_gemm_tile: out2 needs the snake parameters");
    const int nout = gu8 ? g->N / 2 : g->N;
    OMNI_CHECK_ARG((!g->out || (g->ldo >= nout && g->ldo % 8 == 0)) && (!g->resid || (g->ldr >= nout && g->ldr % 4 == 0)) &&
                   (!g->out2 || (g->ldo2 >= nout && g->ldo2 % 8 == 0)) && (!g->out_f32 || (g->ldf >= nout && g->ldf % 4 == 0)),
                   "omni_gemm_tile: ldo / ldr / ldo2 / ldf (>= N; multiples of 8 (bf16) / 4 (fp32))");
    TileArgs a;
    a.x = (const uint16_t*)g->x; a.x_rows = g->x_rows; a.ldx = g->ldx;
    a.seg_len = seg_len; a.seg_rows = g->seg_rows; a.row_off = g->row_off;
    a.W = (const uint16_t*)g->w; a.bias = g->bias; a.scale = g->scale;
    a.resid = g->resid; a.ldr = g->ldr;
    a.out_f32 = g->out_f32; a.ldf = g->ldf;
    a.out = (uint16_t*)g->out; a.ldo = g->ldo;
    a.out2 = (uint16_t*)g->out2; a.ldo2 = g->ldo2; a.snake_alpha = g->snake_alpha; a.snake_inv_beta = g->snake_inv_beta;
    a.M = g->M; a.N = g->N; a.K = g->K; a.act = g->act;
    const int groups = g->groups > 1 ? g->groups : 1;
    OMNI_CHECK_ARG(groups <= 65535, "omni_gemm_tile: groups=%d", g->groups);
    OMNI_CHECK_ARG(groups == 1 || (seg_len == g->K && g->row_off == 0 && g->x_group_rows >= 0 && g->w_group_elems >= 0 && g->out_group_rows >= 0),
                   "omni_gemm_tile: a grouped launch is a plain GEMM per group (no conv window) with non-negative group strides");
    OMNI_CHECK_ARG(groups == 1 || (int64_t)groups * g->w_group_elems * 2 + (int64_t)g->N * g->K * 2 < ((int64_t)1 << 40), "omni_gemm_tile: W groups");
    a.gx_rows = groups > 1 ? g->x_group_rows : 0; a.gw_elems = groups > 1 ? g->w_group_elems : 0; a.gout_rows = groups > 1 ? g->out_group_rows : 0;
    a.group_rows = g->group_rows;
    const bool plain = groups == 1 && !g->group_rows && seg_len == g->K && g->row_off == 0;
    OMNI_CHECK_ARG(g->tile_hint < 5 || plain, "omni_gemm_tile: tile_hint=%d (two-group tile) takes a plain GEMM", g->tile_hint);
    const TileChoice t = tile_choice_bf16(g->M, g->N, groups, plain, gu8, g->tile_hint);
    return gu8 ? launch_choice<true>(t, a, (hipStream_t)stream, groups) : launch_choice<false>(t, a, (hipStream_t)stream, groups);
}

// ---- the MoE prefill's expert GEMMs over the compact batch (entry points: moe_prefill.hip), in the two block heights of TILE_MOE_BLOCK
// (tile_epi.cuh) with the K-slice order of every other geometry: bit-identical expert outputs.
bool k_moe_tile_fused_ok(int block, int I) { return I % (block == 64 ? 64 : 128) == 0; }     // half a block's columns of gate, half of up

int k_moe_tile_gemm(int mode, int block, const void* x, int64_t x_rows, int ldx, const void* w, int64_t w_expert_elems, int experts,
                    const int32_t* block_expert, const int32_t* row_token, const void* row_weight, void* out, int ldo, int rows, int N, int K,
                    void* stream) {
    OMNI_CHECK_ARG(x && w && block_expert && out && (mode == MOE_DOWN ? row_weight != nullptr : row_token != nullptr), "omni_moe_prefill_experts: null argument");
    OMNI_CHECK_ARG((block == 64 || block == 256) && rows > 0 && rows % block == 0, "omni_moe_prefill_experts: block=%d rows=%d", block, rows);
    OMNI_CHECK_ARG(N > 0 && N % 16 == 0 && K > 0 && K % 32 == 0 && ldx % 8 == 0 && ldx >= K && ldo % 8 == 0, "omni_moe_prefill_experts: N=%d K=%d ldx=%d ldo=%d", N, K, ldx, ldo);
    OMNI_CHECK_ARG(x_rows > 0 && x_rows * (int64_t)ldx * 2 < (int64_t)TG_OOB && (int64_t)N * K * 2 < (int64_t)TG_OOB, "omni_moe_prefill_experts: an operand exceeds the 2 GB descriptor");
    OMNI_CHECK_ARG(mode != MOE_DOWN || x_rows >= rows, "omni_moe_prefill_experts: act rows");
    OMNI_CHECK_ARG(mode != MOE_GU_FUSED || (N % 32 == 0 && k_moe_tile_fused_ok(block, N / 2)), "omni_moe_prefill_experts: the fused gate_up tile needs I %% %d == 0", block == 64 ? 64 : 128);
    OMNI_CHECK_ARG(experts >= 1 && w_expert_elems >= (int64_t)N * K, "omni_moe_prefill_experts: expert stride");
    TileArgs a{};
    a.x = (const uint16_t*)x; a.x_rows = x_rows; a.ldx = ldx;
    a.seg_len = K; a.seg_rows = 0; a.row_off = 0;
    a.W = (const uint16_t*)w; a.gw_elems = w_expert_elems;
    a.out = (uint16_t*)out; a.ldo = ldo;
    a.M = rows; a.N = N; a.K = K; a.act = OMNI_TILE_ACT_NONE;
    a.block_expert = block_expert; a.row_token = row_token; a.row_weight = (const uint16_t*)row_weight;
    hipStream_t st = (hipStream_t)stream;
    if (mode == MOE_GU_FUSED) return TILE_MOE_BLOCK(block, launch_tile, MOE_GU_FUSED, a, st);
    if (mode == MOE_GU_PLAIN) return TILE_MOE_BLOCK(block, launch_tile, MOE_GU_PLAIN, a, st);
    return TILE_MOE_BLOCK(block, launch_tile, MOE_DOWN, a, st);
}
