// One row of the fused residual-add + RMSNorm, held in the registers of one wave: the arithmetic of omni_rmsnorm in one place for its
// two users -- rmsnorm_kernel (norm.hip: the bf16 normalised row goes to HBM) and quant_rows_f8_kernel (gemm_prefill_f8.hip: the row is
// quantised to fp8 in registers and only its bytes go to HBM).  Numerics (HF Qwen3RMSNorm; oracle talker_oracle.rms_norm):
//   r = bf16(residual + delta);  out = w * bf16(r * rsqrt(mean(r^2) + eps))   (product rounds to bf16)
// Lane l owns the 8-element vectors l, l + 64, ... of the row; fp32 statistics, wave64 butterfly reduce.
#pragma once
#include "common.cuh"

template <int MAXV>   // MAXV = max 8-element vectors per lane (hidden <= 64 * 8 * MAXV)
struct NormRow {
    float v[MAXV][8];
    uint4 wv[MAXV];                       // norm weights: issued up front, consumed after the reduction

    // loads the row `src` (+ `delta`: the sum goes to `res_out`; without delta a row is copied to res_out when `copy`) and the norm
    // weights; returns rstd
    __device__ __forceinline__ float load(const uint16_t* src /* may be res_out */, const uint16_t* __restrict__ delta, uint16_t* res_out, bool copy,
                                          const uint16_t* __restrict__ w, int hidden, float eps, int lane) {
        const int nvec = hidden >> 3;
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int vi = lane + i * 64;
            wv[i] = (vi < nvec) ? *reinterpret_cast<const uint4*>(w + vi * 8) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int vi = lane + i * 64;
            if (vi < nvec) {
                uint4 a = *reinterpret_cast<const uint4*>(src + vi * 8);
                const uint32_t* aw = reinterpret_cast<const uint32_t*>(&a);
                if (delta) {
                    uint4 d = *reinterpret_cast<const uint4*>(delta + vi * 8);
                    const uint32_t* dw = reinterpret_cast<const uint32_t*>(&d);
                    uint32_t o[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float lo = bfround(bf_lo(aw[j]) + bf_lo(dw[j]));
                        const float hi = bfround(bf_hi(aw[j]) + bf_hi(dw[j]));
                        v[i][2 * j] = lo;
                        v[i][2 * j + 1] = hi;
                        o[j] = pack_bf2(lo, hi);
                    }
                    *reinterpret_cast<uint4*>(res_out + vi * 8) = make_uint4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        v[i][2 * j] = bf_lo(aw[j]);
                        v[i][2 * j + 1] = bf_hi(aw[j]);
                    }
                    if (copy) *reinterpret_cast<uint4*>(res_out + vi * 8) = a;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) ss += v[i][j] * v[i][j];
            }
        }
        ss = wave_sum(ss);
        return rsqrtf(ss / (float)hidden + eps);
    }

    // vector i of the normalised row: 8 bf16 values, packed
    __device__ __forceinline__ uint4 normed(int i, float rstd) const {
        const uint32_t* wp = reinterpret_cast<const uint32_t*>(&wv[i]);
        uint32_t o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float lo = bf_lo(wp[j]) * bfround(v[i][2 * j] * rstd);
            const float hi = bf_hi(wp[j]) * bfround(v[i][2 * j + 1] * rstd);
            o[j] = pack_bf2(lo, hi);
        }
        return make_uint4(o[0], o[1], o[2], o[3]);
    }
};
