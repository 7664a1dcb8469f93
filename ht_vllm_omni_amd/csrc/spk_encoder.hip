// Speaker encoder of the Qwen3-TTS Base checkpoints (ECAPA-TDNN; reference: Qwen3TTSSpeakerEncoder and its blocks,
// V/model_executor/models/qwen3_tts/qwen3_tts_talker.py:57-239, called from _extract_speaker_embedding :1069-1105):
//     log-mel [T, mel_dim] -> one embedding [enc_dim].
// Activations are time-major [T, C] bf16; every product is bf16 x bf16 with fp32 accumulation; everything between two stored tensors
// is fp32 and a tensor is rounded once, where it is stored.  No launch reads the host, allocates or uses a floating atomic: every
// reduction has a fixed order, two runs give the same bits, and the whole call can be captured into a graph.
//
// Kernels
//   spk_conv_kernel     reflect-"same"-padded dilated conv1d as a GEMM over a row window: output row t, tap j reads input row
//                       reflect(t + (j - (k - 1) / 2) * dilation) -- a mirrored INDEX, never a zero row.  K index = tap * C_in + channel.
//                       4 waves, 64 rows x 64 columns per workgroup, operand fragments straight from L2 (the matrices of this network
//                       are small and shared by every row block), bias + none | ReLU | tanh | tanh(ReLU) epilogue, bf16 or fp32 output with its
//                       own row stride (the three block outputs are written side by side: the concatenation is never copied).
//   spk_res2net_kernel  the scale - 1 chained convolutions of a Res2Net block in ONE launch.  A workgroup owns 64 output rows and a
//                       128-row window around them (halo = (scale - 1) * pad rows per side, pad = dilation * (k - 1) / 2): every
//                       stage is computed for the whole window, so that interior tiles RE-COMPUTE their halo rows (after s stages
//                       the outer s * pad rows of a window are stale and no longer read by the tile's own rows), while at the two
//                       ends of the sequence every stage's input index is reflected, exactly as the per-stage convolutions do.
//                       The running chunk in_{s+1} = bf16(relu(conv_s(in_s)) + x_chunk[s+1]) lives in two LDS row buffers (16-byte
//                       row pad) and never goes to HBM; stage s + 1's [w, k w] weight slice and its x chunk are fetched into
//                       registers before stage s's MFMAs and stored to the other LDS weight buffer behind them; the concatenated
//                       [T, C] output is written once, chunk 0 passed through.
//   spk_colsum_kernel   stage 1 of the column statistics: per 32-row block the sums (and sums of squares) of every column.
//   spk_se_gate_kernel  stage 2 (fixed block order) -> mean; gate = sigmoid(W2 relu(W1 mean + b1) + b2), one workgroup.
//   spk_se_apply_kernel out = bf16(h * gate + residual).
//   spk_asp_bias_kernel uniform mean / std per channel from the column sums, folded into the attention bias:
//                       b' = b + W[:, C:2C] mean + W[:, 2C:3C] std  -- the attention GEMM then has K = C, not 3 C.
//   spk_pool_kernel     softmax over time per channel with an online max (16 channels x 16 time lanes per workgroup, merged in lane
//                       order), weighted mean, then a SECOND pass for sum a (x - mean)^2 and std = sqrt(max(var, eps)).
//   spk_matvec_kernel   out = bf16(W v + b), one wave per output row (the final fc).
//
// Supported range (anything else: OMNI_EINVAL)
//   mel_dim and every channel width, channels / scale, se_channels, attention_channels: multiples of 16; enc_dim >= 1
//   3 <= layers <= OMNI_SPK_MAX_LAYERS; channels[0 .. layers - 2] all equal C; channels[layers - 1] = (layers - 2) * C
//   kernel sizes odd, pad = dilation * (k - 1) / 2 <= 4, last kernel size 1; T > pad of every layer (T > 4 covers every config)
//   Res2Net: 2 <= scale, w = C / scale <= 64, (scale - 1) * pad <= 32, w * w * k <= 16384
#include "common.cuh"

#define SPK_PAD_MAX 4
#define R2_TT 64          // output rows of a Res2Net workgroup
#define R2_WR 128         // its window: R2_TT + 2 * halo rows, halo <= 32
#define R2_MAXP 8         // 16-byte weight pieces per thread and stage: w * w * k * 2 B <= 32 KB
#define CS_ROWS 32        // rows per block of the column sums

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

// One MFMA operand of KW k-values: lane (c = lane & 15, q = lane >> 4) holds row c, k = (KW / 4) q .. + KW / 4 - 1.  KW = 32 where the
// channel count allows, KW = 16 for widths that are odd multiples of 16 (v_mfma_f32_16x16x16_bf16).  With A = the weight tile and B = the
// activation tile, lane (c, q) of the result holds output row (time) c, output channels 4 q .. 4 q + 3.
// Weight tiles are stored in lane order: tile (n / 16, k / KW) = KW * 16 contiguous elements, element (row, kk) at
// ((kk / E) * 16 + row) * E + kk % E, E = KW / 4 (KW = 32: OMNI_LAYOUT_W_FRAG).
template <int KW> struct SpkFrag;
template <> struct SpkFrag<32> {
    typedef u32x4 T;
    static __device__ __forceinline__ f32x4 mfma(T a, T b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
template <> struct SpkFrag<16> {
    typedef u32x2 T;
    static __device__ __forceinline__ f32x4 mfma(T a, T b, f32x4 c) {
        return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4, a), __builtin_bit_cast(s16x4, b), c, 0, 0, 0);
    }
};

// input row of output row g at offset off: one reflection at either end of [0, T) (T > |off|)
__device__ __forceinline__ int spk_reflect(int g, int T) {
    if (g < 0) g = -g;
    if (g >= T) g = 2 * (T - 1) - g;
    return g;
}

// ------------------------------------------------------------------ reflect-padded dilated conv as a GEMM
struct SpkConvArgs {
    const uint16_t* x; int ldx;
    const uint16_t* w; const float* bias;
    uint16_t* out; int ldo; float* out_f32; int ldf;
    int T, Cin, N, taps, dil, act;
};

template <int KW>
__global__ __launch_bounds__(256) void spk_conv_kernel(const SpkConvArgs a) {
    using F = SpkFrag<KW>;
    constexpr int E = KW / 4;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = lane & 15, q = lane >> 4;
    const int m = blockIdx.x * 64 + wave * 16 + c;
    const int mr = min(m, a.T - 1);                       // rows past T compute a copy of the last row and store nothing
    const int KS = a.Cin / KW, NS = a.taps * KS, tiles = a.N / 16;
    const uint16_t* wp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) wp[j] = a.w + (size_t)min((int)blockIdx.y * 4 + j, tiles - 1) * NS * (KW * 16) + lane * E;
    f32x4 acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int tap = 0; tap < a.taps; ++tap) {
        const uint16_t* xr = a.x + (size_t)spk_reflect(mr + (tap - a.taps / 2) * a.dil, a.T) * a.ldx + E * q;
        const size_t wo = (size_t)tap * KS * (KW * 16);
        for (int ks = 0; ks < KS; ++ks) {
            const typename F::T xf = *reinterpret_cast<const typename F::T*>(xr + ks * KW);
            typename F::T wf[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) wf[j] = *reinterpret_cast<const typename F::T*>(wp[j] + wo + (size_t)ks * (KW * 16));
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = F::mfma(wf[j], xf, acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tile = blockIdx.y * 4 + j;
        if (tile >= tiles || m >= a.T) continue;
        const int n = tile * 16 + 4 * q;
        const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + n);
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float y = acc[j][e] + b[e];
            v[e] = a.act == OMNI_SPK_ACT_RELU ? fmaxf(y, 0.f) : a.act == OMNI_SPK_ACT_TANH ? tanhf(y) : a.act == OMNI_SPK_ACT_RELU_TANH ? tanhf(fmaxf(y, 0.f)) : y;
        }
        if (a.out_f32) *reinterpret_cast<f32x4*>(a.out_f32 + (size_t)m * a.ldf + n) = f32x4{v[0], v[1], v[2], v[3]};
        if (a.out) *reinterpret_cast<uint2*>(a.out + (size_t)m * a.ldo + n) = uint2{pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3])};
    }
}

static int spk_launch_conv(const SpkConvArgs& a, hipStream_t st, const char* what) {
    OMNI_CHECK_ARG(a.x && a.w && a.bias && (a.out || a.out_f32), "%s: null argument", what);
    OMNI_CHECK_ARG(a.Cin > 0 && a.Cin % 16 == 0 && a.N > 0 && a.N % 16 == 0 && a.ldx % 8 == 0 && a.ldx >= a.Cin, "%s: C_in=%d N=%d ldx=%d (multiples of 16)",
                   what, a.Cin, a.N, a.ldx);
    OMNI_CHECK_ARG((!a.out || (a.ldo >= a.N && a.ldo % 4 == 0)) && (!a.out_f32 || (a.ldf >= a.N && a.ldf % 4 == 0)), "%s: output stride", what);
    OMNI_CHECK_ARG(a.taps >= 1 && a.taps % 2 == 1 && a.dil >= 1 && a.dil * (a.taps / 2) <= SPK_PAD_MAX, "%s: kernel=%d dilation=%d (odd kernel, dilation * (kernel - 1) / 2 <= %d)",
                   what, a.taps, a.dil, SPK_PAD_MAX);
    OMNI_CHECK_ARG(a.T > a.dil * (a.taps / 2), "%s: T=%d frames: reflect padding needs T > %d", what, a.T, a.dil * (a.taps / 2));
    OMNI_CHECK_ARG(a.act >= OMNI_SPK_ACT_NONE && a.act <= OMNI_SPK_ACT_RELU_TANH, "%s: act=%d", what, a.act);
    const dim3 grid((a.T + 63) / 64, (a.N + 63) / 64);
    if (a.Cin % 32 == 0) hipLaunchKernelGGL(spk_conv_kernel<32>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(spk_conv_kernel<16>, grid, dim3(256), 0, st, a);
    OMNI_CHECK_LAUNCH(what);
    return OMNI_OK;
}

// ------------------------------------------------------------------ Res2Net block: scale - 1 chained convolutions, one launch
struct SpkRes2Args {
    const uint16_t* x; int ldx;
    uint16_t* out; int ldo;
    const uint16_t* w; const float* bias;
    int T, scale, taps, dil;
};

template <int NT, int KW>
__global__ __launch_bounds__(256) void spk_res2net_kernel(const SpkRes2Args a) {
    using F = SpkFrag<KW>;
    constexpr int W = NT * 16, E = KW / 4, KS = W / KW, PITCH = W * 2 + 16, CH = W / 8;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, q = lane >> 4;
    const int T = a.T, taps = a.taps;
    const int halo = (a.scale - 1) * a.dil * (taps / 2);
    const int NS = taps * KS, welems = W * taps * W, wpieces = welems / 8;
    uint8_t* const cur = lds;                              // two row buffers of R2_WR * PITCH bytes
    uint8_t* const wts = lds + 2 * R2_WR * PITCH;          // two weight buffers of welems * 2 bytes
    const int t0 = blockIdx.x * R2_TT, gbase = t0 - halo;

    // chunk 0 passes through; the window of chunk 1 (zero outside the sequence: those rows are never read by a row inside it) and the
    // first weight slice go to LDS
    for (int id = tid; id < R2_TT * CH; id += 256) {
        const int g = t0 + id / CH, p = id % CH;
        if (g < T) *reinterpret_cast<u32x4*>(a.out + (size_t)g * a.ldo + p * 8) = *reinterpret_cast<const u32x4*>(a.x + (size_t)g * a.ldx + p * 8);
    }
    for (int id = tid; id < R2_WR * CH; id += 256) {
        const int r = id / CH, p = id % CH, g = gbase + r;
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (g >= 0 && g < T) v = *reinterpret_cast<const u32x4*>(a.x + (size_t)g * a.ldx + W + p * 8);
        *reinterpret_cast<u32x4*>(cur + r * PITCH + p * 16) = v;
    }
    for (int id = tid; id < wpieces; id += 256) *reinterpret_cast<u32x4*>(wts + id * 16) = reinterpret_cast<const u32x4*>(a.w)[id];
    __syncthreads();

    for (int s = 1; s < a.scale; ++s) {
        const uint8_t* cin = cur + ((s - 1) & 1) * (R2_WR * PITCH);
        const uint8_t* win = wts + ((s - 1) & 1) * (welems * 2);
        uint8_t* cout = cur + (s & 1) * (R2_WR * PITCH);
        uint8_t* wout = wts + (s & 1) * (welems * 2);
        const bool more = s + 1 < a.scale;
        // the next stage's weight slice and x chunk: in flight behind this stage's MFMAs
        u32x4 wpre[R2_MAXP];
#pragma unroll
        for (int p = 0; p < R2_MAXP; ++p) {
            const int id = p * 256 + tid;
            wpre[p] = u32x4{0u, 0u, 0u, 0u};
            if (more && id < wpieces) wpre[p] = reinterpret_cast<const u32x4*>(a.w + (size_t)s * welems)[id];
        }
        uint2 xn[NT][2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
            const int g = gbase + (2 * wave + mi) * 16 + c;
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                xn[j][mi] = uint2{0u, 0u};
                if (more && g >= 0 && g < T) xn[j][mi] = *reinterpret_cast<const uint2*>(a.x + (size_t)g * a.ldx + (s + 1) * W + 16 * j + 4 * q);
            }
        }
        f32x4 acc[NT][2];
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int tap = 0; tap < taps; ++tap) {
            const uint8_t* xr[2];
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int gs = spk_reflect(gbase + (2 * wave + mi) * 16 + c + (tap - taps / 2) * a.dil, T);
                xr[mi] = cin + min(max(gs - gbase, 0), R2_WR - 1) * PITCH + E * q * 2;      // the clamp only ever moves rows outside [0, T)
            }
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                typename F::T xf[2], wf[NT];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) xf[mi] = *reinterpret_cast<const typename F::T*>(xr[mi] + ks * KW * 2);
#pragma unroll
                for (int j = 0; j < NT; ++j) wf[j] = *reinterpret_cast<const typename F::T*>(win + ((size_t)(j * NS + tap * KS + ks) * (KW * 16) + lane * E) * 2);
#pragma unroll
                for (int j = 0; j < NT; ++j)
#pragma unroll
                    for (int mi = 0; mi < 2; ++mi) acc[j][mi] = F::mfma(wf[j], xf[mi], acc[j][mi]);
            }
        }
        // y = relu(acc + b): the tile's own rows go to HBM, bf16(y + next chunk) of every window row to the other LDS buffer
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = 16 * j + 4 * q;
            const f32x4 b = *reinterpret_cast<const f32x4*>(a.bias + (s - 1) * W + n);
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int r = (2 * wave + mi) * 16 + c, g = gbase + r;
                float y[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] = fmaxf(acc[j][mi][e] + b[e], 0.f);
                if (g >= t0 && g < t0 + R2_TT && g < T)
                    *reinterpret_cast<uint2*>(a.out + (size_t)g * a.ldo + s * W + n) = uint2{pack_bf2(y[0], y[1]), pack_bf2(y[2], y[3])};
                if (more) {
                    const uint2 xv = xn[j][mi];
                    *reinterpret_cast<uint2*>(cout + r * PITCH + n * 2) =
                        uint2{pack_bf2(y[0] + bf_lo(xv.x), y[1] + bf_hi(xv.x)), pack_bf2(y[2] + bf_lo(xv.y), y[3] + bf_hi(xv.y))};
                }
            }
        }
        if (more) {
#pragma unroll
            for (int p = 0; p < R2_MAXP; ++p) {
                const int id = p * 256 + tid;
                if (id < wpieces) *reinterpret_cast<u32x4*>(wout + id * 16) = wpre[p];
            }
        }
        __syncthreads();      // the one barrier of a stage: stage s + 1 reads what stage s wrote, and writes what stage s read
    }
}

template <int NT, int KW>
static int spk_launch_res2net_t(const SpkRes2Args& a, hipStream_t st) {
    const int W = NT * 16;
    const int bytes = 2 * R2_WR * (W * 2 + 16) + 2 * W * a.taps * W * 2;
    static int attr_bytes = 0;
    if (bytes > attr_bytes) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(spk_res2net_kernel<NT, KW>), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) { omni_set_error("omni_spk_res2net: LDS attribute: %s", hipGetErrorString(e)); return OMNI_EHIP; }
        attr_bytes = bytes;
    }
    hipLaunchKernelGGL((spk_res2net_kernel<NT, KW>), dim3((a.T + R2_TT - 1) / R2_TT), dim3(256), bytes, st, a);
    OMNI_CHECK_LAUNCH("omni_spk_res2net");
    return OMNI_OK;
}

static int spk_launch_res2net(const SpkRes2Args& a, int C, hipStream_t st) {
    OMNI_CHECK_ARG(a.x && a.out && a.w && a.bias && a.x != a.out, "omni_spk_res2net: null or aliased argument");
    OMNI_CHECK_ARG(a.scale >= 2 && C > 0 && C % a.scale == 0 && (C / a.scale) % 16 == 0 && C / a.scale <= 64, "omni_spk_res2net: C=%d scale=%d (C / scale a multiple of 16, <= 64)", C, a.scale);
    const int w = C / a.scale, pad = a.dil * (a.taps / 2);
    OMNI_CHECK_ARG(a.taps >= 1 && a.taps % 2 == 1 && a.dil >= 1 && pad <= SPK_PAD_MAX && (a.scale - 1) * pad <= (R2_WR - R2_TT) / 2 && w * w * a.taps <= R2_MAXP * 256 * 8,
                   "omni_spk_res2net: kernel=%d dilation=%d scale=%d w=%d (pad <= %d, (scale - 1) * pad <= 32, w * w * kernel <= 16384)", a.taps, a.dil, a.scale, w, SPK_PAD_MAX);
    OMNI_CHECK_ARG(a.T > pad, "omni_spk_res2net: T=%d frames: reflect padding needs T > %d", a.T, pad);
    OMNI_CHECK_ARG(a.ldx >= C && a.ldo >= C && a.ldx % 8 == 0 && a.ldo % 8 == 0, "omni_spk_res2net: row strides %d / %d", a.ldx, a.ldo);
    switch (w / 16) {
    case 1: return spk_launch_res2net_t<1, 16>(a, st);
    case 2: return spk_launch_res2net_t<2, 32>(a, st);
    case 3: return spk_launch_res2net_t<3, 16>(a, st);
    default: return spk_launch_res2net_t<4, 32>(a, st);
    }
}

// ------------------------------------------------------------------ column statistics, squeeze-excitation, pooling
// fp32 dot product of a bf16 weight row with an fp32 vector over the wave: lane order inside, fixed butterfly across (K even)
__device__ __forceinline__ float spk_wave_dot(const uint16_t* wrow, const float* v, int K, int lane) {
    float acc = 0.f;
    for (int k = 2 * lane; k < K; k += 128) {
        const uint32_t ww = *reinterpret_cast<const uint32_t*>(wrow + k);
        acc = fmaf(bf_lo(ww), v[k], acc);
        acc = fmaf(bf_hi(ww), v[k + 1], acc);
    }
    return wave_sum(acc);
}

// part[b][c] = sum of x[t][c] over the CS_ROWS rows of block b in ascending t (and part_sq of x^2 when given)
__global__ __launch_bounds__(256) void spk_colsum_kernel(const uint16_t* x, int ldx, float* part, float* part_sq, int T, int C) {
    const int t0 = blockIdx.x * CS_ROWS, t1 = min(t0 + CS_ROWS, T);
    for (int col = 2 * threadIdx.x; col < C; col += 512) {
        float s0 = 0.f, s1 = 0.f, q0 = 0.f, q1 = 0.f;
        for (int t = t0; t < t1; ++t) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(x + (size_t)t * ldx + col);
            const float a = bf_lo(v), b = bf_hi(v);
            s0 += a; s1 += b;
            q0 = fmaf(a, a, q0); q1 = fmaf(b, b, q1);
        }
        *reinterpret_cast<float2*>(part + (size_t)blockIdx.x * C + col) = float2{s0, s1};
        if (part_sq) *reinterpret_cast<float2*>(part_sq + (size_t)blockIdx.x * C + col) = float2{q0, q1};
    }
}

// one workgroup: mean[c] = (sum over blocks, ascending) / T; s = relu(W1 mean + b1); gate = sigmoid(W2 s + b2)
__global__ __launch_bounds__(1024) void spk_se_gate_kernel(const float* part, int nblk, int T, int C, int S, const uint16_t* w1, const float* b1,
                                                           const uint16_t* w2, const float* b2, float* gate) {
    extern __shared__ float sev[];      // mean[C] | s[S]
    float* mean = sev;
    float* sq = sev + C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int col = threadIdx.x; col < C; col += 1024) {
        float s = 0.f;
        for (int b = 0; b < nblk; ++b) s += part[(size_t)b * C + col];
        mean[col] = s / (float)T;
    }
    __syncthreads();
    for (int r = wave; r < S; r += 16) {
        const float d = spk_wave_dot(w1 + (size_t)r * C, mean, C, lane);
        if (lane == 0) sq[r] = fmaxf(d + b1[r], 0.f);
    }
    __syncthreads();
    for (int r = wave; r < C; r += 16) {
        const float d = spk_wave_dot(w2 + (size_t)r * S, sq, S, lane);
        if (lane == 0) gate[r] = 1.f / (1.f + expf(-(d + b2[r])));
    }
}

// out = bf16(h * gate + resid), 8 columns per thread
__global__ __launch_bounds__(256) void spk_se_apply_kernel(const uint16_t* h, int ldh, const float* gate, const uint16_t* resid, int ldr, uint16_t* out, int ldo,
                                                           int T, int C) {
    const int per = C / 8;
    const int id = blockIdx.x * 256 + threadIdx.x;
    if (id >= T * per) return;
    const int t = id / per, col = (id % per) * 8;
    const u32x4 hv = *reinterpret_cast<const u32x4*>(h + (size_t)t * ldh + col);
    const u32x4 rv = *reinterpret_cast<const u32x4*>(resid + (size_t)t * ldr + col);
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gate + col), g1 = *reinterpret_cast<const f32x4*>(gate + col + 4);
    u32x4 o;
    o[0] = pack_bf2(fmaf(bf_lo(hv[0]), g0[0], bf_lo(rv[0])), fmaf(bf_hi(hv[0]), g0[1], bf_hi(rv[0])));
    o[1] = pack_bf2(fmaf(bf_lo(hv[1]), g0[2], bf_lo(rv[1])), fmaf(bf_hi(hv[1]), g0[3], bf_hi(rv[1])));
    o[2] = pack_bf2(fmaf(bf_lo(hv[2]), g1[0], bf_lo(rv[2])), fmaf(bf_hi(hv[2]), g1[1], bf_hi(rv[2])));
    o[3] = pack_bf2(fmaf(bf_lo(hv[3]), g1[2], bf_lo(rv[3])), fmaf(bf_hi(hv[3]), g1[3], bf_hi(rv[3])));
    *reinterpret_cast<u32x4*>(out + (size_t)t * ldo + col) = o;
}

// one workgroup: uniform mean / std per channel (std = sqrt(max(E[x^2] - mean^2, eps)): these two only steer the attention, the
// pooled statistics below take the second pass), then bias'[r] = b[r] + Wms[r, :] . [mean | std]
__global__ __launch_bounds__(1024) void spk_asp_bias_kernel(const float* part, const float* part_sq, int nblk, int T, int C, int A, const uint16_t* wms,
                                                            const float* b, float eps, float* bias_out) {
    extern __shared__ float ms[];       // mean[C] | std[C]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int col = threadIdx.x; col < C; col += 1024) {
        float s = 0.f, s2 = 0.f;
        for (int k = 0; k < nblk; ++k) { s += part[(size_t)k * C + col]; s2 += part_sq[(size_t)k * C + col]; }
        const float mean = s / (float)T;
        ms[col] = mean;
        ms[C + col] = sqrtf(fmaxf(s2 / (float)T - mean * mean, eps));
    }
    __syncthreads();
    for (int r = wave; r < A; r += 16) {
        const float d = spk_wave_dot(wms + (size_t)r * 2 * C, ms, 2 * C, lane);
        if (lane == 0) bias_out[r] = b[r] + d;
    }
}

// softmax over time per channel + weighted mean / std: 16 channels x 16 time lanes per workgroup
__global__ __launch_bounds__(256) void spk_pool_kernel(const uint16_t* h, int ldh, const float* logits, int ldl, float* stats, int T, int C, float eps) {
    __shared__ float pm[16][16], ps[16][16], px[16][16];
    __shared__ float gm[16], gs[16], gmean[16];
    const int ch = threadIdx.x & 15, tl = threadIdx.x >> 4;
    const int col = blockIdx.x * 16 + ch;
    float m = -INFINITY, s = 0.f, sx = 0.f;
    for (int t = tl; t < T; t += 16) {
        const float l = logits[(size_t)t * ldl + col], x = bf2f(h[(size_t)t * ldh + col]);
        if (l > m) {
            const float sc = expf(m - l);       // first element: exp(-inf) = 0
            s = fmaf(s, sc, 1.f);
            sx = fmaf(sx, sc, x);
            m = l;
        } else {
            const float e = expf(l - m);
            s += e;
            sx = fmaf(e, x, sx);
        }
    }
    pm[tl][ch] = m; ps[tl][ch] = s; px[tl][ch] = sx;
    __syncthreads();
    if (tl == 0) {
        float M = pm[0][ch];
        for (int i = 1; i < 16; ++i) M = fmaxf(M, pm[i][ch]);
        float S = 0.f, SX = 0.f;
        for (int i = 0; i < 16; ++i) {
            const float sc = ps[i][ch] > 0.f ? expf(pm[i][ch] - M) : 0.f;     // an empty lane (T < 16) has m = -inf, s = 0
            S = fmaf(ps[i][ch], sc, S);
            SX = fmaf(px[i][ch], sc, SX);
        }
        gm[ch] = M; gs[ch] = S; gmean[ch] = SX / S;
    }
    __syncthreads();
    const float M = gm[ch], mean = gmean[ch];
    float v = 0.f;
    for (int t = tl; t < T; t += 16) {
        const float d = bf2f(h[(size_t)t * ldh + col]) - mean;
        v = fmaf(expf(logits[(size_t)t * ldl + col] - M), d * d, v);
    }
    px[tl][ch] = v;
    __syncthreads();
    if (tl == 0) {
        float V = 0.f;
        for (int i = 0; i < 16; ++i) V += px[i][ch];
        stats[col] = mean;
        stats[C + col] = sqrtf(fmaxf(V / gs[ch], eps));
    }
}

// out[n] = bf16(W[n, :] . v + b[n]): one wave per row
__global__ __launch_bounds__(256) void spk_matvec_kernel(const uint16_t* w, const float* v, const float* b, uint16_t* out, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= N) return;
    const float d = spk_wave_dot(w + (size_t)row * K, v, K, lane);
    if (lane == 0) out[row] = f2bf(d + b[row]);
}

// ------------------------------------------------------------------ host side
static inline int64_t spk_up(int64_t b) { return (b + 255) / 256 * 256; }

struct SpkShape { int C, C3, nblocks; };

static int spk_check_desc(const omni_spk_desc* d, SpkShape* sh) {
    OMNI_CHECK_ARG(d, "omni_spk: null descriptor");
    OMNI_CHECK_ARG(d->layers >= 3 && d->layers <= OMNI_SPK_MAX_LAYERS, "omni_spk: layers=%d (3 .. %d)", d->layers, OMNI_SPK_MAX_LAYERS);
    const int C = d->channels[0], C3 = d->channels[d->layers - 1];
    for (int i = 0; i < d->layers - 1; ++i) OMNI_CHECK_ARG(d->channels[i] == C, "omni_spk: channels[%d]=%d differs from channels[0]=%d (the residual add needs equal widths)", i, d->channels[i], C);
    OMNI_CHECK_ARG(C3 == (d->layers - 2) * C, "omni_spk: channels[last]=%d is not %d blocks x %d", C3, d->layers - 2, C);
    OMNI_CHECK_ARG(d->mel_dim > 0 && d->mel_dim % 16 == 0 && C > 0 && C % 16 == 0 && d->se_channels > 0 && d->se_channels % 16 == 0 && d->att_channels > 0 &&
                   d->att_channels % 16 == 0 && d->enc_dim >= 1, "omni_spk: mel_dim=%d C=%d se=%d attention=%d enc_dim=%d (widths are multiples of 16)", d->mel_dim, C, d->se_channels,
                   d->att_channels, d->enc_dim);
    OMNI_CHECK_ARG(d->kernels[d->layers - 1] == 1, "omni_spk: the aggregation layer's kernel size is %d, not 1", d->kernels[d->layers - 1]);
    sh->C = C; sh->C3 = C3; sh->nblocks = d->layers - 2;
    return OMNI_OK;
}

// scratch regions for T frames (each 256-byte aligned)
struct SpkScratch {
    uint16_t *a0, *cat, *t1, *t2, *t3, *mfa, *att;
    float *logits, *part, *part_sq, *gate, *biasp, *stats;
    int64_t bytes;
};
static SpkScratch spk_carve(const omni_spk_desc* d, const SpkShape& sh, int T, void* base) {
    SpkScratch s;
    int64_t off = 0;
    uint8_t* p = (uint8_t*)base;
    auto take = [&](int64_t bytes) { uint8_t* r = p + off; off += spk_up(bytes); return r; };
    const int64_t nblk = (T + CS_ROWS - 1) / CS_ROWS;
    s.a0 = (uint16_t*)take((int64_t)T * sh.C * 2);
    s.cat = (uint16_t*)take((int64_t)T * sh.C3 * 2);
    s.t1 = (uint16_t*)take((int64_t)T * sh.C * 2);
    s.t2 = (uint16_t*)take((int64_t)T * sh.C * 2);
    s.t3 = (uint16_t*)take((int64_t)T * sh.C * 2);
    s.mfa = (uint16_t*)take((int64_t)T * sh.C3 * 2);
    s.att = (uint16_t*)take((int64_t)T * d->att_channels * 2);
    s.logits = (float*)take((int64_t)T * sh.C3 * 4);
    s.part = (float*)take(nblk * sh.C3 * 4);
    s.part_sq = (float*)take(nblk * sh.C3 * 4);
    s.gate = (float*)take((int64_t)sh.C * 4);
    s.biasp = (float*)take((int64_t)d->att_channels * 4);
    s.stats = (float*)take((int64_t)2 * sh.C3 * 4);
    s.bytes = off;
    return s;
}

extern "C" int64_t omni_spk_scratch_bytes(const omni_spk_desc* d, int T) {
    SpkShape sh;
    if (spk_check_desc(d, &sh) != OMNI_OK) return OMNI_EINVAL;
    if (T < 1) { omni_set_error("omni_spk_scratch_bytes: T=%d", T); return OMNI_EINVAL; }
    return spk_carve(d, sh, T, nullptr).bytes;
}

extern "C" int omni_spk_conv(const void* x, int ldx, const void* w, const float* bias, void* out, int ldo, int T, int C_in, int N, int kernel,
                             int dilation, int act, void* stream) {
    SpkConvArgs a{(const uint16_t*)x, ldx, (const uint16_t*)w, bias, (uint16_t*)out, ldo, nullptr, 0, T, C_in, N, kernel, dilation, act};
    return spk_launch_conv(a, (hipStream_t)stream, "omni_spk_conv");
}

extern "C" int omni_spk_res2net(const void* x, int ldx, const void* w, const float* bias, void* out, int ldo, int T, int C, int scale, int kernel,
                                int dilation, void* stream) {
    SpkRes2Args a{(const uint16_t*)x, ldx, (uint16_t*)out, ldo, (const uint16_t*)w, bias, T, scale, kernel, dilation};
    return spk_launch_res2net(a, C, (hipStream_t)stream);
}

// attentive statistics pooling of h [T, C3] -> stats fp32 [2 C3] = [mean | std]
static int spk_asp(const omni_spk_desc* d, const SpkShape& sh, const uint16_t* h, int ldh, int T, float* stats, const SpkScratch& s, hipStream_t st) {
    OMNI_CHECK_ARG(d->att_wh && d->att_wms && d->att_b && d->att_conv_w && d->att_conv_b, "omni_spk_asp: null weight");
    const int C3 = sh.C3, A = d->att_channels, nblk = (T + CS_ROWS - 1) / CS_ROWS;
    const float eps = 1e-12f;
    hipLaunchKernelGGL(spk_colsum_kernel, dim3(nblk), dim3(256), 0, st, h, ldh, s.part, s.part_sq, T, C3);
    hipLaunchKernelGGL(spk_asp_bias_kernel, dim3(1), dim3(1024), 2 * C3 * sizeof(float), st, s.part, s.part_sq, nblk, T, C3, A, (const uint16_t*)d->att_wms, d->att_b, eps,
                       s.biasp);
    OMNI_CHECK_LAUNCH("omni_spk_asp: statistics");
    SpkConvArgs c1{h, ldh, (const uint16_t*)d->att_wh, s.biasp, s.att, A, nullptr, 0, T, C3, A, 1, 1, OMNI_SPK_ACT_RELU_TANH};      // the attention TDNN block ends in ReLU; tanh follows
    int rc = spk_launch_conv(c1, st, "omni_spk_asp: attention tdnn");
    if (rc) return rc;
    SpkConvArgs c2{s.att, A, (const uint16_t*)d->att_conv_w, d->att_conv_b, nullptr, 0, s.logits, C3, T, A, C3, 1, 1, OMNI_SPK_ACT_NONE};
    rc = spk_launch_conv(c2, st, "omni_spk_asp: attention conv");
    if (rc) return rc;
    hipLaunchKernelGGL(spk_pool_kernel, dim3(C3 / 16), dim3(256), 0, st, h, ldh, s.logits, C3, stats, T, C3, eps);
    OMNI_CHECK_LAUNCH("omni_spk_asp: pooling");
    return OMNI_OK;
}

extern "C" int omni_spk_asp(const omni_spk_desc* d, const void* h, int T, float* stats, void* scratch, void* stream) {
    SpkShape sh;
    int rc = spk_check_desc(d, &sh);
    if (rc) return rc;
    OMNI_CHECK_ARG(h && stats && scratch && T >= 1, "omni_spk_asp: null argument or T=%d", T);
    return spk_asp(d, sh, (const uint16_t*)h, sh.C3, T, stats, spk_carve(d, sh, T, scratch), (hipStream_t)stream);
}

extern "C" int omni_spk_encode(const omni_spk_desc* d, const void* mel, int T, void* out, void* scratch, void* stream) {
    SpkShape sh;
    int rc = spk_check_desc(d, &sh);
    if (rc) return rc;
    OMNI_CHECK_ARG(mel && out && scratch, "omni_spk_encode: null argument");
    OMNI_CHECK_ARG(T > SPK_PAD_MAX, "omni_spk_encode: T=%d frames: reflect padding needs T > %d", T, SPK_PAD_MAX);
    OMNI_CHECK_ARG(d->conv0_w && d->conv0_b && d->mfa_w && d->mfa_b && d->fc_w && d->fc_b, "omni_spk_encode: null weight");
    hipStream_t st = (hipStream_t)stream;
    const SpkScratch s = spk_carve(d, sh, T, scratch);
    const int C = sh.C, C3 = sh.C3, S = d->se_channels, nblk = (T + CS_ROWS - 1) / CS_ROWS;
    SpkConvArgs c0{(const uint16_t*)mel, d->mel_dim, (const uint16_t*)d->conv0_w, d->conv0_b, s.a0, C, nullptr, 0, T, d->mel_dim, C, d->kernels[0], d->dilations[0],
                   OMNI_SPK_ACT_RELU};
    if ((rc = spk_launch_conv(c0, st, "omni_spk_encode: block 0"))) return rc;
    const uint16_t* in = s.a0;
    int ldin = C;
    for (int i = 0; i < sh.nblocks; ++i) {
        const omni_spk_block* b = &d->blocks[i];
        OMNI_CHECK_ARG(b->tdnn1_w && b->tdnn1_b && b->res_w && b->res_b && b->tdnn2_w && b->tdnn2_b && b->se1_w && b->se1_b && b->se2_w && b->se2_b,
                       "omni_spk_encode: block %d: null weight", i + 1);
        SpkConvArgs t1{in, ldin, (const uint16_t*)b->tdnn1_w, b->tdnn1_b, s.t1, C, nullptr, 0, T, C, C, 1, 1, OMNI_SPK_ACT_RELU};
        if ((rc = spk_launch_conv(t1, st, "omni_spk_encode: tdnn1"))) return rc;
        SpkRes2Args r2{s.t1, C, s.t2, C, (const uint16_t*)b->res_w, b->res_b, T, d->scale, d->kernels[i + 1], d->dilations[i + 1]};
        if ((rc = spk_launch_res2net(r2, C, st))) return rc;
        SpkConvArgs t2{s.t2, C, (const uint16_t*)b->tdnn2_w, b->tdnn2_b, s.t3, C, nullptr, 0, T, C, C, 1, 1, OMNI_SPK_ACT_RELU};
        if ((rc = spk_launch_conv(t2, st, "omni_spk_encode: tdnn2"))) return rc;
        hipLaunchKernelGGL(spk_colsum_kernel, dim3(nblk), dim3(256), 0, st, (const uint16_t*)s.t3, C, s.part, (float*)nullptr, T, C);
        hipLaunchKernelGGL(spk_se_gate_kernel, dim3(1), dim3(1024), (C + S) * sizeof(float), st, (const float*)s.part, nblk, T, C, S, (const uint16_t*)b->se1_w, b->se1_b,
                           (const uint16_t*)b->se2_w, b->se2_b, s.gate);
        uint16_t* bout = s.cat + (size_t)i * C;          // block i's output = columns [i C, (i + 1) C) of the aggregation layer's input
        hipLaunchKernelGGL(spk_se_apply_kernel, dim3((T * (C / 8) + 255) / 256), dim3(256), 0, st, (const uint16_t*)s.t3, C, (const float*)s.gate, in, ldin, bout, C3, T, C);
        OMNI_CHECK_LAUNCH("omni_spk_encode: squeeze-excitation");
        in = bout;
        ldin = C3;
    }
    SpkConvArgs mf{s.cat, C3, (const uint16_t*)d->mfa_w, d->mfa_b, s.mfa, C3, nullptr, 0, T, C3, C3, 1, 1, OMNI_SPK_ACT_RELU};
    if ((rc = spk_launch_conv(mf, st, "omni_spk_encode: aggregation"))) return rc;
    if ((rc = spk_asp(d, sh, s.mfa, C3, T, s.stats, s, st))) return rc;
    hipLaunchKernelGGL(spk_matvec_kernel, dim3((d->enc_dim + 3) / 4), dim3(256), 0, st, (const uint16_t*)d->fc_w, (const float*)s.stats, d->fc_b, (uint16_t*)out, d->enc_dim,
                       2 * C3);
    OMNI_CHECK_LAUNCH("omni_spk_encode: fc");
    return OMNI_OK;
}
