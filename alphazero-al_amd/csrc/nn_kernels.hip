// nn_kernels.hip - the two element-wise kernels of the Connect4 evaluator that are left outside its three fused launches
// (stem + first block, residual blocks, attention + heads: nn_conv.hip, nn_stem.hip, nn_attn_heads.hip).
//
//   k_embed<32>    the token embedding on its own (az_nn_embed).  No route runs it: it is kept as the ORACLE of the stem
//                  tests, which hold the stem kernels with the embedding fused in to az_nn_embed + az_nn_conv_block(c_in 32)
//                  bit for bit.
//   k_heads_prep   the policy head's column pooling and the value head's token mean (az_nn_heads_prep): what
//                  fast_net.FastConnect4Net.forward's log-probability path runs in front of its torch heads, and the
//                  oracle of the heads tests.
//
// 16-byte loads and stores (8 bf16 per lane), statistics in fp32, 8-lane shuffle reductions, LDS only in the head
// pooling.  Layout: tokens (B, 42, C) bf16 == channels-last image.
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdint>

#include "az_nn.h"

namespace {

constexpr int CELLS = 42, ROWS = 6, COLS = 7;

struct alignas(16) V8 { uint32_t w[4]; };        // 8 bf16

__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }

__device__ __forceinline__ uint32_t pack_bf16(float a, float b)
{
    const __hip_bfloat16 x = __float2bfloat16(a), y = __float2bfloat16(b);   // round to nearest even
    return static_cast<uint32_t>(*reinterpret_cast<const uint16_t *>(&x)) |
           (static_cast<uint32_t>(*reinterpret_cast<const uint16_t *>(&y)) << 16);
}

__device__ __forceinline__ void unpack8(const V8 &v, float f[8])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[2 * i] = bf_lo(v.w[i]); f[2 * i + 1] = bf_hi(v.w[i]); }
}

__device__ __forceinline__ V8 pack8(const float f[8])
{
    V8 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v.w[i] = pack_bf16(f[2 * i], f[2 * i + 1]);
    return v;
}

// ---------------------------------------------------------------- embedding
// tokens[b, cell, :] = pos[cell, :] + own * e_own + opp * e_opp      (Network.py:226-239)
template <int E>
__global__ void __launch_bounds__(256) k_embed(const float *feat, const uint16_t *e_own, const uint16_t *e_opp,
                                               const uint16_t *pos, uint16_t *tokens, int64_t B,
                                               const int32_t *gather, const int64_t *batch_dev)
{
    constexpr int VPT = E / 8;
    const int64_t rows_total = B;
    if (batch_dev != nullptr && *batch_dev < B) B = *batch_dev;
    const int64_t gid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    const int64_t tok = gid / VPT;
    const int vec = static_cast<int>(gid - tok * VPT);
    if (tok >= B * CELLS) return;
    const int64_t b = tok / CELLS;
    const int cell = static_cast<int>(tok - b * CELLS);
    int64_t src = gather != nullptr ? gather[b] : b;             // row of `feat` that sample b of the compact batch shows
    if (src < 0 || src >= rows_total) src = 0;
    const float own = feat[src * 3 * CELLS + cell], opp = feat[src * 3 * CELLS + CELLS + cell];
    float p[8], a[8], o[8], r[8];
    unpack8(*reinterpret_cast<const V8 *>(pos + cell * E + vec * 8), p);
    unpack8(*reinterpret_cast<const V8 *>(e_own + vec * 8), a);
    unpack8(*reinterpret_cast<const V8 *>(e_opp + vec * 8), o);
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = p[i] + own * a[i] + opp * o[i];
    *reinterpret_cast<V8 *>(tokens + tok * E + vec * 8) = pack8(r);
}

// ---------------------------------------------------------------- head pooling
// Per sample (one wavefront): RMSNorm of the 42 tokens with the policy head's norm weight,
// row-gate score per token, softmax over the 6 rows of every column, weighted column sum
// (Network.py:107-113) -> col (B, 7, 64); and the plain token mean for the value head
// (Network.py:135) -> mean (B, 64).
__global__ void __launch_bounds__(64) k_heads_prep(const uint16_t *tok, const uint16_t *p_norm_w,
                                                   const uint16_t *p_gate_w, float p_gate_b, uint16_t *col,
                                                   uint16_t *mean, int64_t B, float eps)
{
    __shared__ float s_pn[CELLS * 64];
    __shared__ float s_score[CELLS + 6];
    const int64_t b = blockIdx.x;
    if (b >= B) return;
    const int lane = threadIdx.x;
    const int sub = lane >> 3, vec = lane & 7;             // token slot (0-7), channel vector
    const uint16_t *xs = tok + b * (CELLS * 64);
    float nw[8], gw[8];
    unpack8(*reinterpret_cast<const V8 *>(p_norm_w + vec * 8), nw);
    unpack8(*reinterpret_cast<const V8 *>(p_gate_w + vec * 8), gw);
    float msum[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int t = sub + 8 * k;
        const bool live = t < CELLS;
        float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (live) unpack8(*reinterpret_cast<const V8 *>(xs + t * 64 + vec * 8), a);
        float ss = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) { ss += a[i] * a[i]; msum[i] += a[i]; }
        ss += __shfl_xor(ss, 1, 8); ss += __shfl_xor(ss, 2, 8); ss += __shfl_xor(ss, 4, 8);
        const float r = rsqrtf(ss * (1.0f / 64.0f) + eps);
        float sc = 0.0f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            // the reference rounds the normalised token to bf16 before the gate and the pooling
            const float pn = __bfloat162float(__float2bfloat16(a[i] * r * nw[i]));
            a[i] = pn;
            sc += pn * gw[i];
        }
        sc += __shfl_xor(sc, 1, 8); sc += __shfl_xor(sc, 2, 8); sc += __shfl_xor(sc, 4, 8);
        if (live) {
#pragma unroll
            for (int i = 0; i < 8; ++i) s_pn[t * 64 + vec * 8 + i] = a[i];
            if (vec == 0) s_score[t] = sc + p_gate_b;
        }
    }
    __syncthreads();
    // softmax over rows, per column; then weighted sum over rows: 7*64 outputs, 7 per lane
#pragma unroll
    for (int c = 0; c < COLS; ++c) {
        float sc[ROWS], mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) { sc[r] = s_score[r * COLS + c]; mx = fmaxf(mx, sc[r]); }
        float den = 0.0f;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) { sc[r] = __expf(sc[r] - mx); den += sc[r]; }
        const float inv = 1.0f / den;
        float acc = 0.0f;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const float w = __bfloat162float(__float2bfloat16(sc[r] * inv));
            acc += w * s_pn[(r * COLS + c) * 64 + lane];
        }
        const __hip_bfloat16 o = __float2bfloat16(acc);
        col[(b * COLS + c) * 64 + lane] = *reinterpret_cast<const uint16_t *>(&o);
    }
    // token mean: reduce the 8 token slots that share a channel vector
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float m = msum[i];
        m += __shfl_xor(m, 8, 64); m += __shfl_xor(m, 16, 64); m += __shfl_xor(m, 32, 64);
        msum[i] = m * (1.0f / CELLS);
    }
    if (sub == 0) *reinterpret_cast<V8 *>(mean + b * 64 + vec * 8) = pack8(msum);
}

inline unsigned blocks(int64_t threads, int per) { return static_cast<unsigned>((threads + per - 1) / per); }
inline const uint16_t *u16(const void *p) { return static_cast<const uint16_t *>(p); }
inline uint16_t *u16(void *p) { return static_cast<uint16_t *>(p); }

}  // namespace

extern "C" {

int az_nn_embed(const float *features, const void *emb_own, const void *emb_opp, const void *pos, void *tokens,
                int64_t batch, int embed_dim, const int32_t *gather, const int64_t *batch_dev, void *stream)
{
    if (embed_dim != 32 || batch <= 0) return 1;
    hipLaunchKernelGGL(k_embed<32>, dim3(blocks(batch * CELLS * 4, 256)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       features, u16(emb_own), u16(emb_opp), u16(pos), u16(tokens), batch, gather, batch_dev);
    return 0;
}

int az_nn_heads_prep(const void *tokens, const void *p_norm_w, const void *p_gate_w, float p_gate_b, void *col,
                     void *mean, int64_t batch, float eps, void *stream)
{
    if (batch <= 0) return 1;
    hipLaunchKernelGGL(k_heads_prep, dim3(static_cast<unsigned>(batch)), dim3(64), 0, static_cast<hipStream_t>(stream),
                       u16(tokens), u16(p_norm_w), u16(p_gate_w), p_gate_b, u16(col), u16(mean), batch, eps);
    return 0;
}

}  // extern "C"
