// nn_attn.hip - the evaluator's gated attention block as ONE MFMA kernel.
//
//   y = x + o_proj( sigmoid(gate) * softmax(q_norm(Q) k_norm(K)^T / sqrt(16)) V )
//   with [Q | K | V | gate] = qkvg_proj(RMSNorm(x))                     (Network.py:51-93)
//
// One wavefront owns one sample; the attention itself is attn::attn_sample of nn_attn_core.h (the orientation of its
// products, and why no intermediate leaves the registers, is described there), shared with the fused kernel of
// nn_attn_heads.hip.  This kernel adds the residual and stores y.  HBM traffic: read x, write y.  Replaces RMSNorm +
// 196-wide GEMM + split/normalise + SDPA + gate + out-projection (six kernels, 1.8 ms per 32768-leaf iteration in
// the first profile).
//
// Three workgroups of four wavefronts per CU (three wavefronts per SIMD): 167 registers, the per-sample constants and
// the gates in LDS (37 KB per workgroup).  k_attn_block<true> is the same kernel with rsqrtf() for its reciprocal square
// roots (attn::attn_sample's GUARDED), launched when eps < FLT_MIN.
#include <cfloat>

#include "az_nn.h"
#include "nn_attn_core.h"

namespace {

using namespace attn;

template <bool GUARDED>
__global__ void __launch_bounds__(256, 3) k_attn_block(const uint16_t *x, const uint16_t *pre_w, const uint16_t *qkvg,
                                                       const uint16_t *qn_w, const uint16_t *kn_w, const uint16_t *o_w,
                                                       uint16_t *y, int64_t B, float eps, const int64_t *batch_dev)
{
    if (batch_dev != nullptr && *batch_dev < B) B = *batch_dev;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;

    __shared__ V8 s_w32[W32_N];
    __shared__ V4 s_w16[W16_N];
    __shared__ __align__(16) float s_gate[4 * GATE_N];     // [wave][GATE_N]
    __shared__ float s_pw[C];
    __shared__ float s_qk[2 * HD];
    stage_weights(qkvg, o_w, pre_w, qn_w, kn_w, s_w32, s_w16, s_pw, s_qk);
    __syncthreads();
    const bool bounded = scores_bounded(s_qk, l4);

    const int64_t stride = static_cast<int64_t>(gridDim.x) * 4;
    for (int64_t b = static_cast<int64_t>(blockIdx.x) * 4 + wave; b < B; b += stride) {
        const uint16_t *xs = x + b * (CELLS * C);
        f32x4 out[4][TT];
        attn_sample<GUARDED>(xs, s_w32, s_w16, s_pw, s_qk, s_gate + wave * GATE_N, bounded, eps, lane, l15, l4, out);

        // ---- y = out + x : lane holds 4 consecutive output channels of token qt*16 + lane&15
        uint16_t *ys = y + b * (CELLS * C);
#pragma unroll
        for (int qt = 0; qt < TT; ++qt) {
            const int tok = qt * 16 + l15;
            if (tok < CELLS) {
#pragma unroll
                for (int ot = 0; ot < 4; ++ot) {
                    const int ch = ot * 16 + 4 * l4;
                    const V4 xr = *reinterpret_cast<const V4 *>(xs + tok * C + ch);
                    V4 o;
                    o.w[0] = pack2(out[ot][qt][0] + bf_lo(xr.w[0]), out[ot][qt][1] + bf_hi(xr.w[0]));
                    o.w[1] = pack2(out[ot][qt][2] + bf_lo(xr.w[1]), out[ot][qt][3] + bf_hi(xr.w[1]));
                    *reinterpret_cast<V4 *>(ys + tok * C + ch) = o;
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int az_nn_attn_block(const void *x, const void *prenorm_w, const void *qkvg_w, const void *q_norm_w,
                     const void *k_norm_w, const void *o_w, void *y, int64_t batch, float eps, const int64_t *batch_dev,
                     void *stream)
{
    if (batch <= 0) return 1;
    const int64_t wgs = (batch + 3) / 4;
    const unsigned cap = 256u * 3u * 2u;       // two rounds of resident workgroups
    const unsigned grid = static_cast<unsigned>(wgs < cap ? wgs : cap);
    // the default form takes its reciprocal square roots bare (rsq_normal): a smaller eps goes to the form that guards them
    const auto kern = !(eps >= FLT_MIN) ? k_attn_block<true> : k_attn_block<false>;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(x), static_cast<const uint16_t *>(prenorm_w),
                       static_cast<const uint16_t *>(qkvg_w), static_cast<const uint16_t *>(q_norm_w),
                       static_cast<const uint16_t *>(k_norm_w), static_cast<const uint16_t *>(o_w),
                       static_cast<uint16_t *>(y), batch, eps, batch_dev);
    return 0;
}

}  // extern "C"
