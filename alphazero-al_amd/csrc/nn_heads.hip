// nn_heads.hip - both output heads of the evaluator as ONE kernel: final tokens in, the three
// arrays the tree backup consumes out (what the heads compute, and the pair tail: nn_heads_core.h).
//
// One wavefront walks a grid-stride list of sample PAIRS; the next sample's tokens are in flight
// while the current one is reduced.  This file holds the token pass from HBM - 8 lanes per token,
// packed-f32 arithmetic (two elements per VALU instruction) with DPP reductions; the policy pooling
// and everything on the pair's 16-column B operand are shared with the fused kernel of
// nn_attn_heads.hip (this kernel runs the value tail per pair, on columns 7 and 15).  A lone
// vector on a 16-wide tile wastes most of that MFMA and is still ~10x cheaper than the 64 LDS
// reads + 64 FMAs per lane of a VALU matvec.  The kernel is VALU-issue bound (profiles/): the
// first version spent 2.3 k vector instructions per sample, this one ~0.75 k.
// HBM traffic: read tokens (5376 B per sample), write 11 floats.  Replaces az_nn_heads_prep
// + ~25 small PyTorch kernels (0.33 ms per 32768-leaf iteration in profiles/r01).
#include "az_nn.h"
#include "nn_heads_core.h"

namespace {

using namespace heads;

constexpr int WPB = 4;          // wavefronts per workgroup, each on its own sample pairs
constexpr int VS = 72;          // bf16 row stride of the B-operand buffer: 144 B keeps b128 reads conflict-free

__device__ __forceinline__ uint16_t to_bf16(float a)
{
    const __hip_bfloat16 x = __float2bfloat16(a);
    return *reinterpret_cast<const uint16_t *>(&x);
}

__device__ __forceinline__ void load_tokens(V8 (&v)[6], const uint16_t *xs, int sub, int vec)
{
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int t = sub + 8 * k;
        V8 z; z.w[0] = z.w[1] = z.w[2] = z.w[3] = 0;
        v[k] = t < CELLS ? *reinterpret_cast<const V8 *>(xs + t * C + vec * 8) : z;
    }
}

// dynamic LDS layout (bytes)
constexpr int L_A = 0;                                   // V8 [26*64]: A fragments
constexpr int L_C = L_A + A_N * 16;                       // float [K_TAIL_N][64]: per-channel constants
constexpr int L_PN = L_C + K_TAIL_N * C * 4;             // per wave: V8 [42*8] normalised tokens (bf16)
constexpr int L_VEC = L_PN + WPB * CELLS * C * 2;        // per wave: u16 [16*VS] B operand, row n = column n of V^T
constexpr int L_PART = L_VEC + WPB * 16 * VS * 2;        // per wave: float [8][64] channel sums of the 8 token slots
constexpr int L_SCORE = L_PART + WPB * 8 * C * 4;        // per wave: float [48] row-gate scores, then weights
constexpr int L_MEAN = L_SCORE + WPB * 48 * 4;           // per wave: float [2][64] token means of the pair
constexpr int L_TOTAL = L_MEAN + WPB * 2 * C * 4;

__global__ void __launch_bounds__(64 * WPB) k_heads(const uint16_t *tok, az_nn_heads_weights w, const uint8_t *mask,
                                                    float *probs, float *wdl, float *moves_left, int64_t B, float eps,
                                                    const int32_t *scatter, const int64_t *batch_dev)
{
    const int64_t rows_total = B;                 // rows of mask / outputs: a compact list may name any of them
    if (batch_dev != nullptr && *batch_dev < B) B = *batch_dev;
    extern __shared__ __align__(16) uint8_t smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int sub = lane >> 3, vec = lane & 7;
    V8 *s_a = reinterpret_cast<V8 *>(smem + L_A);
    float (*s_c)[C] = reinterpret_cast<float (*)[C]>(smem + L_C);
    V8 *s_pn = reinterpret_cast<V8 *>(smem + L_PN + wave * CELLS * C * 2);
    uint16_t *s_vec = reinterpret_cast<uint16_t *>(smem + L_VEC + wave * 16 * VS * 2);
    float *s_part = reinterpret_cast<float *>(smem + L_PART + wave * 8 * C * 4);
    float *s_score = reinterpret_cast<float *>(smem + L_SCORE + wave * 48 * 4);
    float *s_mean = reinterpret_cast<float *>(smem + L_MEAN + wave * 2 * C * 4);

    stage_weights(w, s_a, s_c);
    for (int i = lane; i < 16 * VS; i += 64) s_vec[i] = 0;
    __syncthreads();

    // policy-norm weight and norm x row-gate weight of this lane's 8 channels
    f32x2 nw2[4], ngw2[4];
    {
        const V8 a = *reinterpret_cast<const V8 *>(static_cast<const uint16_t *>(w.p_norm) + vec * 8);
        const V8 g = *reinterpret_cast<const V8 *>(static_cast<const uint16_t *>(w.p_gate_w) + vec * 8);
#pragma unroll
        for (int q = 0; q < 4; ++q) { nw2[q] = unpack2(a.w[q]); ngw2[q] = nw2[q] * unpack2(g.w[q]); }
    }
    const float dpool_norm = s_c[K_DPOOL_NORM][lane];

    const int64_t npairs = (B + 1) / 2;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * WPB;
    int64_t pr = static_cast<int64_t>(blockIdx.x) * WPB + wave;
    V8 cur[6];
    if (pr < npairs) load_tokens(cur, tok + (2 * pr) * (CELLS * C), sub, vec);
    for (; pr < npairs; pr += stride) {
#pragma unroll 1
        for (int h = 0; h < 2; ++h) {
            // the sample after this one: second of the pair, or the first of this wave's next pair
            int64_t nb = h == 0 ? 2 * pr + 1 : 2 * (pr + stride);
            if (nb >= B) nb = 2 * pr;                                  // loaded and never used
            V8 nxt[6];
            load_tokens(nxt, tok + nb * (CELLS * C), sub, vec);

            // ---- pass over the tokens: RMS statistics, row-gate score, channel sums, normalised tokens
            f32x2 msum[4] = {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}};
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const int t = sub + 8 * k;
                f32x2 f[4], ss2 = {0.f, 0.f}, sc2 = {0.f, 0.f};
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    f[q] = unpack2(cur[k].w[q]);
                    ss2 = __builtin_elementwise_fma(f[q], f[q], ss2);
                    sc2 = __builtin_elementwise_fma(f[q], ngw2[q], sc2);
                    msum[q] += f[q];
                }
                const float ss = sum8(ss2.x + ss2.y), sc = sum8(sc2.x + sc2.y);
                const float r = rsqrtf(ss * (1.0f / C) + eps);
                if (t < CELLS) {
                    V8 o;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const f32x2 pn = f[q] * f32x2{r, r} * nw2[q];
                        o.w[q] = pack2(pn.x, pn.y);
                    }
                    s_pn[t * 8 + vec] = o;
                    if (vec == 0) s_score[t] = sc * r + w.p_gate_b;
                }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) *reinterpret_cast<f32x2 *>(&s_part[sub * C + vec * 8 + 2 * q]) = msum[q];
            wave_lds_sync();

            // ---- token mean (bf16, like the reference's mean of a bf16 tensor), lane = channel:
            // kept for the residual, and its pool_norm goes to this sample's value column
            {
                float m = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) m += s_part[j * C + lane];
                const f32x2 g0 = rbf2(f32x2{m * (1.0f / CELLS), 0.0f});
                const float r = rsqrtf(wave_sum(g0.x * g0.x) * (1.0f / C) + eps);
                s_mean[h * C + lane] = g0.x;
                s_vec[(8 * h + 7) * VS + lane] = to_bf16(g0.x * r * dpool_norm);
            }
            pool_columns<VS>(s_score, s_pn, s_vec, h, lane);
#pragma unroll
            for (int k = 0; k < 6; ++k) cur[k] = nxt[k];
        }
        heads_pair_tail<VS>(s_a, s_c, s_vec, s_mean, w, mask, probs, wdl, moves_left, 2 * pr, 2 * pr + 1, B, rows_total,
                            scatter, eps, lane, l15, l4);
    }
}

}  // namespace

extern "C" int az_nn_heads(const void *tokens, const az_nn_heads_weights *w, const uint8_t *mask, float *probs,
                           float *wdl, float *moves_left, int64_t batch, float eps, const int32_t *scatter,
                           const int64_t *batch_dev, void *stream)
{
    if (batch <= 0 || w == nullptr || tokens == nullptr || probs == nullptr || wdl == nullptr || moves_left == nullptr) return 1;
    static DeviceSetup setup;
    if (setup.cus({reinterpret_cast<const void *>(k_heads)}, L_TOTAL) == 0) return 2;
    // 70 KB of LDS per workgroup: two workgroups (8 wavefronts) per CU, each walking its sample pairs
    const int64_t want = ((batch + 1) / 2 + WPB - 1) / WPB;
    const unsigned grid = static_cast<unsigned>(want < 512 ? want : 512);
    hipLaunchKernelGGL(k_heads, dim3(grid), dim3(64 * WPB), L_TOTAL, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(tokens), *w, mask, probs, wdl, moves_left, batch, eps, scatter, batch_dev);
    return 0;
}
