// nn_heads_core.h - what the two kernels that end the evaluator share after their token passes: k_heads
// (nn_heads.hip: tokens from HBM) and k_attn_heads (nn_attn_heads.hip: tokens from the attention's registers).
//
//   policy  (Network.py:96-118):  pn = RMSNorm(tokens); per column, softmax over its 6 rows of
//           row_gate(pn) pools the column's tokens; logits = out(silu(fc(col))); masked softmax
//   value / moves left (Network.py:121-141):  x = mean(tokens); x += silu(pool_fc(norm(x)));
//           h = out_norm(silu(fc(norm(x)))); wdl = softmax(value_out(h)); ml = 42*sigmoid(aux_out(h))
//
// A token pass (the kernel's own) leaves, per wavefront and sample hs of a pair, the normalised tokens s_pn and the
// row-gate scores s_score in LDS.  pool_columns() fills columns 8 hs .. 8 hs + 6 of a 16-column B operand;
// policy_tail() runs the policy's 64x64 linear on the matrix cores in the orientation out^T = W . V^T for both samples
// at once (A = a weight fragment, B = the 16 columns) and the masked softmax of each sample's seven logits.
//
// value_tail() is the value / moves-left head of up to 16 columns at once: every live column of the B operand holds
// pool_norm(token mean) of one sample, and three stages (pool_fc + residual + norm, fc + out_norm, the two outputs) run
// on all of them, each lane on the column it holds in the MFMA C layout.  MFMA columns are independent and col_sum stays
// inside a column, so a sample's outputs do not depend on the column it sits in nor on what the other columns hold.
// The callers differ in which columns are live:
//   per pair (k_heads): columns 7 and 15 of the pair's B operand, next to the policy columns; the token pass leaves
//       the mean in s_mean[hs] and its pool_norm in column 8 hs + 7;
//   deferred (k_attn_heads): the token pass only parks the bf16 token mean in one of 16 slots; once per 16 samples (and
//       after the last one) the wavefront fills ALL 16 columns with value vectors and runs the three stages once, where
//       the per-pair form runs them eight times for the same samples.
// Rounding points (bf16 after every normalisation / linear / activation) are those of the reference under bf16
// autocast, except that the row gate sees the normalised tokens before their rounding.
#pragma once

#include "az_nn.h"
#include "nn_common.h"

namespace {

namespace heads {

constexpr int CELLS = 42, ROWS = 6, COLS = 7, C = 64;
constexpr int A_N = 26 * 64;        // V8 A fragments (fragment f, lane l -> 16 bytes at f*64+l): policy fc 0-7, pool_fc 8-15,
                                    // fc 16-23 as [m tile][k step]; 24-25 = rows {value_out 0-2, aux_out} x k step
// per-channel constants in LDS, float [K_..][64].  The first K_TAIL_N are staged by stage_weights(); the policy norm
// weight and norm x row-gate weight belong to the token pass (k_heads keeps them in registers).
enum { K_PFC_B, K_POUT_W, K_DPOOL_B, K_DNORM, K_DFC_B, K_DOUT_NORM, K_DVAL_B, K_DPOOL_NORM, K_TAIL_N, K_PNORM = K_TAIL_N, K_PNGW, K_N };

// A fragment f of lane (r = lane & 15, q = lane >> 4), straight from the weights
__device__ __forceinline__ V8 load_afrag(const az_nn_heads_weights &w, int f, int r, int q)
{
    V8 v; v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
    if (f < 24) {
        const int m = (f >> 1) & 3, ks = f & 1;
        const void *mat = f < 8 ? w.p_fc_w : (f < 16 ? w.d_pool_w : w.d_fc_w);
        v = *reinterpret_cast<const V8 *>(static_cast<const uint16_t *>(mat) + (16 * m + r) * C + 32 * ks + 8 * q);
    } else if (r < 3) {
        v = *reinterpret_cast<const V8 *>(static_cast<const uint16_t *>(w.d_val_w) + r * C + 32 * (f & 1) + 8 * q);
    } else if (r == 3) {
        v = *reinterpret_cast<const V8 *>(static_cast<const uint16_t *>(w.d_aux_w) + 32 * (f & 1) + 8 * q);
    }
    return v;
}
// where value_tail() takes its A fragments (8-25) from: the staged copy, or the weights themselves (L2) - for a caller
// that runs it once per 16 samples and has better uses for 18 KB of LDS
struct AFragLds {
    const V8 *s_a;
    int lane;
    __device__ __forceinline__ bf16x8 operator()(int f) const { return as_bf16x8(s_a[f * 64 + lane]); }
};
struct AFragGlobal {
    const az_nn_heads_weights &w;
    int l15, l4;
    __device__ __forceinline__ bf16x8 operator()(int f) const { return as_bf16x8(load_afrag(w, f, l15, l4)); }
};

// once per workgroup; the caller's __syncthreads() follows.  FRAGS: 26, or 8 (the policy's only)
template <int FRAGS = 26>
__device__ __forceinline__ void stage_weights(const az_nn_heads_weights &w, V8 *s_a, float (*s_c)[C])
{
    for (int i = threadIdx.x; i < FRAGS * 64; i += blockDim.x) s_a[i] = load_afrag(w, i >> 6, i & 15, (i & 63) >> 4);
    if (threadIdx.x < C) {
        const int i = threadIdx.x;
        s_c[K_PFC_B][i] = bf1(static_cast<const uint16_t *>(w.p_fc_b) + i);
        s_c[K_POUT_W][i] = bf1(static_cast<const uint16_t *>(w.p_out_w) + i);
        s_c[K_DPOOL_B][i] = bf1(static_cast<const uint16_t *>(w.d_pool_b) + i);
        s_c[K_DNORM][i] = bf1(static_cast<const uint16_t *>(w.d_norm) + i);
        s_c[K_DFC_B][i] = bf1(static_cast<const uint16_t *>(w.d_fc_b) + i);
        s_c[K_DOUT_NORM][i] = bf1(static_cast<const uint16_t *>(w.d_out_norm) + i);
        s_c[K_DVAL_B][i] = i < 3 ? bf1(static_cast<const uint16_t *>(w.d_val_b) + i) : 0.0f;
        s_c[K_DPOOL_NORM][i] = bf1(static_cast<const uint16_t *>(w.d_pool_norm) + i);
    }
}

// Policy pooling of sample hs of the pair: softmax of the row-gate scores over the 6 rows of each column, then the
// weighted column sums of the normalised tokens into columns 8 hs .. 8 hs + 6 of the B operand (row stride VS bf16).
// After the token pass's wave_lds_sync(); ends with one.
template <int VS>
__device__ __forceinline__ void pool_columns(float *s_score, const void *s_pn, uint16_t *s_vec, int hs, int lane)
{
    // ---- softmax over the 6 rows of each column: lane t owns token t's pooling weight
    if (lane < CELLS) {
        const int c = lane % COLS;
        float sc[ROWS], mx = -INFINITY, den = 0.0f;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) { sc[r] = s_score[r * COLS + c]; mx = fmaxf(mx, sc[r]); }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) den += fast_exp(sc[r] - mx);
        const float wt = fast_exp(s_score[lane] - mx) * __builtin_amdgcn_rcpf(den);
        wave_lds_sync();                                       // every lane has read the scores
        s_score[lane] = rbf2(f32x2{wt, 0.0f}).x;
    } else {
        wave_lds_sync();
    }
    wave_lds_sync();
    // ---- weighted column sums: lane = (channel pair, half of the columns), packed f32
    {
        const uint32_t *pn2 = static_cast<const uint32_t *>(s_pn);
        const int cp = lane & 31, c0 = (lane >> 5) * 4;       // columns c0 .. c0+3 (the 8th does not exist)
#pragma unroll
        for (int cc = 0; cc < 4; ++cc) {
            const int c = c0 + cc;
            if (c < COLS) {
                f32x2 acc = {0.0f, 0.0f};
#pragma unroll
                for (int r = 0; r < ROWS; ++r) {
                    const float wt = s_score[r * COLS + c];
                    acc = __builtin_elementwise_fma(f32x2{wt, wt}, unpack2(pn2[(r * COLS + c) * (C / 2) + cp]), acc);
                }
                *reinterpret_cast<uint32_t *>(&s_vec[(8 * hs + c) * VS + 2 * cp]) = pack2(acc.x, acc.y);
            }
        }
    }
    wave_lds_sync();
}

// The policy of both samples of a pair, b0 and b1 (b1 >= B: a half-empty pair): columns 0-6 and 8-14 of the B operand.
// Compact batch: sample b stands for row scatter[b] of the mask and of the outputs; an index outside the rows (a list
// longer than what was written) is dropped, never dereferenced.
// policy_tail_at(): the same for a caller that already holds, per lane, its column's output row b, whether that row is
// written (real) and whether the column is masked out (a real row whose mask byte is 0) - k_attn_heads requests the
// row index and the mask byte a sample ahead, so that the tail waits for neither.
template <int VS>
__device__ __forceinline__ void policy_tail_at(const V8 *s_a, const float (*s_c)[C], const uint16_t *s_vec,
                                               const az_nn_heads_weights &w, float *probs, int64_t b, bool real, bool masked,
                                               int lane, int l15, int l4)
{
    auto afrag = [&](int f) { return as_bf16x8(s_a[f * 64 + lane]); };
    auto bfrag = [&](int ks) { return as_bf16x8(*reinterpret_cast<const V8 *>(&s_vec[l15 * VS + 32 * ks + 8 * l4])); };
    auto cvec2 = [&](int which, int m, int h) { return *reinterpret_cast<const f32x2 *>(&s_c[which][16 * m + 4 * l4 + 2 * h]); };
    const bool live = (l15 & 7) != 7;          // columns 7 and 15 are no policy columns
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 ap[4];
    {
        const bf16x8 v0 = bfrag(0), v1 = bfrag(1);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            ap[m] = MFMA32(afrag(2 * m), v0, zero);
            ap[m] = MFMA32(afrag(2 * m + 1), v1, ap[m]);
        }
    }
    // logit[c] = out . silu(fc(col_c) + b), masked softmax over the 7 columns of a sample
    f32x2 part2 = {0.0f, 0.0f};
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
            const f32x2 xv = rbf2(f32x2{ap[m][2 * hh], ap[m][2 * hh + 1]} + cvec2(K_PFC_B, m, hh));
            part2 = __builtin_elementwise_fma(rbf2(silu2(xv)), cvec2(K_POUT_W, m, hh), part2);
        }
    float logit = col_sum(part2.x + part2.y) + w.p_out_b;
    if (live && masked) logit = -1e9f;
    if (!live) logit = -INFINITY;
    const float mx = max8(logit);
    const float e = live ? fast_exp(logit - mx) : 0.0f;
    const float den = sum8(e);
    if (live && real && l4 == 0) probs[b * COLS + (l15 & 7)] = e * __builtin_amdgcn_rcpf(den);
    wave_lds_sync();
}
template <int VS>
__device__ __forceinline__ void policy_tail(const V8 *s_a, const float (*s_c)[C], const uint16_t *s_vec,
                                            const az_nn_heads_weights &w, const uint8_t *mask, float *probs, int64_t b0,
                                            int64_t b1, int64_t B, int64_t rows_total, const int32_t *scatter, int lane,
                                            int l15, int l4)
{
    const int64_t bc = (l15 >> 3) == 0 ? b0 : b1;       // the sample this lane's column belongs to
    const int64_t b = (bc < B && scatter != nullptr) ? scatter[bc] : bc;
    const bool real = bc < B && b >= 0 && b < rows_total;
    const bool masked = (l15 & 7) != 7 && real && mask != nullptr && mask[b * COLS + (l15 & 7)] == 0;
    policy_tail_at<VS>(s_a, s_c, s_vec, w, probs, b, real, masked, lane, l15, l4);
}

// The value / moves-left head of the live columns of the B operand (row l15 of s_vec = pool_norm(mean) of the sample
// of column l15).  Per lane: col_live - its column holds a sample; b, real - that sample's output row and whether it is
// written; mean2(m, hh) - the sample's token mean, channels 16 m + 4 l4 + 2 hh, + 1.  afrag: AFragLds or AFragGlobal.
// After a wave_lds_sync(); ends with one.  BARE_RSQ: the two reciprocal square roots as rsq_normal(), for a caller
// launched with eps >= FLT_MIN only.
template <int VS, bool BARE_RSQ = false, class AFrag, class Mean>
__device__ __forceinline__ void value_tail(const AFrag &afrag, const float (*s_c)[C], uint16_t *s_vec, const Mean &mean2,
                                           const az_nn_heads_weights &w, float *wdl, float *moves_left, bool col_live,
                                           int64_t b, bool real, float eps, int l15, int l4)
{
    auto bfrag = [&](int ks) { return as_bf16x8(*reinterpret_cast<const V8 *>(&s_vec[l15 * VS + 32 * ks + 8 * l4])); };
    auto cvec2 = [&](int which, int m, int h) { return *reinterpret_cast<const f32x2 *>(&s_c[which][16 * m + 4 * l4 + 2 * h]); };
    // a live lane's 16 accumulator values (channel 16m+4*l4+reg) -> its own B-operand row
    auto put_col = [&](const f32x2 (&v)[4][2]) {
        if (col_live) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                uint32_t *p = reinterpret_cast<uint32_t *>(&s_vec[l15 * VS + 16 * m + 4 * l4]);
                p[0] = pack2(v[m][0].x, v[m][0].y);
                p[1] = pack2(v[m][1].x, v[m][1].y);
            }
        }
    };
    auto rsq = [](float v) {
        if constexpr (BARE_RSQ) return rsq_normal(v);
        else return rsqrtf(v);
    };
    const f32x4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    // stage 1: g = mean + silu(pool_fc(pool_norm(mean)) + b); n2 = norm(g)
    f32x2 g[4][2];
    {
        const bf16x8 v0 = bfrag(0), v1 = bfrag(1);
        f32x2 ss2 = {0.0f, 0.0f};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            f32x4 ad = MFMA32(afrag(8 + 2 * m), v0, zero);
            ad = MFMA32(afrag(8 + 2 * m + 1), v1, ad);
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const f32x2 xv = rbf2(f32x2{ad[2 * hh], ad[2 * hh + 1]} + cvec2(K_DPOOL_B, m, hh));
                g[m][hh] = rbf2(mean2(m, hh) + rbf2(silu2(xv)));
                ss2 = __builtin_elementwise_fma(g[m][hh], g[m][hh], ss2);
            }
        }
        const float rn = rsq(col_sum(ss2.x + ss2.y) * (1.0f / C) + eps);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) g[m][hh] = g[m][hh] * f32x2{rn, rn} * cvec2(K_DNORM, m, hh);
    }
    wave_lds_sync();
    put_col(g);
    wave_lds_sync();
    // stage 2: h = out_norm(silu(fc(n2) + b))
    {
        const bf16x8 v0 = bfrag(0), v1 = bfrag(1);
        f32x2 ss2 = {0.0f, 0.0f};
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            f32x4 acc = MFMA32(afrag(16 + 2 * m), v0, zero);
            acc = MFMA32(afrag(16 + 2 * m + 1), v1, acc);
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const f32x2 xv = rbf2(f32x2{acc[2 * hh], acc[2 * hh + 1]} + cvec2(K_DFC_B, m, hh));
                g[m][hh] = rbf2(silu2(xv));
                ss2 = __builtin_elementwise_fma(g[m][hh], g[m][hh], ss2);
            }
        }
        const float rn = rsq(col_sum(ss2.x + ss2.y) * (1.0f / C) + eps);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) g[m][hh] = g[m][hh] * f32x2{rn, rn} * cvec2(K_DOUT_NORM, m, hh);
    }
    wave_lds_sync();
    put_col(g);
    wave_lds_sync();
    // stage 3: rows 0-2 = value logits, row 3 = moves-left logit, in the live lanes with l4 == 0
    {
        f32x4 acc = MFMA32(afrag(24), bfrag(0), zero);
        acc = MFMA32(afrag(25), bfrag(1), acc);
        if (col_live && l4 == 0 && real) {
            const f32x2 v01 = rbf2(f32x2{acc[0] + s_c[K_DVAL_B][0], acc[1] + s_c[K_DVAL_B][1]});
            const float v2 = rbf2(f32x2{acc[2] + s_c[K_DVAL_B][2], 0.0f}).x;
            const float mx = fmaxf(v01.x, fmaxf(v01.y, v2));
            const float e0 = fast_exp(v01.x - mx), e1 = fast_exp(v01.y - mx), e2 = fast_exp(v2 - mx);
            const float inv = 1.0f / (e0 + e1 + e2);
            wdl[b * 3 + 0] = e0 * inv;
            wdl[b * 3 + 1] = e1 * inv;
            wdl[b * 3 + 2] = e2 * inv;
            moves_left[b] = w.aux_scale / (1.0f + fast_exp(-(acc[3] + w.d_aux_b)));
        }
    }
    wave_lds_sync();
}

// policy_tail() and value_tail() of a pair whose value vectors sit in columns 7 and 15 (means in s_mean[2][64])
template <int VS>
__device__ __forceinline__ void heads_pair_tail(const V8 *s_a, const float (*s_c)[C], uint16_t *s_vec, const float *s_mean,
                                          const az_nn_heads_weights &w, const uint8_t *mask, float *probs, float *wdl,
                                          float *moves_left, int64_t b0, int64_t b1, int64_t B, int64_t rows_total,
                                          const int32_t *scatter, float eps, int lane, int l15, int l4)
{
    policy_tail<VS>(s_a, s_c, s_vec, w, mask, probs, b0, b1, B, rows_total, scatter, lane, l15, l4);
    const int half = l15 >> 3;
    const int64_t bc = half == 0 ? b0 : b1;
    const int64_t b = (bc < B && scatter != nullptr) ? scatter[bc] : bc;
    const bool real = bc < B && b >= 0 && b < rows_total;
    auto mean2 = [&](int m, int hh) { return *reinterpret_cast<const f32x2 *>(&s_mean[half * C + 16 * m + 4 * l4 + 2 * hh]); };
    value_tail<VS>(AFragLds{s_a, lane}, s_c, s_vec, mean2, w, wdl, moves_left, (l15 & 7) == 7, b, real, eps, l15, l4);
}

}  // namespace heads

}  // namespace
