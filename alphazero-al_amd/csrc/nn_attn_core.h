// nn_attn_core.h - the evaluator's gated attention of ONE sample by ONE wavefront, shared by k_attn_block
// (nn_attn.hip: y = bf16(x + out) goes to HBM) and k_attn_heads (nn_attn_heads.hip: the output heads follow in
// registers).
//
//   out = o_proj( sigmoid(gate) * softmax(q_norm(Q) k_norm(K)^T / sqrt(16)) V )
//   with [Q | K | V | gate] = qkvg_proj(RMSNorm(x))                     (Network.py:51-93)
//
// The wavefront keeps every intermediate in registers (42 tokens padded to 3 row tiles of 16).  The point of the
// design is the ORIENTATION of each product: with C/D in the MFMA layout (column = lane & 15, rows =
// 4*(lane>>4)+reg) a result can feed the next MFMA with no lane movement if that product sums over its ROW index.  So
//
//   Q^T, K^T, gate^T = W . H^T      (features x tokens; A = weights, B = H^T)   v_mfma 16x16x32
//   V               = H . Wv^T      (tokens x features; A = H, B = Wv^T)        v_mfma 16x16x32
//   S^T             = K . Q^T       (keys x queries;  A = K^T regs, B = Q^T regs) 16x16x16
//   O^T             = V^T . P^T     (d x queries;     A = V regs,   B = P^T regs) 16x16x16
//   out^T           = Wo_h . O_h^T  summed over heads (A = weights, B = O^T regs) 16x16x16
//
// The per-(token, head) RMSNorm of q and k and the softmax over keys reduce over rows, i.e. over the 4 registers of a
// lane and the 4 lane groups that share a column (col_sum / col_max).  H fragments serve both as B operand (H^T) and
// as A operand (H): the element sets coincide.  The weights (26 KB + 8 KB) sit in LDS in operand-fragment order; what
// a wavefront would otherwise hold across a whole sample - the sigmoid gates of every (token, head), the pre-norm
// weight, the q / k norm weights - lives in LDS too (36 registers: three wavefronts then share a SIMD).
//
// The gate tile has 4 distinct rows (one per head) on a 16-row MFMA.  Staged as row 4 g + r = head g, lane group g
// ends up with head g of its token in every accumulator register: it computes ONE sigmoid and stores one float, and
// the head loop reads gate (token tile, head h, token l15) from the slot lane group h wrote.
#pragma once

#include "nn_common.h"

namespace {

namespace attn {

constexpr int CELLS = 42, C = 64, HEADS = 4, HD = 16, TT = 3;     // 3 token tiles of 16
constexpr int W32_N = (3 * HEADS * 2 + 2) * 64;                    // V8: wq, wk, wv [h][s], wg [s]
constexpr int W16_N = 4 * HEADS * 64;                              // V4: wo [ot][h]
constexpr int GATE_N = TT * 64;                                    // per wavefront: float [token tile][head][token]
constexpr float QSCALE = 0.25f * 1.44269504f;     // 1/sqrt(16) of the scores and log2(e) of their softmax ride on q

// The weights, staged once per workgroup into LDS in exactly the order the lanes read them (fragment f, lane l ->
// 16 or 8 contiguous bytes at f*64+l), so every operand fetch is one conflict-free ds_read.  The caller's
// __syncthreads() follows.  qkvg: (196, 64) row-major [out][in]: rows 0-63 Q, 64-127 K, 128-191 V, 192-195 gate.
// s_pw [64]: pre-norm weight; s_qk [32]: q norm weight x QSCALE, k norm weight.
__device__ __forceinline__ void stage_weights(const uint16_t *qkvg, const uint16_t *o_w, const uint16_t *pre_w,
                                              const uint16_t *qn_w, const uint16_t *kn_w, V8 *s_w32, V4 *s_w16, float *s_pw,
                                              float *s_qk)
{
    for (int i = threadIdx.x; i < W32_N; i += blockDim.x) {
        const int f = i >> 6, l = i & 63, ll15 = l & 15, ll4 = l >> 4;
        V8 v;
        if (f < 3 * HEADS * 2) {
            const int part = f / (HEADS * 2), h = (f >> 1) % HEADS, sk = f & 1;
            v = *reinterpret_cast<const V8 *>(qkvg + (part * C + h * HD + ll15) * C + 32 * sk + 8 * ll4);
        } else {
            // the 4 gate rows over the tile's 16 rows: row 4 g + r = head g, so every accumulator register of lane
            // group g is head g of the lane's token
            v = *reinterpret_cast<const V8 *>(qkvg + (3 * C + (ll15 >> 2)) * C + 32 * (f & 1) + 8 * ll4);
        }
        s_w32[i] = v;
    }
    for (int i = threadIdx.x; i < W16_N; i += blockDim.x) {
        const int f = i >> 6, l = i & 63, ot = f / HEADS, h = f % HEADS;
        s_w16[i] = *reinterpret_cast<const V4 *>(o_w + (ot * 16 + (l & 15)) * C + h * HD + 4 * (l >> 4));
    }
    if (threadIdx.x < C) s_pw[threadIdx.x] = bf1(pre_w + threadIdx.x);
    if (threadIdx.x < HD) {
        s_qk[threadIdx.x] = bf1(qn_w + threadIdx.x) * QSCALE;
        s_qk[HD + threadIdx.x] = bf1(kn_w + threadIdx.x);
    }
}

// |score| <= 16 max|q_norm w| max|k_norm w| in log2 units (q and k are RMS-normalised): when that is far from fp32's
// exp2 range the softmax needs no running maximum.  After the staging's barrier; uniform over the wavefront.
__device__ __forceinline__ bool scores_bounded(const float *s_qk, int l4)
{
    float mq = 0.0f, mk = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        mq = fmaxf(mq, fabsf(s_qk[4 * l4 + r]));
        mk = fmaxf(mk, fabsf(s_qk[HD + 4 * l4 + r]));
    }
    col_max2(mq, mk);
    return 16.0f * mq * mk < 100.0f;
}

// One sample: xs = its 42 x 64 residual-stream rows (bf16), out = out^T in the MFMA C layout (lane holds channels
// 16 ot + 4 l4 + r of token qt*16 + l15).  s_gate: this wavefront's gate store (GATE_N floats), written and read here.
// GUARDED: the reciprocal square roots as rsqrtf(), which takes any eps, where the default takes rsq_normal().
template <bool GUARDED = false>
__device__ __forceinline__ void attn_sample(const uint16_t *xs, const V8 *s_w32, const V4 *s_w16, const float *s_pw,
                                            const float *s_qk, float *s_gate, bool bounded, float eps, int lane, int l15,
                                            int l4, f32x4 (&out)[4][TT])
{
    // (the head loop below is not unrolled and indexes these by the runtime head number, so the
    // reads stay ds_read_b128 / ds_read_b64 inside the loop instead of becoming live registers)
    auto frag32 = [&](int f) { return as_bf16x8(s_w32[f * 64 + lane]); };     // part*8 + h*2 + s ; gate: 24 + s
    auto frag16 = [&](int f) {
        union { V4 v; s16x4 s; } r;
        r.v = s_w16[f * 64 + lane];
        return r.s;
    };
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    // 1 / sqrt of an RMS statistic, sum / n + eps.  The default form is launched with eps >= FLT_MIN only (the host
    // entry points see to it), which is rsq_normal()'s precondition.
    auto rsq = [](float v) {
        if constexpr (GUARDED) return rsqrtf(v);
        else return rsq_normal(v);
    };

    // ---- H = RMSNorm(x) * w, as MFMA fragments (token = tile*16 + lane&15, 8 channels per k-step)
    // The sample's six row vectors are requested together and without a branch: a padding token reads row 41 and is
    // zeroed once the vector is in, so the first tile's statistics start when its two vectors have arrived while the
    // later tiles' are in flight - one memory latency per sample.
    V8 xv[TT][2];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        const int tok = tt * 16 + l15, row = tok < CELLS ? tok : CELLS - 1;
#pragma unroll
        for (int s = 0; s < 2; ++s) xv[tt][s] = *reinterpret_cast<const V8 *>(xs + row * C + 32 * s + 8 * l4);
    }
    bf16x8 hf[TT][2];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        const int tok = tt * 16 + l15;
        f32x2 f[2][4], ss2 = {0.0f, 0.0f};
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            V8 v;
#pragma unroll
            for (int i = 0; i < 4; ++i) v.w[i] = tok < CELLS ? xv[tt][s].w[i] : 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                f[s][i] = unpack2(v.w[i]);
                ss2 = __builtin_elementwise_fma(f[s][i], f[s][i], ss2);
            }
        }
        const float ss = col_sum(ss2.x + ss2.y);
        const float r = rsq(ss * (1.0f / C) + eps);
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            V8 o;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const f32x2 hv = f[s][i] * f32x2{r, r} * *reinterpret_cast<const f32x2 *>(&s_pw[32 * s + 8 * l4 + 2 * i]);
                o.w[i] = pack2(hv.x, hv.y);
            }
            hf[tt][s] = as_bf16x8(o);
        }
    }
    // ---- sigmoid gates of every token: lane group l4 holds head l4
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        f32x4 g = MFMA32(frag32(24), hf[tt][0], zero);
        g = MFMA32(frag32(25), hf[tt][1], g);
        s_gate[tt * 64 + lane] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504f * g[0]));
    }
    wave_lds_sync();          // a gate is read by the lanes of other lane groups

#pragma unroll
    for (int ot = 0; ot < 4; ++ot)
#pragma unroll
        for (int qt = 0; qt < TT; ++qt) out[ot][qt] = zero;
    // ---- one head at a time: projection, attention, contribution to the output projection.
    // Not unrolled: the four heads share the code and, more importantly, the registers.
#pragma unroll 1
    for (int h = 0; h < HEADS; ++h) {
        s16x4 qb[TT], kb[TT], vb[TT];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
            f32x4 q = MFMA32(frag32(h * 2), hf[tt][0], zero);
            q = MFMA32(frag32(h * 2 + 1), hf[tt][1], q);
            f32x4 k = MFMA32(frag32(8 + h * 2), hf[tt][0], zero);
            k = MFMA32(frag32(8 + h * 2 + 1), hf[tt][1], k);
            f32x4 v = MFMA32(hf[tt][0], frag32(16 + h * 2), zero);
            v = MFMA32(hf[tt][1], frag32(16 + h * 2 + 1), v);
            // per-(token, head) RMSNorm over d: rows of the column this lane sits in
            f32x2 q2[2] = {{q[0], q[1]}, {q[2], q[3]}}, k2[2] = {{k[0], k[1]}, {k[2], k[3]}};
            const f32x2 qq = __builtin_elementwise_fma(q2[1], q2[1], q2[0] * q2[0]);
            const f32x2 kk = __builtin_elementwise_fma(k2[1], k2[1], k2[0] * k2[0]);
            float qs = qq.x + qq.y, ks = kk.x + kk.y;
            col_sum2(qs, ks);
            const float qr = rsq(qs * (1.0f / HD) + eps), kr = rsq(ks * (1.0f / HD) + eps);
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const f32x2 qw = *reinterpret_cast<const f32x2 *>(&s_qk[4 * l4 + 2 * r]);
                const f32x2 kw = *reinterpret_cast<const f32x2 *>(&s_qk[HD + 4 * l4 + 2 * r]);
                q2[r] = q2[r] * f32x2{qr, qr} * qw; k2[r] = k2[r] * f32x2{kr, kr} * kw;
            }
            qb[tt] = to_s16x4(f32x4{q2[0].x, q2[0].y, q2[1].x, q2[1].y});
            kb[tt] = to_s16x4(f32x4{k2[0].x, k2[0].y, k2[1].x, k2[1].y});
            vb[tt] = to_s16x4(v);
        }
        // E^T = exp2(S^T - max) of query tile qt against every key, as the bf16 B operands of the next product (S^T tile
        // rows = keys, column = query lane&15); returns this lane's share of the column's softmax denominator
        auto scores = [&](int qt, s16x4 (&pb)[TT]) {
            f32x4 st[TT];
            f32x2 den2 = {0.0f, 0.0f};
            if (bounded) {
                // No running maximum.  The six padding keys have k = 0, i.e. score 0 and weight exp2(0) = 1 exactly,
                // and their V rows are 0: they add nothing to the product and exactly 6 to the denominator.
#pragma unroll
                for (int kt = 0; kt < TT; ++kt) {
                    st[kt] = MFMA16(kb[kt], qb[qt], zero);      // already in log2 units (QSCALE)
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {
                        const f32x2 e = {__builtin_amdgcn_exp2f(st[kt][r]), __builtin_amdgcn_exp2f(st[kt][r + 1])};
                        st[kt][r] = e.x;
                        st[kt][r + 1] = e.y;
                        den2 += e;
                    }
                }
            } else {
                float m = -INFINITY;
#pragma unroll
                for (int kt = 0; kt < TT; ++kt) {
                    st[kt] = MFMA16(kb[kt], qb[qt], zero);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (kt == TT - 1 && kt * 16 + 4 * l4 + r >= CELLS) st[kt][r] = -INFINITY;   // padding keys
                        m = fmaxf(m, st[kt][r]);
                    }
                }
                m = col_max(m);
                const f32x2 nm = {-m, -m};
#pragma unroll
                for (int kt = 0; kt < TT; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; r += 2) {
                        const f32x2 d = f32x2{st[kt][r], st[kt][r + 1]} + nm;
                        const f32x2 e = {__builtin_amdgcn_exp2f(d.x), __builtin_amdgcn_exp2f(d.y)};
                        st[kt][r] = e.x;
                        st[kt][r + 1] = e.y;
                        den2 += e;
                    }
            }
#pragma unroll
            for (int kt = 0; kt < TT; ++kt) pb[kt] = to_s16x4(st[kt]);
            return den2.x + den2.y;
        };
        // O^T = (V^T . E^T) / den, gated, and its contribution to the output projection.  den: the column's sum of
        // scores()' shares; the bounded form counted the six padding keys into it.
        auto attend = [&](int qt, const s16x4 (&pb)[TT], float den) {
            if (bounded) den -= static_cast<float>(TT * 16 - CELLS);
            // normalise after the product: one scale per output element
            const float scale = __builtin_amdgcn_rcpf(den) * s_gate[qt * 64 + h * 16 + l15];
            f32x4 o = zero;                                  // O^T rows = d, column = query
#pragma unroll
            for (int kt = 0; kt < TT; ++kt) o = MFMA16(vb[kt], pb[kt], o);
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] *= scale;
            const s16x4 ob = to_s16x4(o);
#pragma unroll
            for (int ot = 0; ot < 4; ++ot) out[ot][qt] = MFMA16(frag16(ot * HEADS + h), ob, out[ot][qt]);
        };
        // the three query tiles' denominators are independent: tiles 0 and 1 share one set of swaps, and the
        // tiles' exp2 / add chains stand next to each other for the scheduler to interleave
        static_assert(TT == 3, "denominators paired as (0, 1), 2");
        s16x4 pb[TT][TT];
        float den[TT];
#pragma unroll
        for (int qt = 0; qt < TT; ++qt) den[qt] = scores(qt, pb[qt]);
        col_sum2(den[0], den[1]);
        den[2] = col_sum(den[2]);
#pragma unroll
        for (int qt = 0; qt < TT; ++qt) attend(qt, pb[qt], den[qt]);
    }
}

}  // namespace attn

}  // namespace
