// nn_attn_heads.hip - the gated attention block and both output heads as ONE kernel: residual stream in,
// the three arrays the tree backup consumes out, no token tensor in HBM.
//
// The attention phase is attn::attn_sample (nn_attn_core.h), the body k_attn_block runs: one wavefront per sample,
// every intermediate in registers.  It ends with out^T in the MFMA C layout - column = token (lane & 15), rows =
// channels - and that is the layout this kernel's token pass wants: the per-token RMS statistics and row-gate score are
// sums over a lane's 16 values plus col_sum, the token mean is a sum over the 16 lanes of a row (DPP).  The
// rounded output y = bf16(x + o_proj(...)) never leaves the registers; only the normalised tokens go to a
// per-wave LDS image, for the policy pooling over the 6 rows of each column (tokens 7 apart live in
// different lanes).  From there on the code is the one k_heads runs (nn_heads_core.h).  The POLICY runs per pair: a
// wavefront fills the 16-column B operand with the pooled columns of two samples (its own two consecutive samples of
// the grid-stride list) and runs the 64x64 linear and the masked softmax once per pair.  The VALUE / moves-left head is
// deferred: per sample only the bf16 token mean is parked in one of 16 slots of the wavefront; after its last sample
// (and whenever the 16 slots are full: more than 16 samples per wavefront, i.e. batches above 16 x 12 x CUs) the
// wavefront makes pool_norm(mean) of every slot one column of the B operand - in the MFMA C layout with column = slot a
// lane holds channels 16 ot + 4 l4 + r, the channel set the token pass had, so the statistics are summed in the same
// order - and runs value_tail() once on up to 16 live columns.  At a search iteration's ~26 k leaves that is one value
// tail per wavefront where the per-pair form ran four or five with 2 live columns of 16.  The value head's 18 A
// fragments are read from the weights (L2) in that one pass; their 18 KB of LDS hold the mean slots instead.
//
// k_attn_heads<true> (GUARDED) is the same kernel with rsqrtf() for every reciprocal square root where the default
// takes a bare v_rsq_f32 (rsq_normal), launched when eps < FLT_MIN.
//
// Rounding points are those of k_attn_block followed by k_heads: results differ from the two launches only
// through f32 summation order (token mean, RMS statistics) - the two token passes are the only code not shared.
//
// Shape: one 12-wavefront workgroup per CU (three per SIMD, the attention kernel's occupancy): one copy of
// the attention weights (35 KB) and of the policy's (10 KB), and 9.4 KB per wavefront (normalised tokens, which double
// as the attention's gate store, the B operand, scores and the 16 mean slots): 158 KB of LDS.
#include <cfloat>

#include "az_nn.h"
#include "nn_attn_core.h"
#include "nn_heads_core.h"

namespace {

using attn::TT;
using namespace heads;          // CELLS, C, ROWS, COLS, K_*

constexpr int WPB = 12;         // wavefronts per workgroup: one workgroup per CU
constexpr int VS = 64;          // bf16 row stride of the B-operand buffer

// dynamic LDS layout (bytes)
constexpr int A_FRAGS = 8;                                       // heads' A fragments kept in LDS: the policy's
constexpr int L_W32 = 0;                                         // V8 [attn::W32_N]
constexpr int L_W16 = L_W32 + attn::W32_N * 16;                  // V4 [attn::W16_N]
constexpr int L_A = L_W16 + attn::W16_N * 8;                     // V8 [A_FRAGS * 64]
constexpr int L_C = L_A + A_FRAGS * 64 * 16;                     // float [K_N][64]
constexpr int L_PW = L_C + K_N * C * 4;                          // float [64]: attention pre-norm weight
constexpr int L_QK = L_PW + C * 4;                               // float [32]: q norm weight x QSCALE, k norm weight
constexpr int L_PN = L_QK + 2 * attn::HD * 4;                    // per wave: u16 [42*64] normalised tokens | the attention's gates
constexpr int L_VEC = L_PN + WPB * CELLS * C * 2;                // per wave: u16 [16*VS] B operand, row n = column n of V^T
constexpr int L_SCORE = L_VEC + WPB * 16 * VS * 2;               // per wave: float [48] row-gate scores, then weights
constexpr int L_SLOT = L_SCORE + WPB * 48 * 4;                   // per wave: bf16 [16][64] token means awaiting their value tail
constexpr int L_TOTAL = L_SLOT + WPB * 16 * C * 2;
static_assert(L_TOTAL <= 160 * 1024, "LDS of one CU");
static_assert(CELLS * C * 2 >= attn::GATE_N * 4, "the gate store fits in the token image");

template <bool GUARDED>
__global__ void __launch_bounds__(64 * WPB, 1)
k_attn_heads(const uint16_t *x, const uint16_t *pre_w, const uint16_t *qkvg, const uint16_t *qn_w, const uint16_t *kn_w,
             const uint16_t *o_w, az_nn_heads_weights w, const uint8_t *mask, float *probs, float *wdl, float *moves_left,
             int64_t B, float eps, const int32_t *scatter, const int64_t *batch_dev)
{
    const int64_t rows_total = B;                 // rows of mask / outputs: a compact list may name any of them
    if (batch_dev != nullptr && *batch_dev < B) B = *batch_dev;
    extern __shared__ __align__(16) uint8_t smem[];
    const int wave = threadIdx.x >> 6;
    int lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
    // the loops below start every phase from an opaque copy of the lane number: otherwise the compiler keeps every
    // lane address of every phase live across the whole sample loop (and spills them around the attention)
    auto refresh_lane = [&] {
        asm volatile("" : "+v"(lane));
        l15 = lane & 15;
        l4 = lane >> 4;
    };

    V8 *s_w32 = reinterpret_cast<V8 *>(smem + L_W32);
    V4 *s_w16 = reinterpret_cast<V4 *>(smem + L_W16);
    V8 *s_a = reinterpret_cast<V8 *>(smem + L_A);
    float (*s_c)[C] = reinterpret_cast<float (*)[C]>(smem + L_C);
    float *s_pw = reinterpret_cast<float *>(smem + L_PW);
    float *s_qk = reinterpret_cast<float *>(smem + L_QK);
    uint16_t *s_pn = reinterpret_cast<uint16_t *>(smem + L_PN + wave * CELLS * C * 2);
    float *s_gate = reinterpret_cast<float *>(smem + L_PN + wave * CELLS * C * 2);      // [token tile][head][token], attention only
    uint16_t *s_vec = reinterpret_cast<uint16_t *>(smem + L_VEC + wave * 16 * VS * 2);
    float *s_score = reinterpret_cast<float *>(smem + L_SCORE + wave * 48 * 4);
    uint16_t *s_slot = reinterpret_cast<uint16_t *>(smem + L_SLOT + wave * 16 * C * 2);

    // ---- weights, staged once per workgroup in fragment order
    attn::stage_weights(qkvg, o_w, pre_w, qn_w, kn_w, s_w32, s_w16, s_pw, s_qk);
    stage_weights<A_FRAGS>(w, s_a, s_c);
    if (threadIdx.x < C) {
        const int i = threadIdx.x;
        const float nw = bf1(static_cast<const uint16_t *>(w.p_norm) + i);
        s_c[K_PNORM][i] = nw;
        s_c[K_PNGW][i] = nw * bf1(static_cast<const uint16_t *>(w.p_gate_w) + i);
    }
    for (int i = lane; i < 16 * VS; i += 64) s_vec[i] = 0;
    __syncthreads();
    // 1 / sqrt of an RMS statistic: the default form is launched with eps >= FLT_MIN only (rsq_normal()'s precondition)
    auto rsq = [](float v) {
        if constexpr (GUARDED) return rsqrtf(v);
        else return rsq_normal(v);
    };
    auto cvec4 = [&](int which, int ot) { return *reinterpret_cast<const f32x4 *>(&s_c[which][16 * ot + 4 * l4]); };
    const bool bounded = attn::scores_bounded(s_qk, l4);

    // a wavefront's samples: b0, b0 + S, b0 + 2S, ... (S = wavefronts in the grid), taken two at a time.  nslot of them
    // wait for their value tail, in slots 0 .. nslot - 1: samples fbase, fbase + S, ...
    const int64_t S = static_cast<int64_t>(gridDim.x) * WPB;
    int nslot = 0;
    int64_t fbase = static_cast<int64_t>(blockIdx.x) * WPB + wave;
    for (int64_t b0 = fbase;; b0 += 2 * S) {
        const bool more = b0 < B;
        if (more) {
            const int64_t b1 = b0 + S;
            // The policy tail's two dependent loads, off its path: the pair's output rows are requested next to the first
            // sample's rows, and the mask bytes at those rows after the first sample's token pass - a sample ahead of the
            // tail that reads them.  srow, mbyte: of the sample this lane's policy column belongs to.  srow is consumed
            // through an opaque copy (the "+v" statements below): otherwise the compiler widens it where it is loaded and
            // waits for it there.
            int32_t srow = 0;
            uint32_t mbyte = 1;
#pragma unroll 1
            for (int hs = 0; hs < 2; ++hs) {
                const int64_t bs = hs == 0 ? b0 : b1;
                if (bs >= B) break;
                refresh_lane();
                if (hs == 0) {
                    const int64_t bc = (l15 >> 3) == 0 ? b0 : b1;
                    if (scatter != nullptr && bc < B) srow = scatter[bc];
                }
                const uint16_t *xs = x + bs * (CELLS * C);

                f32x4 out[4][TT];
                attn::attn_sample<GUARDED>(xs, s_w32, s_w16, s_pw, s_qk, s_gate, bounded, eps, lane, l15, l4, out);
                // the residual rows the token pass adds, requested one token tile ahead of the tile that consumes them
                // (a padding token reads row 41 and is zeroed on arrival)
                V4 xq[TT][4];
                auto request_rows = [&](int qt) {
                    const int tok = qt * 16 + l15, row = tok < CELLS ? tok : CELLS - 1;
#pragma unroll
                    for (int ot = 0; ot < 4; ++ot) xq[qt][ot] = *reinterpret_cast<const V4 *>(xs + row * C + ot * 16 + 4 * l4);
                };
                request_rows(0);
                wave_lds_sync();                     // the gates are read: the token image may overwrite them

                // ======== token pass on y = bf16(x + out): lane = token qt*16 + l15, channels 16 ot + 4 l4 + r ========
                f32x2 msum[4][2];
#pragma unroll
                for (int ot = 0; ot < 4; ++ot) msum[ot][0] = msum[ot][1] = f32x2{0.0f, 0.0f};
#pragma unroll
                for (int qt = 0; qt < TT; ++qt) {
                    const int tok = qt * 16 + l15;
                    const bool live = tok < CELLS;
                    f32x2 f[4][2], ss2 = {0.0f, 0.0f}, sc2 = {0.0f, 0.0f};
                    if (qt + 1 < TT) {
                        request_rows(qt + 1);
                        asm volatile("" ::: "memory");       // the requests stay ahead of this tile's arithmetic
                    }
#pragma unroll
                    for (int ot = 0; ot < 4; ++ot) {
                        V4 xr;
                        xr.w[0] = live ? xq[qt][ot].w[0] : 0u;
                        xr.w[1] = live ? xq[qt][ot].w[1] : 0u;
                        const f32x4 ngw = cvec4(K_PNGW, ot);
                        f[ot][0] = unpack2(pack2(out[ot][qt][0] + bf_lo(xr.w[0]), out[ot][qt][1] + bf_hi(xr.w[0])));
                        f[ot][1] = unpack2(pack2(out[ot][qt][2] + bf_lo(xr.w[1]), out[ot][qt][3] + bf_hi(xr.w[1])));
#pragma unroll
                        for (int j = 0; j < 2; ++j) {
                            ss2 = __builtin_elementwise_fma(f[ot][j], f[ot][j], ss2);
                            sc2 = __builtin_elementwise_fma(f[ot][j], f32x2{ngw[2 * j], ngw[2 * j + 1]}, sc2);
                            if (live) msum[ot][j] += f[ot][j];
                        }
                    }
                    float ss = ss2.x + ss2.y, sc = sc2.x + sc2.y;
                    col_sum2(ss, sc);
                    const float r = rsq(ss * (1.0f / C) + eps);
                    if (live) {
#pragma unroll
                        for (int ot = 0; ot < 4; ++ot) {
                            const f32x4 nw = cvec4(K_PNORM, ot);
                            const f32x2 p0 = f[ot][0] * f32x2{r, r} * f32x2{nw[0], nw[1]};
                            const f32x2 p1 = f[ot][1] * f32x2{r, r} * f32x2{nw[2], nw[3]};
                            V4 o;
                            o.w[0] = pack2(p0.x, p0.y);
                            o.w[1] = pack2(p1.x, p1.y);
                            *reinterpret_cast<V4 *>(&s_pn[tok * C + ot * 16 + 4 * l4]) = o;
                        }
                        if (l4 == 0) s_score[tok] = sc * r + w.p_gate_b;
                    }
                }
                // ---- token mean (bf16, like the reference's mean of a bf16 tensor): sums over the 16 lanes of a row,
                // parked in the sample's slot; everything else about the value head waits for the flush
#pragma unroll
                for (int ot = 0; ot < 4; ++ot) {
                    V4 o;
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const f32x2 m = f32x2{sum16_dpp(msum[ot][j].x), sum16_dpp(msum[ot][j].y)} * f32x2{1.0f / CELLS, 1.0f / CELLS};
                        o.w[j] = pack2(m.x, m.y);
                    }
                    if (l15 == 0) *reinterpret_cast<V4 *>(&s_slot[(nslot + hs) * C + 16 * ot + 4 * l4]) = o;
                }
                if (hs == 0) {
                    // the rows are in (they came back with the first sample's): the mask bytes of the pair.  The guard
                    // comes before the address: an index outside the rows is never dereferenced.
                    const int64_t bc = (l15 >> 3) == 0 ? b0 : b1;
                    int32_t sr = srow;
                    asm volatile("" : "+v"(sr));
                    const int64_t b = scatter != nullptr ? sr : bc;
                    if ((l15 & 7) != 7 && bc < B && b >= 0 && b < rows_total && mask != nullptr) mbyte = mask[b * COLS + (l15 & 7)];
                }
                wave_lds_sync();
                pool_columns<VS>(s_score, s_pn, s_vec, hs, lane);
            }

            refresh_lane();
            const int64_t bc = (l15 >> 3) == 0 ? b0 : b1;
            asm volatile("" : "+v"(srow));
            const int64_t b = scatter != nullptr ? srow : bc;
            const bool real = bc < B && b >= 0 && b < rows_total;
            policy_tail_at<VS>(s_a, s_c, s_vec, w, probs, b, real, real && mask != nullptr && mbyte == 0, lane, l15, l4);
            nslot += b1 < B ? 2 : 1;
        }
        // ======== value tail of the parked samples: the slots are full, or this was the last pair ========
        if (nslot == 16 || (!more && nslot > 0)) {
            refresh_lane();
            // Columns nslot .. 15 are dead: they read slot bytes nobody wrote and carry that garbage (NaN included)
            // through the MFMAs on purpose - a column never meets another one (MFMA columns are independent, col_sum
            // stays inside a column) and every store below is guarded by col_live.  Keep it so: no reduction ACROSS
            // columns belongs in this block.
            const bool col_live = l15 < nslot;
            const int64_t bc = fbase + l15 * S;        // column = slot: the slot's sample (< B where the column is live)
            const int64_t b = (col_live && scatter != nullptr) ? scatter[bc] : bc;
            const bool real = col_live && b >= 0 && b < rows_total;
            // pool_norm of the slot's mean -> row l15 of the B operand (s_vec is free: the policy tail has read it)
            f32x2 g0[4][2], q2 = {0.0f, 0.0f};
#pragma unroll
            for (int ot = 0; ot < 4; ++ot) {
                const V4 mv = *reinterpret_cast<const V4 *>(&s_slot[l15 * C + 16 * ot + 4 * l4]);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    g0[ot][j] = unpack2(mv.w[j]);
                    q2 = __builtin_elementwise_fma(g0[ot][j], g0[ot][j], q2);
                }
            }
            const float rn = rsq(col_sum(q2.x + q2.y) * (1.0f / C) + eps);
#pragma unroll
            for (int ot = 0; ot < 4; ++ot) {
                const f32x4 pw = cvec4(K_DPOOL_NORM, ot);
                const f32x2 v0 = g0[ot][0] * f32x2{rn, rn} * f32x2{pw[0], pw[1]};
                const f32x2 v1 = g0[ot][1] * f32x2{rn, rn} * f32x2{pw[2], pw[3]};
                V4 o;
                o.w[0] = pack2(v0.x, v0.y);
                o.w[1] = pack2(v1.x, v1.y);
                *reinterpret_cast<V4 *>(&s_vec[l15 * VS + 16 * ot + 4 * l4]) = o;
            }
            wave_lds_sync();
            auto mean2 = [&](int m, int hh) { return g0[m][hh]; };
            value_tail<VS, !GUARDED>(AFragGlobal{w, l15, l4}, s_c, s_vec, mean2, w, wdl, moves_left, col_live, b, real, eps, l15, l4);
            fbase += nslot * S;
            nslot = 0;
        }
        if (!more) break;
    }
}

}  // namespace

extern "C" int az_nn_attn_heads(const void *x, const void *prenorm_w, const void *qkvg_w, const void *q_norm_w,
                                const void *k_norm_w, const void *o_w, const az_nn_heads_weights *w, const uint8_t *mask,
                                float *probs, float *wdl, float *moves_left, int64_t batch, float eps,
                                const int32_t *scatter, const int64_t *batch_dev, void *stream)
{
    if (batch <= 0 || x == nullptr || w == nullptr || probs == nullptr || wdl == nullptr || moves_left == nullptr) return 1;
    static DeviceSetup setup;
    int cus = setup.cus({reinterpret_cast<const void *>(k_attn_heads<false>), reinterpret_cast<const void *>(k_attn_heads<true>)}, L_TOTAL);
    if (cus == 0) return 2;
    // az_nn_debug: bits 16-27 a cap on the grid (tests: many samples per wavefront)
    const int cap = (az_nn_debug_flags() >> 16) & 0xfff;
    // the default form takes its reciprocal square roots bare (rsq_normal): a smaller eps goes to the form that guards them
    const auto kern = !(eps >= FLT_MIN) ? k_attn_heads<true> : k_attn_heads<false>;
    if (cap > 0 && cap < cus) cus = cap;
    // one workgroup per CU, each wavefront on every S-th sample (S = wavefronts in the grid)
    const int64_t want = (batch + WPB - 1) / WPB;
    const unsigned grid = static_cast<unsigned>(want < cus ? want : cus);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * WPB), L_TOTAL, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(x), static_cast<const uint16_t *>(prenorm_w),
                       static_cast<const uint16_t *>(qkvg_w), static_cast<const uint16_t *>(q_norm_w),
                       static_cast<const uint16_t *>(k_norm_w), static_cast<const uint16_t *>(o_w), *w, mask, probs, wdl,
                       moves_left, batch, eps, scatter, batch_dev);
    return 0;
}
