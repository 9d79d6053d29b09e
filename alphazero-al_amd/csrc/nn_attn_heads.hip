// nn_attn_heads.hip - the gated attention block and both output heads as ONE kernel: residual stream in,
// the three arrays the tree backup consumes out, no token tensor in HBM.
//
// The attention phase is k_attn_block<3> of nn_attn.hip (one wavefront per sample, every intermediate in
// registers).  It ends with out^T in the MFMA C layout - column = token (lane & 15), rows = channels - and
// that is the layout the heads' token pass wants: the per-token RMS statistics and row-gate score are sums
// over a lane's 16 values plus col_sum, the token mean is a sum over the 16 lanes of a row (DPP).  The
// rounded output y = bf16(x + o_proj(...)) never leaves the registers; only the normalised tokens go to a
// per-wave LDS image, for the policy pooling over the 6 rows of each column (tokens 7 apart live in
// different lanes).  From there on the code is that of nn_heads.hip: a wavefront fills the 16-column B
// operand with two samples (its own two consecutive samples of the grid-stride list) and runs the 64x64
// linears and the epilogues once per pair.
//
// Rounding points are those of k_attn_block followed by k_heads: results differ from the two launches only
// through f32 summation order (token mean, RMS statistics).
//
// Shape: one 12-wavefront workgroup per CU (three per SIMD, the attention kernel's occupancy): one copy of
// the attention weights (35 KB) and of the heads' weights (28 KB), and 7.9 KB per wavefront (normalised
// tokens, which double as the attention's gate store, the B operand, scores and means): 158 KB of LDS.
#include <hip/hip_bf16.h>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "az_nn.h"

namespace {

constexpr int CELLS = 42, C = 64, HEADS = 4, HD = 16, TT = 3, ROWS = 6, COLS = 7;
constexpr int WPB = 12;         // wavefronts per workgroup: one workgroup per CU
constexpr int VS = 64;          // bf16 row stride of the B-operand buffer

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
struct alignas(16) V8 { uint32_t w[4]; };
struct alignas(8) V4 { uint32_t w[2]; };

__device__ __forceinline__ float bf_lo(uint32_t w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf_hi(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
// one v_cvt_pk_bf16_f32 (round to nearest even, NaN preserving)
__device__ __forceinline__ uint32_t pack2(float a, float b)
{
    typedef __bf16 pk_bf16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{a, b}, pk_bf16x2));
}
__device__ __forceinline__ f32x2 unpack2(uint32_t w) { return f32x2{bf_lo(w), bf_hi(w)}; }
__device__ __forceinline__ f32x2 rbf2(f32x2 v) { return unpack2(pack2(v.x, v.y)); }       // round to bf16 and back
__device__ __forceinline__ s16x4 to_s16x4(const f32x4 &v)
{
    union { uint32_t u[2]; s16x4 s; } r;
    r.u[0] = pack2(v[0], v[1]);
    r.u[1] = pack2(v[2], v[3]);
    return r.s;
}
__device__ __forceinline__ bf16x8 as_bf16x8(const V8 &v)
{
    union { V8 a; bf16x8 b; } r;
    r.a = v;
    return r.b;
}
__device__ __forceinline__ float bf1(const uint16_t *p) { return __uint_as_float(static_cast<uint32_t>(*p) << 16); }
__device__ __forceinline__ f32x2 silu2(f32x2 x)
{
    const f32x2 t = x * f32x2{-1.44269504f, -1.44269504f};
    const f32x2 e = f32x2{__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)} + f32x2{1.0f, 1.0f};
    return x * f32x2{__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
}
__device__ __forceinline__ float fast_exp(float x) { return __builtin_amdgcn_exp2f(1.44269504f * x); }

template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false));
}
__device__ __forceinline__ float sum8(float v)      // over the 8 lanes that share lane >> 3
{
    v += dpp_mov<0xB1>(v);           // quad_perm [1,0,3,2]
    v += dpp_mov<0x4E>(v);           // quad_perm [2,3,0,1]
    v += dpp_mov<0x141>(v);          // row_half_mirror
    return v;
}
__device__ __forceinline__ float sum16(float v) { v = sum8(v); return v + dpp_mov<0x140>(v); }   // + row_mirror: the 16-lane row
__device__ __forceinline__ float max8(float v)
{
    v = fmaxf(v, dpp_mov<0xB1>(v));
    v = fmaxf(v, dpp_mov<0x4E>(v));
    v = fmaxf(v, dpp_mov<0x141>(v));
    return v;
}
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float col_sum(float v)   // sum over the 4 lane groups that share lane & 15
{
    u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(r.x) + __uint_as_float(r.y);
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(r.x) + __uint_as_float(r.y);
}
__device__ __forceinline__ float col_max(float v)
{
    u32x2 r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(r.x), __uint_as_float(r.y));
    r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(r.x), __uint_as_float(r.y));
}
// LDS traffic between lanes of ONE wavefront: only the compiler has to be stopped from moving accesses across
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16((a), (b), (c), 0, 0, 0)
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x16bf16_1k((a), (b), (c), 0, 0, 0)

// per-channel constants of the heads: those of nn_heads.hip, plus the policy norm weight and norm x row-gate weight
enum { K_PFC_B, K_POUT_W, K_DPOOL_B, K_DNORM, K_DFC_B, K_DOUT_NORM, K_DVAL_B, K_DPOOL_NORM, K_PNORM, K_PNGW, K_N };

// dynamic LDS layout (bytes)
constexpr int L_W32 = 0;                                 // V8 [(3*4*2+2)*64]: wq, wk, wv [h][s], wg [s]
constexpr int L_W16 = L_W32 + 26 * 64 * 16;              // V4 [16*64]: wo [ot][h]
constexpr int L_A = L_W16 + 16 * 64 * 8;                 // V8 [26*64]: heads' A fragments (as nn_heads.hip)
constexpr int L_C = L_A + 26 * 64 * 16;                  // float [K_N][64]
constexpr int L_PW = L_C + K_N * C * 4;                  // float [64]: attention pre-norm weight
constexpr int L_QK = L_PW + C * 4;                       // float [32]: q norm weight x QSCALE, k norm weight
constexpr int L_PN = L_QK + 2 * HD * 4;                  // per wave: u16 [42*64] normalised tokens | f32x4 [3*64] gates
constexpr int L_VEC = L_PN + WPB * CELLS * C * 2;        // per wave: u16 [16*VS] B operand, row n = column n of V^T
constexpr int L_SCORE = L_VEC + WPB * 16 * VS * 2;       // per wave: float [48] row-gate scores, then weights
constexpr int L_MEAN = L_SCORE + WPB * 48 * 4;           // per wave: float [2][64] token means of the pair
constexpr int L_TOTAL = L_MEAN + WPB * 2 * C * 4;
static_assert(CELLS * C * 2 >= TT * 64 * 16, "the gate store fits in the token image");
static_assert(L_TOTAL <= 160 * 1024, "LDS of one CU");

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
    f32x4 *s_gate = reinterpret_cast<f32x4 *>(smem + L_PN + wave * CELLS * C * 2);      // [token tile][lane], attention only
    uint16_t *s_vec = reinterpret_cast<uint16_t *>(smem + L_VEC + wave * 16 * VS * 2);
    float *s_score = reinterpret_cast<float *>(smem + L_SCORE + wave * 48 * 4);
    float *s_mean = reinterpret_cast<float *>(smem + L_MEAN + wave * 2 * C * 4);

    // ---- weights, staged once per workgroup in fragment order (nn_attn.hip, nn_heads.hip)
    for (int i = threadIdx.x; i < (3 * HEADS * 2 + 2) * 64; i += blockDim.x) {
        const int f = i >> 6, l = i & 63, ll15 = l & 15, ll4 = l >> 4;
        V8 v;
        if (f < 3 * HEADS * 2) {
            const int part = f / (HEADS * 2), h = (f >> 1) % HEADS, sk = f & 1;
            v = *reinterpret_cast<const V8 *>(qkvg + (part * C + h * HD + ll15) * C + 32 * sk + 8 * ll4);
        } else {
            // the 4 gate rows repeated over the tile's 16 rows: register r of every lane = head r of its token
            v = *reinterpret_cast<const V8 *>(qkvg + (3 * C + (ll15 & 3)) * C + 32 * (f & 1) + 8 * ll4);
        }
        s_w32[i] = v;
    }
    for (int i = threadIdx.x; i < 4 * HEADS * 64; i += blockDim.x) {
        const int f = i >> 6, l = i & 63, ot = f / HEADS, h = f % HEADS;
        s_w16[i] = *reinterpret_cast<const V4 *>(o_w + (ot * 16 + (l & 15)) * C + h * HD + 4 * (l >> 4));
    }
    for (int i = threadIdx.x; i < 26 * 64; i += blockDim.x) {
        const int f = i >> 6, l = i & 63, r = l & 15, q = l >> 4;
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
        s_a[i] = v;
    }
    constexpr float QSCALE = 0.25f * 1.44269504f;     // 1/sqrt(16) of the scores and log2(e) of their softmax ride on q
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
        const float nw = bf1(static_cast<const uint16_t *>(w.p_norm) + i);
        s_c[K_PNORM][i] = nw;
        s_c[K_PNGW][i] = nw * bf1(static_cast<const uint16_t *>(w.p_gate_w) + i);
        s_pw[i] = bf1(pre_w + i);
        if (i < HD) {
            s_qk[i] = bf1(qn_w + i) * QSCALE;
            s_qk[HD + i] = bf1(kn_w + i);
        }
    }
    for (int i = lane; i < 16 * VS; i += 64) s_vec[i] = 0;
    __syncthreads();

    auto frag32 = [&](int f) { return as_bf16x8(s_w32[f * 64 + lane]); };     // part*8 + h*2 + s ; gate: 24 + s
    auto frag16 = [&](int f) {
        union { V4 v; s16x4 s; } r;
        r.v = s_w16[f * 64 + lane];
        return r.s;
    };
    auto afrag = [&](int f) { return as_bf16x8(s_a[f * 64 + lane]); };
    auto bfrag = [&](int ks) { return as_bf16x8(*reinterpret_cast<const V8 *>(&s_vec[l15 * VS + 32 * ks + 8 * l4])); };
    auto cvec2 = [&](int which, int m, int h) { return *reinterpret_cast<const f32x2 *>(&s_c[which][16 * m + 4 * l4 + 2 * h]); };
    auto cvec4 = [&](int which, int ot) { return *reinterpret_cast<const f32x4 *>(&s_c[which][16 * ot + 4 * l4]); };

    // bound of the scores in log2 units (nn_attn.hip): softmax without a running maximum when it is small
    float mq = 0.0f, mk = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        mq = fmaxf(mq, fabsf(s_qk[4 * l4 + r]));
        mk = fmaxf(mk, fabsf(s_qk[HD + 4 * l4 + r]));
    }
    const bool bounded = 16.0f * col_max(mq) * col_max(mk) < 100.0f;
    auto put_dual = [&](const f32x2 (&v)[4][2]) {
        if ((l15 & 7) == 7) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                uint32_t *p = reinterpret_cast<uint32_t *>(&s_vec[l15 * VS + 16 * m + 4 * l4]);
                p[0] = pack2(v[m][0].x, v[m][0].y);
                p[1] = pack2(v[m][1].x, v[m][1].y);
            }
        }
    };
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};

    // a wavefront's samples: b0, b0 + S, b0 + 2S, ... (S = wavefronts in the grid), taken two at a time
    const int64_t S = static_cast<int64_t>(gridDim.x) * WPB;
    for (int64_t b0 = static_cast<int64_t>(blockIdx.x) * WPB + wave; b0 < B; b0 += 2 * S) {
        const int64_t b1 = b0 + S;
#pragma unroll 1
        for (int hs = 0; hs < 2; ++hs) {
            const int64_t bs = hs == 0 ? b0 : b1;
            if (bs >= B) break;
            refresh_lane();
            const uint16_t *xs = x + bs * (CELLS * C);

            // ======== attention (k_attn_block<3>) ========
            bf16x8 hf[TT][2];
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) {
                const int tok = tt * 16 + l15;
                f32x2 f[2][4], ss2 = {0.0f, 0.0f};
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    V8 v; v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0;
                    if (tok < CELLS) v = *reinterpret_cast<const V8 *>(xs + tok * C + 32 * s + 8 * l4);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        f[s][i] = unpack2(v.w[i]);
                        ss2 = __builtin_elementwise_fma(f[s][i], f[s][i], ss2);
                    }
                }
                const float ss = col_sum(ss2.x + ss2.y);
                const float r = rsqrtf(ss * (1.0f / C) + eps);
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
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) {
                f32x4 g = MFMA32(frag32(24), hf[tt][0], zero);
                g = MFMA32(frag32(25), hf[tt][1], g);
                f32x4 gs;
#pragma unroll
                for (int h = 0; h < HEADS; ++h) gs[h] = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.44269504f * g[h]));
                s_gate[tt * 64 + lane] = gs;
            }

            f32x4 out[4][TT];
#pragma unroll
            for (int ot = 0; ot < 4; ++ot)
#pragma unroll
                for (int qt = 0; qt < TT; ++qt) out[ot][qt] = zero;
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
                    f32x2 q2[2] = {{q[0], q[1]}, {q[2], q[3]}}, k2[2] = {{k[0], k[1]}, {k[2], k[3]}};
                    const f32x2 qq = __builtin_elementwise_fma(q2[1], q2[1], q2[0] * q2[0]);
                    const f32x2 kk = __builtin_elementwise_fma(k2[1], k2[1], k2[0] * k2[0]);
                    const float qs = col_sum(qq.x + qq.y), ks = col_sum(kk.x + kk.y);
                    const float qr = rsqrtf(qs * (1.0f / HD) + eps), kr = rsqrtf(ks * (1.0f / HD) + eps);
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
#pragma unroll
                for (int qt = 0; qt < TT; ++qt) {
                    f32x4 st[TT];
                    float den;
                    if (bounded) {
                        // the six padding keys have k = 0: weight exp2(0) = 1 each, V rows 0 (nn_attn.hip)
                        f32x2 den2 = {0.0f, 0.0f};
#pragma unroll
                        for (int kt = 0; kt < TT; ++kt) {
                            st[kt] = MFMA16(kb[kt], qb[qt], zero);
#pragma unroll
                            for (int r = 0; r < 4; r += 2) {
                                const f32x2 e = {__builtin_amdgcn_exp2f(st[kt][r]), __builtin_amdgcn_exp2f(st[kt][r + 1])};
                                st[kt][r] = e.x;
                                st[kt][r + 1] = e.y;
                                den2 += e;
                            }
                        }
                        den = col_sum(den2.x + den2.y) - static_cast<float>(TT * 16 - CELLS);
                    } else {
                        float m = -INFINITY;
#pragma unroll
                        for (int kt = 0; kt < TT; ++kt) {
                            st[kt] = MFMA16(kb[kt], qb[qt], zero);
#pragma unroll
                            for (int r = 0; r < 4; ++r) {
                                if (kt == TT - 1 && kt * 16 + 4 * l4 + r >= CELLS) st[kt][r] = -INFINITY;
                                m = fmaxf(m, st[kt][r]);
                            }
                        }
                        m = col_max(m);
                        f32x2 den2 = {0.0f, 0.0f};
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
                        den = col_sum(den2.x + den2.y);
                    }
                    const float gq = reinterpret_cast<const float *>(&s_gate[qt * 64 + lane])[h];
                    const float scale = __builtin_amdgcn_rcpf(den) * gq;
                    f32x4 o = zero;
#pragma unroll
                    for (int kt = 0; kt < TT; ++kt) o = MFMA16(vb[kt], to_s16x4(st[kt]), o);
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] *= scale;
                    const s16x4 ob = to_s16x4(o);
#pragma unroll
                    for (int ot = 0; ot < 4; ++ot) out[ot][qt] = MFMA16(frag16(ot * HEADS + h), ob, out[ot][qt]);
                }
            }
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
#pragma unroll
                for (int ot = 0; ot < 4; ++ot) {
                    V4 xr; xr.w[0] = xr.w[1] = 0;
                    if (live) xr = *reinterpret_cast<const V4 *>(xs + tok * C + ot * 16 + 4 * l4);
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
                const float ss = col_sum(ss2.x + ss2.y), sc = col_sum(sc2.x + sc2.y);
                const float r = rsqrtf(ss * (1.0f / C) + eps);
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
            // ---- token mean (bf16, like the reference's mean of a bf16 tensor): sums over the 16 lanes of a row;
            // kept for the residual, and its pool_norm goes to this sample's value column 8 hs + 7
            {
                f32x2 g0[4][2], q2 = {0.0f, 0.0f};
#pragma unroll
                for (int ot = 0; ot < 4; ++ot)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const f32x2 m = {sum16(msum[ot][j].x), sum16(msum[ot][j].y)};
                        g0[ot][j] = rbf2(m * f32x2{1.0f / CELLS, 1.0f / CELLS});
                        q2 = __builtin_elementwise_fma(g0[ot][j], g0[ot][j], q2);
                    }
                const float rn = rsqrtf(col_sum(q2.x + q2.y) * (1.0f / C) + eps);
                if (l15 == 0) {
#pragma unroll
                    for (int ot = 0; ot < 4; ++ot) {
                        *reinterpret_cast<f32x4 *>(&s_mean[hs * C + 16 * ot + 4 * l4]) = f32x4{g0[ot][0].x, g0[ot][0].y, g0[ot][1].x, g0[ot][1].y};
                        const f32x4 pw = cvec4(K_DPOOL_NORM, ot);
                        const f32x2 v0 = g0[ot][0] * f32x2{rn, rn} * f32x2{pw[0], pw[1]};
                        const f32x2 v1 = g0[ot][1] * f32x2{rn, rn} * f32x2{pw[2], pw[3]};
                        V4 o;
                        o.w[0] = pack2(v0.x, v0.y);
                        o.w[1] = pack2(v1.x, v1.y);
                        *reinterpret_cast<V4 *>(&s_vec[(8 * hs + 7) * VS + 16 * ot + 4 * l4]) = o;
                    }
                }
            }
            wave_lds_sync();
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
                const uint32_t *pn2 = reinterpret_cast<const uint32_t *>(s_pn);
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

        // ======== both samples of the pair: columns 0-6 | 7 and 8-14 | 15 of the B operand (nn_heads.hip) ========
        refresh_lane();
        const bool dual = (l15 & 7) == 7;          // this lane's accumulator column is a value-head vector
        const int half = l15 >> 3;                 // which sample of the pair the column belongs to
        const int64_t bc = half == 0 ? b0 : b1;       // the sample this lane's column belongs to
        const int64_t b = (bc < B && scatter != nullptr) ? scatter[bc] : bc;
        const bool real = bc < B && b >= 0 && b < rows_total;
        f32x4 ap[4], ad[4];
        {
            const bf16x8 v0 = bfrag(0), v1 = bfrag(1);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                ap[m] = MFMA32(afrag(2 * m), v0, zero);
                ap[m] = MFMA32(afrag(2 * m + 1), v1, ap[m]);
                ad[m] = MFMA32(afrag(8 + 2 * m), v0, zero);
                ad[m] = MFMA32(afrag(8 + 2 * m + 1), v1, ad[m]);
            }
        }
        // policy: logit[c] = out . silu(fc(col_c) + b), masked softmax over the 7 columns of a sample
        {
            f32x2 part2 = {0.0f, 0.0f};
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const f32x2 xv = rbf2(f32x2{ap[m][2 * hh], ap[m][2 * hh + 1]} + cvec2(K_PFC_B, m, hh));
                    part2 = __builtin_elementwise_fma(rbf2(silu2(xv)), cvec2(K_POUT_W, m, hh), part2);
                }
            float logit = col_sum(part2.x + part2.y) + w.p_out_b;
            const bool live = !dual;
            if (live && real && mask != nullptr && mask[b * COLS + (l15 & 7)] == 0) logit = -1e9f;
            if (!live) logit = -INFINITY;
            const float mx = max8(logit);
            const float e = live ? fast_exp(logit - mx) : 0.0f;
            const float den = sum8(e);
            if (live && real && l4 == 0) probs[b * COLS + (l15 & 7)] = e * __builtin_amdgcn_rcpf(den);
        }
        // value head, stage 1 (dual columns): g = mean + silu(pool_fc(pool_norm(mean)) + b); n2 = norm(g)
        f32x2 g[4][2];
        {
            f32x2 ss2 = {0.0f, 0.0f};
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    const f32x2 mean = *reinterpret_cast<const f32x2 *>(&s_mean[half * C + 16 * m + 4 * l4 + 2 * hh]);
                    const f32x2 xv = rbf2(f32x2{ad[m][2 * hh], ad[m][2 * hh + 1]} + cvec2(K_DPOOL_B, m, hh));
                    g[m][hh] = rbf2(mean + rbf2(silu2(xv)));
                    ss2 = __builtin_elementwise_fma(g[m][hh], g[m][hh], ss2);
                }
            const float rn = rsqrtf(col_sum(ss2.x + ss2.y) * (1.0f / C) + eps);
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) g[m][hh] = g[m][hh] * f32x2{rn, rn} * cvec2(K_DNORM, m, hh);
        }
        wave_lds_sync();
        put_dual(g);
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
            const float rn = rsqrtf(col_sum(ss2.x + ss2.y) * (1.0f / C) + eps);
#pragma unroll
            for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) g[m][hh] = g[m][hh] * f32x2{rn, rn} * cvec2(K_DOUT_NORM, m, hh);
        }
        wave_lds_sync();
        put_dual(g);
        wave_lds_sync();
        // stage 3: rows 0-2 = value logits, row 3 = moves-left logit, in the dual lanes with l4 == 0
        {
            f32x4 acc = MFMA32(afrag(24), bfrag(0), zero);
            acc = MFMA32(afrag(25), bfrag(1), acc);
            if (dual && l4 == 0 && real) {
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
}

// per device: the dynamic-LDS limit raised once, and the CU count the grid is sized by
constexpr int kMaxDevices = 64;
struct DeviceSetup {
    std::once_flag once;
    bool ok = false;
    int cus = 0;
} g_setup[kMaxDevices];

}  // namespace

extern "C" int az_nn_attn_heads(const void *x, const void *prenorm_w, const void *qkvg_w, const void *q_norm_w,
                                const void *k_norm_w, const void *o_w, const az_nn_heads_weights *w, const uint8_t *mask,
                                float *probs, float *wdl, float *moves_left, int64_t batch, float eps,
                                const int32_t *scatter, const int64_t *batch_dev, void *stream)
{
    if (batch <= 0 || x == nullptr || w == nullptr || probs == nullptr || wdl == nullptr || moves_left == nullptr) return 1;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return 2;
    DeviceSetup &ds = g_setup[dev];
    std::call_once(ds.once, [&] {
        ds.ok = hipFuncSetAttribute(reinterpret_cast<const void *>(k_attn_heads), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    L_TOTAL) == hipSuccess &&
                hipDeviceGetAttribute(&ds.cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ds.cus > 0;
    });
    if (!ds.ok) return 2;
    // one workgroup per CU, each wavefront on every S-th sample (S = wavefronts in the grid)
    const int64_t want = (batch + WPB - 1) / WPB;
    const unsigned grid = static_cast<unsigned>(want < ds.cus ? want : ds.cus);
    hipLaunchKernelGGL(k_attn_heads, dim3(grid), dim3(64 * WPB), L_TOTAL, static_cast<hipStream_t>(stream),
                       static_cast<const uint16_t *>(x), static_cast<const uint16_t *>(prenorm_w),
                       static_cast<const uint16_t *>(qkvg_w), static_cast<const uint16_t *>(q_norm_w),
                       static_cast<const uint16_t *>(k_norm_w), static_cast<const uint16_t *>(o_w), *w, mask, probs, wdl,
                       moves_left, batch, eps, scatter, batch_dev);
    return 0;
}
