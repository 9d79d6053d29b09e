// train_attn_kernels.hip - the learner's second network piece: the training forward and backward of the Connect4 gated
// attention block (az_train_*attn* in az_train.h; the reference's `AttentionBlock(64, 4, dropout)`), kernels and host
// entry points in this one unit.  float32, 42 tokens of 64 channels, 4 heads of 16.  Three kernels:
//
//   k_attn_fwd     a workgroup of four wavefronts takes samples n = blockIdx, blockIdx + grid, ...  Per sample: the
//                  tokens into LDS as [48][65] (rows 42 .. 47 stay zero), the RMS pre-norm (four lanes a token), then
//                  WAVEFRONT a OWNS HEAD a: its q, k, v as a 48 x 48 x 64 product on v_mfma_f32_16x16x4_f32 into its
//                  own LDS region, the gate, the two 16-wide norms (a lane a token), the scores TRANSPOSED
//                  (S^T[j][i], so that a softmax row is a lane's registers and its three partners across lane / 16),
//                  the softmax with keys 42 .. 47 left out, the mask bits, and P'V straight from the registers: a
//                  16 x 16 x 4 MFMA's K index may be any permutation as long as both operands use it, so the C layout
//                  of S^T (row 4 * (lane / 16) + r, column lane % 16) IS the A layout of P' with K = 4 * (lane / 16) + r.
//                  Then all four wavefronts run the output projection (wavefront w owns channels 16w .. 16w + 15), add
//                  the skip and store 64-byte runs.
//   k_attn_bwd     a workgroup walks a contiguous run of samples.  Per sample it runs the forward again (nothing but
//                  the inputs is kept between the passes) and keeps P in registers; do = Wo^T dy for head a is again
//                  wavefront a's; dP'^T and dS^T are formed in the registers' layout, the two products that contract
//                  over the queries (dv, dk) read P'^T and dS^T back from the wavefront's LDS region; the norms'
//                  backward runs on the tiles (a token's 16 values are 16 lanes).  dq, dk, dv replace q, k, v in place,
//                  then d_qkv += dqkv^T h (48 accumulator registers a lane, kept over the workgroup's samples, as are
//                  d_o's 16), dh = dqkv Wqkv + dg Wgate, the pre-norm's backward and the skip.  At the end ONE partial
//                  row (16736 floats) in the caller's workspace.
//   k_attn_reduce  one lane per parameter-gradient element adds the rows in row order.
//
// The weights (66 KB) are read from global memory (L2-resident) as MFMA operands; every other operand is LDS.
// Row strides 65, 17 and 49 keep the 16 rows of an operand on 16 banks.
// An MFMA here is a k-ordered chain of float32 fused multiply-adds: exact float32, nothing narrower anywhere.
// No atomics, nothing cleared beforehand: two calls on the same inputs give the same bytes.  Plain C++ and vector
// stores only.
#include "engine_internal.h"

#include "az_train.h"
#include "nn_common.h"
#include "train_common.h"

namespace az {
namespace {

constexpr int WAVE = 64;
constexpr int BLOCK = 256, WAVES = BLOCK / WAVE;
constexpr int CH = 64, HEADS = 4, HD = 16, TOK = 42;
constexpr int TP = 48, TT = TP / 16;            // tokens padded to three tiles of 16
constexpr int TOK_STEPS = 11;                   // 44 tokens in K steps of 4 (rows 42 and 43 are zero)
constexpr int ACT = TOK * CH;                   // 2688 values of a sample
constexpr int PER_LANE = (ACT + BLOCK - 1) / BLOCK;
constexpr int RS = CH + 1, HS = HD + 1, PS = TP + 1;     // row strides in LDS: [48][65], [48][17], [48][49]
constexpr int QKV_NUMEL = 3 * CH * CH, O_NUMEL = CH * CH, G_NUMEL = HEADS * CH;
constexpr int ROW_FLOATS = QKV_NUMEL + O_NUMEL + G_NUMEL + CH + 2 * HD;      // 16736: d_qkv, d_o, d_gate, d_prenorm, d_q_norm, d_k_norm
constexpr int FWD_GRID = 1024;
constexpr float SCALE = 0.25f;                  // 1 / sqrt(16)
static_assert(WAVES == HEADS && HEADS * HD == CH, "a wavefront owns a head and a 16-channel tile");
static_assert(ROW_FLOATS % 4 == 0 && ROW_FLOATS == 16736, "rows of the workspace stay 16-byte aligned");
static_assert(TOK_STEPS * 4 >= TOK && TOK_STEPS * 4 <= TP, "the token steps stay inside the padded rows");

struct AttnArgs {
    const float *x, *pre, *Wqkv, *Wg, *Wo, *qn, *kn, *dy;
    const uint64_t *bits;
    float *y;
    float *dx, *d_pre, *d_qkv, *d_gate, *d_o, *d_qn, *d_kn, *ws;
    int64_t N, per;                             // per: the run of samples a backward workgroup walks
    int rows;                                   // backward workgroups = partial rows
    int token_major;
    float eps, keep_scale;
};

struct FwdLds {
    float tok[TP * RS];                         // the sample's tokens; rows 42 .. 47 are zero from the start on
    float h[TP * RS];                           // the pre-normed tokens
    float o[TP * RS];                           // P'V of the four heads side by side, BEFORE the gate
    float hd[WAVES][3][TP * HS];                // head a: q, k (normalised, without the norm's weight), v
    float rinv[TP];                             // the pre-norm's rsqrt per token
    float rq[WAVES][TP], rk[WAVES][TP];         // the head norms' rsqrt per token
    float gs[WAVES][TP];                        // sigmoid of the gate
};

struct BwdLds {
    FwdLds f;
    float dy[TP * RS];                          // the upstream gradient, rows 42 .. 47 zero; at the end dx's tokens
    float g[TP * RS];                           // do, then do * gate per head, then dh
    float pt[WAVES][TP * PS];                   // head a: P'^T, then dS^T, as [key][query]
    float delta[WAVES][TP], dg[WAVES][TP];
    float red[2][WAVES][HD];
};

__device__ __forceinline__ f4 zero4() { return f4{0.0f, 0.0f, 0.0f, 0.0f}; }

// element e of a sample in the caller's layout -> its place in a [48][65] token image
__device__ __forceinline__ int token_pos(int e, int token_major)
{
    return token_major ? (e >> 6) * RS + (e & 63) : (e % TOK) * RS + e / TOK;
}

// the mask words of this lane's three queries (lane % 16 + 16 * it); a query beyond 41 keeps nothing
__device__ __forceinline__ void load_bits(const AttnArgs &a, int64_t n, uint64_t kb[TT])
{
    const int l15 = threadIdx.x & 15, wave = threadIdx.x / WAVE;
#pragma unroll
    for (int it = 0; it < TT; ++it) {
        const int i = 16 * it + l15;
        kb[it] = i >= TOK ? 0 : a.bits != nullptr ? a.bits[(n * HEADS + wave) * TOK + i] : ~uint64_t(0);
    }
}

// The forward up to the head norms: tokens, pre-norm, this wavefront's q, k, v and gate.  Ends behind a barrier.
__device__ __forceinline__ void forward_front(const AttnArgs &a, int64_t n, FwdLds &L)
{
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, l15 = lane & 15, kq = lane >> 4;
    const float *xs = a.x + n * ACT;
#pragma unroll
    for (int j = 0; j < PER_LANE; ++j) {
        const int e = tid + j * BLOCK;
        if (e < ACT) L.tok[token_pos(e, a.token_major)] = xs[e];
    }
    __syncthreads();
    {   // the pre-norm: four lanes a token, 16 channels each
        const int t = tid >> 2, q = tid & 3;
        float ss = 0.0f;
        if (t < TP)
#pragma unroll
            for (int k = 0; k < CH / 4; ++k) { const float v = L.tok[t * RS + q + 4 * k]; ss += v * v; }
        ss += __shfl_xor(ss, 1, WAVE);
        ss += __shfl_xor(ss, 2, WAVE);
        const float r = 1.0f / sqrtf(ss / static_cast<float>(CH) + a.eps);
        if (t < TP) {
            if (q == 0) L.rinv[t] = r;
#pragma unroll
            for (int k = 0; k < CH / 4; ++k) { const int c = q + 4 * k; L.h[t * RS + c] = L.tok[t * RS + c] * r * a.pre[c]; }
        }
    }
    __syncthreads();
    // q, k, v of head `wave`: [t][d] = sum_c h[t][c] * Wqkv[third * 64 + wave * 16 + d][c]
#pragma unroll
    for (int th = 0; th < 3; ++th) {
        f4 acc[TT];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) acc[tt] = zero4();
        const float *wrow = a.Wqkv + (th * CH + wave * HD + l15) * CH;
#pragma unroll 4
        for (int s = 0; s < CH / 4; ++s) {
            const int c = 4 * s + kq;
            const float b = wrow[c];
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) acc[tt] = mfma(L.h[(16 * tt + l15) * RS + c], b, acc[tt]);
        }
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) L.hd[wave][th][(16 * tt + 4 * kq + r) * HS + l15] = acc[tt][r];
    }
    if (lane < TP) {                            // the gate of head `wave`, a lane a token
        float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
        for (int c = 0; c < CH; c += 4)
#pragma unroll
            for (int u = 0; u < 4; ++u) g[u] += a.Wg[wave * CH + c + u] * L.h[lane * RS + c + u];
        L.gs[wave][lane] = sigmoid((g[0] + g[1]) + (g[2] + g[3]));
    }
    __syncthreads();
    if (lane < TP) {                            // the two head norms, a lane a token; the weight is applied where q and k are read
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            float *p = &L.hd[wave][which][lane * HS];
            float ss = 0.0f;
#pragma unroll
            for (int d = 0; d < HD; ++d) ss += p[d] * p[d];
            const float r = 1.0f / sqrtf(ss / static_cast<float>(HD) + a.eps);
#pragma unroll
            for (int d = 0; d < HD; ++d) p[d] *= r;
            (which == 0 ? L.rq : L.rk)[wave][lane] = r;
        }
    }
    __syncthreads();
}

// P^T of head `wave` in registers: p[jt][it][r] = P[query 16 it + lane % 16][key 16 jt + 4 (lane / 16) + r]; keys beyond 41 are 0
__device__ __forceinline__ void head_probs(const AttnArgs &a, const FwdLds &L, f4 p[TT][TT])
{
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, l15 = lane & 15, kq = lane >> 4;
    const float *Q = L.hd[wave][0], *K = L.hd[wave][1];
#pragma unroll
    for (int jt = 0; jt < TT; ++jt)
#pragma unroll
        for (int it = 0; it < TT; ++it) p[jt][it] = zero4();
#pragma unroll
    for (int s = 0; s < HD / 4; ++s) {
        const int d = 4 * s + kq;
        const float wq = a.qn[d], wk = a.kn[d];
        float av[TT], bv[TT];
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            av[t] = K[(16 * t + l15) * HS + d] * wk;
            bv[t] = Q[(16 * t + l15) * HS + d] * wq;
        }
#pragma unroll
        for (int jt = 0; jt < TT; ++jt)
#pragma unroll
            for (int it = 0; it < TT; ++it) p[jt][it] = mfma(av[jt], bv[it], p[jt][it]);
    }
#pragma unroll
    for (int it = 0; it < TT; ++it) {
        float m = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < TT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (16 * jt + 4 * kq + r < TOK) m = fmaxf(m, p[jt][it][r] * SCALE);
        m = fmaxf(m, __shfl_xor(m, 16, WAVE));
        m = fmaxf(m, __shfl_xor(m, 32, WAVE));
        float l = 0.0f;
#pragma unroll
        for (int jt = 0; jt < TT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float e = 16 * jt + 4 * kq + r < TOK ? expf(p[jt][it][r] * SCALE - m) : 0.0f;
                p[jt][it][r] = e;
                l += e;
            }
        l += __shfl_xor(l, 16, WAVE);
        l += __shfl_xor(l, 32, WAVE);
#pragma unroll
        for (int jt = 0; jt < TT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) p[jt][it][r] = p[jt][it][r] / l;
    }
}

// the factor dropout puts on probability (query of word `w`, key j): 0 or keep_scale
__device__ __forceinline__ float keep_factor(uint64_t w, int j, float keep_scale) { return (w >> j) & 1 ? keep_scale : 0.0f; }

// o[i][16 wave + d] = sum_j P'[i][j] v[j][d], straight from the registers (K index 4 (lane / 16) + r in both operands)
__device__ __forceinline__ void head_pv(const AttnArgs &a, FwdLds &L, const f4 p[TT][TT], const uint64_t kb[TT])
{
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE, l15 = lane & 15, kq = lane >> 4;
    const float *V = L.hd[wave][2];
#pragma unroll
    for (int it = 0; it < TT; ++it) {
        f4 acc = zero4();
#pragma unroll
        for (int jt = 0; jt < TT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * jt + 4 * kq + r;
                acc = mfma(p[jt][it][r] * keep_factor(kb[it], j, a.keep_scale), V[j * HS + l15], acc);
            }
#pragma unroll
        for (int r = 0; r < 4; ++r) L.o[(16 * it + 4 * kq + r) * RS + wave * HD + l15] = acc[r];
    }
}

__global__ void __launch_bounds__(BLOCK) k_attn_fwd(AttnArgs a)
{
    __shared__ FwdLds L;
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, l15 = lane & 15, kq = lane >> 4;
    for (int i = tid; i < static_cast<int>(sizeof(FwdLds) / sizeof(float)); i += BLOCK) reinterpret_cast<float *>(&L)[i] = 0.0f;
    __syncthreads();
    for (int64_t n = blockIdx.x; n < a.N; n += gridDim.x) {
        forward_front(a, n, L);
        f4 p[TT][TT];
        uint64_t kb[TT];
        load_bits(a, n, kb);
        head_probs(a, L, p);
        head_pv(a, L, p, kb);
        __syncthreads();
        // y[i][16 wave + c] = sum_c' gate * o[i][c'] * Wo[16 wave + c][c'] + tok[i][.]
        f4 acc[TT];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) acc[tt] = zero4();
        const float *wrow = a.Wo + (wave * HD + l15) * CH;
#pragma unroll 4
        for (int s = 0; s < CH / 4; ++s) {
            const int c = 4 * s + kq;
            const float b = wrow[c];
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) {
                const int i = 16 * tt + l15;
                acc[tt] = mfma(L.o[i * RS + c] * L.gs[c >> 4][i], b, acc[tt]);
            }
        }
        float *ys = a.y + n * ACT;
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = 16 * tt + 4 * kq + r, c = wave * HD + l15;
                if (i < TOK) ys[i * CH + c] = acc[tt][r] + L.tok[i * RS + c];
            }
        __syncthreads();                        // tok and o are read to the end before the next sample goes in
    }
}

// the backward of a 16-wide RMS norm on a tile: g[r] is the gradient of the normed, weighted value of token
// 16 t + 4 (lane / 16) + r at d = lane % 16; `img` holds the normalised values and receives the input's gradient.
// Returns this lane's share of the weight's gradient.
__device__ __forceinline__ float head_norm_bwd(float *img, const float *rstd, int t, f4 g, float w)
{
    const int lane = threadIdx.x % WAVE, l15 = lane & 15, kq = lane >> 4;
    float dw = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 16 * t + 4 * kq + r;
        const float xn = img[i * HS + l15], u = g[r] * w;
        dw += g[r] * xn;
        float s = u * xn;
        s += __shfl_xor(s, 1, WAVE);
        s += __shfl_xor(s, 2, WAVE);
        s += __shfl_xor(s, 4, WAVE);
        s += __shfl_xor(s, 8, WAVE);
        img[i * HS + l15] = rstd[i] * (u - xn * (s / static_cast<float>(HD)));
    }
    return dw;
}

__global__ void __launch_bounds__(BLOCK) k_attn_bwd(AttnArgs a)
{
    __shared__ BwdLds B;
    FwdLds &L = B.f;
    const int tid = threadIdx.x, lane = tid % WAVE, wave = tid / WAVE, l15 = lane & 15, kq = lane >> 4;
    for (int i = tid; i < static_cast<int>(sizeof(BwdLds) / sizeof(float)); i += BLOCK) reinterpret_cast<float *>(&B)[i] = 0.0f;
    __syncthreads();

    f4 acc_w[3][HEADS];                         // d_qkv rows third * 64 + 16 wave + (0 .. 15), all 64 columns
    f4 acc_o[HEADS];                            // d_o columns 16 wave + (0 .. 15), all 64 rows
#pragma unroll
    for (int ct = 0; ct < HEADS; ++ct) {
        acc_o[ct] = zero4();
#pragma unroll
        for (int th = 0; th < 3; ++th) acc_w[th][ct] = zero4();
    }
    float p_dgate = 0.0f;                       // d_gate[wave][lane]
    float p_dpre = 0.0f;                        // d_prenorm[tid / 4], the same in its four lanes
    float p_dqn = 0.0f, p_dkn = 0.0f;           // this lane's share of d_q_norm[lane % 16], d_k_norm[lane % 16]
    const float wq_l = a.qn[l15], wk_l = a.kn[l15];
    float *Q = L.hd[wave][0], *K = L.hd[wave][1], *V = L.hd[wave][2], *PT = B.pt[wave];
    const int col = wave * HD + l15;            // this lane's column of its head in a [48][65] image

    const int64_t n0 = static_cast<int64_t>(blockIdx.x) * a.per;
    const int64_t n1 = n0 + a.per < a.N ? n0 + a.per : a.N;
    for (int64_t n = n0; n < n1; ++n) {
        const float *dys = a.dy + n * ACT;
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            const int e = tid + j * BLOCK;
            if (e < ACT) B.dy[(e >> 6) * RS + (e & 63)] = dys[e];
        }
        forward_front(a, n, L);                 // its barriers cover dy as well
        f4 p[TT][TT];
        uint64_t kb[TT];
        load_bits(a, n, kb);
        head_probs(a, L, p);
        head_pv(a, L, p, kb);
        {   // do[i][16 wave + c'] = sum_c dy[i][c] * Wo[c][16 wave + c']
            f4 acc[TT];
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) acc[tt] = zero4();
#pragma unroll 4
            for (int s = 0; s < CH / 4; ++s) {
                const int c = 4 * s + kq;
                const float b = a.Wo[c * CH + col];
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) acc[tt] = mfma(B.dy[(16 * tt + l15) * RS + c], b, acc[tt]);
            }
#pragma unroll
            for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) B.g[(16 * tt + 4 * kq + r) * RS + col] = acc[tt][r];
        }
        __syncthreads();
        if (lane < TP) {                        // a lane a token: the gate's gradient, do * gate in place, delta = sum_j P' dP'
            const float sg = L.gs[wave][lane];
            float *dop = &B.g[lane * RS + wave * HD];
            const float *op = &L.o[lane * RS + wave * HD];
            float s = 0.0f;
#pragma unroll
            for (int d = 0; d < HD; ++d) s += dop[d] * op[d];
#pragma unroll
            for (int d = 0; d < HD; ++d) dop[d] *= sg;
            B.dg[wave][lane] = s * (sg * (1.0f - sg));
            B.delta[wave][lane] = s * sg;
        }
        __syncthreads();
        // d_o[c][16 wave + c'] += sum_i dy[i][c] * gate * o[i][16 wave + c']
#pragma unroll 1
        for (int s = 0; s < TOK_STEPS; ++s) {
            const int i = 4 * s + kq;
            const float b = L.o[i * RS + col] * L.gs[wave][i];
#pragma unroll
            for (int ct = 0; ct < HEADS; ++ct) acc_o[ct] = mfma(B.dy[i * RS + 16 * ct + l15], b, acc_o[ct]);
        }
        // dP'^T[j][i] = sum_d v[j][d] * dov[i][d], in p's layout; then dS^T in its place
        f4 ds[TT][TT];
#pragma unroll
        for (int jt = 0; jt < TT; ++jt)
#pragma unroll
            for (int it = 0; it < TT; ++it) ds[jt][it] = zero4();
#pragma unroll
        for (int s = 0; s < HD / 4; ++s) {
            const int d = 4 * s + kq;
            float av[TT], bv[TT];
#pragma unroll
            for (int t = 0; t < TT; ++t) {
                av[t] = V[(16 * t + l15) * HS + d];
                bv[t] = B.g[(16 * t + l15) * RS + wave * HD + d];
            }
#pragma unroll
            for (int jt = 0; jt < TT; ++jt)
#pragma unroll
                for (int it = 0; it < TT; ++it) ds[jt][it] = mfma(av[jt], bv[it], ds[jt][it]);
        }
#pragma unroll
        for (int it = 0; it < TT; ++it) {
            const int i = 16 * it + l15;
            const float delta = B.delta[wave][i];
#pragma unroll
            for (int jt = 0; jt < TT; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * jt + 4 * kq + r;
                    const float keep = keep_factor(kb[it], j, a.keep_scale);
                    PT[j * PS + i] = p[jt][it][r] * keep;
                    ds[jt][it][r] = i < TOK ? SCALE * (p[jt][it][r] * (keep * ds[jt][it][r] - delta)) : 0.0f;
                }
        }
        __syncthreads();
        f4 dvt[TT];                             // dv[j][d] = sum_i P'^T[j][i] * dov[i][d]
#pragma unroll
        for (int jt = 0; jt < TT; ++jt) dvt[jt] = zero4();
#pragma unroll 1
        for (int s = 0; s < TOK_STEPS; ++s) {
            const int i = 4 * s + kq;
            const float b = B.g[i * RS + col];
#pragma unroll
            for (int jt = 0; jt < TT; ++jt) dvt[jt] = mfma(PT[(16 * jt + l15) * PS + i], b, dvt[jt]);
        }
        __syncthreads();
        f4 dqh[TT];                             // dqh[i][d] = sum_j dS[i][j] * kh[j][d], from the registers
#pragma unroll
        for (int it = 0; it < TT; ++it) {
            dqh[it] = zero4();
#pragma unroll
            for (int jt = 0; jt < TT; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * jt + 4 * kq + r;
                    PT[j * PS + 16 * it + l15] = ds[jt][it][r];
                    dqh[it] = mfma(ds[jt][it][r], K[j * HS + l15] * wk_l, dqh[it]);
                }
        }
        __syncthreads();
        f4 dkh[TT];                             // dkh[j][d] = sum_i dS^T[j][i] * qh[i][d]
#pragma unroll
        for (int jt = 0; jt < TT; ++jt) dkh[jt] = zero4();
#pragma unroll 1
        for (int s = 0; s < TOK_STEPS; ++s) {
            const int i = 4 * s + kq;
            const float b = Q[i * HS + l15] * wq_l;
#pragma unroll
            for (int jt = 0; jt < TT; ++jt) dkh[jt] = mfma(PT[(16 * jt + l15) * PS + i], b, dkh[jt]);
        }
        __syncthreads();                        // q, k, v are read to the end: their gradients take their places
#pragma unroll
        for (int t = 0; t < TT; ++t) {
            p_dqn += head_norm_bwd(Q, L.rq[wave], t, dqh[t], wq_l);
            p_dkn += head_norm_bwd(K, L.rk[wave], t, dkh[t], wk_l);
#pragma unroll
            for (int r = 0; r < 4; ++r) V[(16 * t + 4 * kq + r) * HS + l15] = dvt[t][r];
        }
        __syncthreads();
        // d_qkv[third * 64 + 16 wave + d][c] += sum_t dqkv[t][.] * h[t][c]
#pragma unroll 1
        for (int s = 0; s < TOK_STEPS; ++s) {
            const int t = 4 * s + kq;
            float av[3], bv[HEADS];
#pragma unroll
            for (int th = 0; th < 3; ++th) av[th] = L.hd[wave][th][t * HS + l15];
#pragma unroll
            for (int ct = 0; ct < HEADS; ++ct) bv[ct] = L.h[t * RS + 16 * ct + l15];
#pragma unroll
            for (int th = 0; th < 3; ++th)
#pragma unroll
                for (int ct = 0; ct < HEADS; ++ct) acc_w[th][ct] = mfma(av[th], bv[ct], acc_w[th][ct]);
        }
        {   // d_gate[wave][lane] += sum_t dg[t][wave] * h[t][lane]
            float v = 0.0f;
            for (int t = 0; t < TOK; ++t) v += B.dg[wave][t] * L.h[t * RS + lane];
            p_dgate += v;
        }
        {   // dh[t][16 wave + c] = sum_o dqkv[t][o] * Wqkv[o][16 wave + c]; dov of this head is read to the end, dh takes its place
            f4 acc[TT];
#pragma unroll
            for (int tt = 0; tt < TT; ++tt) acc[tt] = zero4();
#pragma unroll 1
            for (int th = 0; th < 3; ++th)
#pragma unroll 1
                for (int hh = 0; hh < HEADS; ++hh)
#pragma unroll
                    for (int s = 0; s < HD / 4; ++s) {
                        const int d = 4 * s + kq;
                        const float b = a.Wqkv[(th * CH + hh * HD + d) * CH + col];
#pragma unroll
                        for (int tt = 0; tt < TT; ++tt) acc[tt] = mfma(L.hd[hh][th][(16 * tt + l15) * HS + d], b, acc[tt]);
                    }
#pragma unroll
            for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                for (int r = 0; r < 4; ++r) B.g[(16 * tt + 4 * kq + r) * RS + col] = acc[tt][r];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {    // the gate's part of dh
            const int e = tid + j * BLOCK;
            if (e >= ACT) continue;
            const int t = e >> 6, c = e & 63;
            float v = B.g[t * RS + c];
#pragma unroll
            for (int h = 0; h < HEADS; ++h) v += a.Wg[h * CH + c] * B.dg[h][t];
            B.g[t * RS + c] = v;
        }
        __syncthreads();
        {   // d_prenorm[c] += sum_t dh[t][c] * tok[t][c] * rinv[t]: lane 4c + q adds tokens q, q + 4, ...
            const int c = tid >> 2, q = tid & 3;
            float v = 0.0f;
            for (int t = q; t < TOK; t += 4) v += B.g[t * RS + c] * (L.tok[t * RS + c] * L.rinv[t]);
            v += __shfl_xor(v, 1, WAVE);
            v += __shfl_xor(v, 2, WAVE);
            p_dpre += v;
        }
        {   // the pre-norm's backward and the skip, four lanes a token; dx's tokens take dy's place
            const int t = tid >> 2, q = tid & 3;
            const bool on = t < TOK;
            const float r = on ? L.rinv[t] : 0.0f;
            float s = 0.0f;
            if (on)
#pragma unroll
                for (int k = 0; k < CH / 4; ++k) {
                    const int c = q + 4 * k;
                    s += (B.g[t * RS + c] * a.pre[c]) * (L.tok[t * RS + c] * r);
                }
            s += __shfl_xor(s, 1, WAVE);
            s += __shfl_xor(s, 2, WAVE);
            s = s / static_cast<float>(CH);
            if (on)
#pragma unroll
                for (int k = 0; k < CH / 4; ++k) {
                    const int c = q + 4 * k;
                    const float u = B.g[t * RS + c] * a.pre[c], hn = L.tok[t * RS + c] * r;
                    B.dy[t * RS + c] = B.dy[t * RS + c] + r * (u - hn * s);
                }
        }
        __syncthreads();
        float *dxs = a.dx + n * ACT;
#pragma unroll
        for (int j = 0; j < PER_LANE; ++j) {
            const int e = tid + j * BLOCK;
            if (e < ACT) dxs[e] = B.dy[token_pos(e, a.token_major)];
        }
        __syncthreads();                        // every image is read to the end before the next sample goes in
    }

    float *row = a.ws + static_cast<size_t>(blockIdx.x) * ROW_FLOATS;
#pragma unroll
    for (int th = 0; th < 3; ++th)
#pragma unroll
        for (int ct = 0; ct < HEADS; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                row[(th * CH + wave * HD + 4 * kq + r) * CH + 16 * ct + l15] = acc_w[th][ct][r];
#pragma unroll
    for (int ct = 0; ct < HEADS; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) row[QKV_NUMEL + (16 * ct + 4 * kq + r) * CH + col] = acc_o[ct][r];
    row[QKV_NUMEL + O_NUMEL + wave * CH + lane] = p_dgate;
    if ((tid & 3) == 0) row[QKV_NUMEL + O_NUMEL + G_NUMEL + (tid >> 2)] = p_dpre;
    p_dqn += __shfl_xor(p_dqn, 16, WAVE);
    p_dqn += __shfl_xor(p_dqn, 32, WAVE);
    p_dkn += __shfl_xor(p_dkn, 16, WAVE);
    p_dkn += __shfl_xor(p_dkn, 32, WAVE);
    if (lane < HD) { B.red[0][wave][lane] = p_dqn; B.red[1][wave][lane] = p_dkn; }
    __syncthreads();
    if (tid < 2 * HD) {
        const int which = tid / HD, d = tid % HD;
        row[QKV_NUMEL + O_NUMEL + G_NUMEL + CH + tid] = ((B.red[which][0][d] + B.red[which][1][d]) + B.red[which][2][d]) + B.red[which][3][d];
    }
}

__global__ void __launch_bounds__(BLOCK) k_attn_reduce(AttnArgs a)
{
    int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= ROW_FLOATS) return;
    float v = 0.0f;
    for (int r = 0; r < a.rows; ++r) v += a.ws[static_cast<size_t>(r) * ROW_FLOATS + i];
    if (i < QKV_NUMEL) { a.d_qkv[i] = v; return; }
    i -= QKV_NUMEL;
    if (i < O_NUMEL) { a.d_o[i] = v; return; }
    i -= O_NUMEL;
    if (i < G_NUMEL) { a.d_gate[i] = v; return; }
    i -= G_NUMEL;
    if (i < CH) { a.d_pre[i] = v; return; }
    i -= CH;
    if (i < HD) a.d_qn[i] = v;
    else a.d_kn[i - HD] = v;
}

}  // namespace
}  // namespace az

using namespace az::host;

namespace {

void attn_inputs(const std::string &w, const az_train_attn_params *p, const float *x, int x_token_major,
                 const uint64_t *keep_bits, float keep_scale, int64_t N, az::AttnArgs &a)
{
    require(n_ok(N), w + ": N must be positive (and at most 2^30)");
    require(p != nullptr, w + ": null argument");
    require(aligned(x, 16) && aligned(p->qkv_weight, 16) && aligned(p->o_weight, 16),
            w + ": x, qkv_weight or o_weight null or not 16-byte aligned");
    require(aligned(p->prenorm_weight, 4) && aligned(p->gate_weight, 4) && aligned(p->q_norm_weight, 4) && aligned(p->k_norm_weight, 4),
            w + ": prenorm_weight, gate_weight, q_norm_weight or k_norm_weight null or misaligned");
    require(keep_bits == nullptr || aligned(keep_bits, 8), w + ": keep_bits not 8-byte aligned");
    require(std::isfinite(keep_scale) && keep_scale >= 1.0f, w + ": keep_scale must be finite and at least 1");
    require(keep_bits != nullptr || keep_scale == 1.0f, w + ": null keep_bits need keep_scale 1");
    require(x_token_major == 0 || x_token_major == 1, w + ": x_token_major must be 0 or 1");
    a.x = x; a.bits = keep_bits; a.keep_scale = keep_scale; a.N = N; a.token_major = x_token_major;
    a.pre = p->prenorm_weight; a.Wqkv = p->qkv_weight; a.Wg = p->gate_weight; a.Wo = p->o_weight;
    a.qn = p->q_norm_weight; a.kn = p->k_norm_weight;
}

}  // namespace

extern "C" {

int64_t az_train_attn_workspace_bytes(int64_t N, int max_workgroups)
{
    if (!n_ok(N) || max_workgroups < 0) return -1;
    return rows_bytes(partition(N, max_workgroups).rows, az::ROW_FLOATS);
}

int az_train_dev_attn_fwd(const az_train_attn_params *params, const float *x, int x_token_major, const uint64_t *keep_bits,
                          float keep_scale, int64_t N, float eps, float *y, void *stream)
{
    return guarded([&] {
        const std::string w("az_train_dev_attn_fwd");
        az::AttnArgs a{};
        attn_inputs(w, params, x, x_token_major, keep_bits, keep_scale, N, a);
        require(eps > 0.0f && std::isfinite(eps), w + ": eps must be positive");
        require(aligned(y, 16), w + ": a null y or one that is not 16-byte aligned");
        a.y = y; a.eps = eps;
        hipLaunchKernelGGL(az::k_attn_fwd, dim3(fwd_grid(N, az::FWD_GRID)), dim3(az::BLOCK), 0, static_cast<hipStream_t>(stream), a);
        HIP_OK(hipGetLastError());
    });
}

int az_train_dev_attn_bwd(const az_train_attn_params *params, const float *x, int x_token_major, const uint64_t *keep_bits,
                          float keep_scale, const float *dy, int64_t N, float eps, int max_workgroups,
                          const az_train_attn_grads *grads, void *stream)
{
    return guarded([&] {
        const std::string w("az_train_dev_attn_bwd");
        az::AttnArgs a{};
        attn_inputs(w, params, x, x_token_major, keep_bits, keep_scale, N, a);
        require(eps > 0.0f && std::isfinite(eps), w + ": eps must be positive");
        require(max_workgroups >= 0, w + ": max_workgroups must not be negative");
        require(grads != nullptr, w + ": null argument");
        require(aligned(dy, 16) && aligned(grads->dx, 16) && aligned(grads->d_qkv_weight, 16) && aligned(grads->d_o_weight, 16) &&
                aligned(grads->workspace, 16), w + ": dy, dx, d_qkv_weight, d_o_weight or workspace null or not 16-byte aligned");
        require(aligned(grads->d_prenorm_weight, 4) && aligned(grads->d_gate_weight, 4) && aligned(grads->d_q_norm_weight, 4) &&
                aligned(grads->d_k_norm_weight, 4), w + ": d_prenorm_weight, d_gate_weight, d_q_norm_weight or d_k_norm_weight null or misaligned");
        const Runs runs = partition(N, max_workgroups);
        a.per = runs.per; a.rows = runs.rows;
        require(grads->workspace_bytes >= rows_bytes(a.rows, az::ROW_FLOATS),
                w + ": a workspace smaller than az_train_attn_workspace_bytes says");
        a.dy = dy; a.eps = eps;
        a.dx = grads->dx; a.d_pre = grads->d_prenorm_weight; a.d_qkv = grads->d_qkv_weight; a.d_gate = grads->d_gate_weight;
        a.d_o = grads->d_o_weight; a.d_qn = grads->d_q_norm_weight; a.d_kn = grads->d_k_norm_weight;
        a.ws = static_cast<float *>(grads->workspace);
        const hipStream_t s = static_cast<hipStream_t>(stream);
        hipLaunchKernelGGL(az::k_attn_bwd, dim3(a.rows), dim3(az::BLOCK), 0, s, a);
        hipLaunchKernelGGL(az::k_attn_reduce, dim3((az::ROW_FLOATS + az::BLOCK - 1) / az::BLOCK), dim3(az::BLOCK), 0, s, a);
        HIP_OK(hipGetLastError());
    });
}

}  // extern "C"
