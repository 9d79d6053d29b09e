// train_heads_kernels.hip - the training forward and backward of the Connect4 heads (az_train_*heads* in az_train.h): the
// column policy head and the WDL value + moves-left head on the tokens [N][42][64] the attention kernel writes; kernels
// and host entry points in this one unit.  float32, 64 channels, token t = 7 * row + col.  The formulas are in the header.
//
// Three kernels, 256 lanes each:
//
//   k_heads_fwd     a workgroup takes samples n = blockIdx, blockIdx + grid, ...  The three 64 x 64 weights sit in LDS with
//                   a row stride of 65 floats for the whole run, so that lane o reading W[o][i] (the product) and lane i
//                   reading W[o][i] (its transpose) both touch 32 different banks; the small parameters sit next to them.
//                   Per sample the 42 tokens go into LDS (row stride 68: the four lanes of a token read channels
//                   sub + 4 j, eight tokens to a half wave, 32 banks).  Four lanes per token form the token's rms factor
//                   and row score; seven lanes the row softmax; all lanes the column features and the 64 x 64 product of
//                   the seven columns (lane = output channel, two columns a wave); wave 0, lane = channel, walks the value
//                   head with its norms as wave sums.  Six barriers a sample.
//   k_heads_bwd     the same forward on a contiguous run of samples, then the backward of both heads: wave 1 the policy
//                   tail, wave 0 the value head, all lanes the transposed products, the three outer-product sums (lane
//                   tid / 4 owns output channel o, inputs 16 (tid % 4) .. + 15: 48 registers) and the tokens' part, whose
//                   d_tokens row leaves through LDS as whole float4s.  A lane keeps its share of the 18 gradient sums in
//                   registers over the run; at the end the per-token shares are added in token order and ONE partial row
//                   (13126 floats, the gradients in parameter order) goes to the caller's workspace.
//   k_heads_reduce  one lane per element adds the rows in row order and stores the element in its gradient.
//
// No atomics, nothing cleared beforehand: two calls on the same inputs give the same bytes.  Sums are chains of fmaf (the
// 64-term products down four interleaved chains).  Plain C++ and vector stores only.
#include "engine_internal.h"

#include "az_train.h"
#include "train_common.h"

namespace az {
namespace {

constexpr int BLOCK = 256;
constexpr int CH = 64, TOK = ROWS * COLS;
constexpr int SAMPLE = TOK * CH;                // 2688 values of a sample's tokens
constexpr int TS = 68;                          // a token's row in LDS
constexpr int WS = 65;                          // a weight's row in LDS
constexpr int SQ = CH * CH;
constexpr int NPARAM = 18;
constexpr int FWD_GRID = 512;

// the parameters in the order of az_train_heads_params, and where each one's gradient sits in a partial row
enum { P_NORM, P_GATE_W, P_GATE_B, P_FC_W, P_FC_B, P_OUT_W, P_OUT_B, D_POOL_NORM, D_POOL_W, D_POOL_B, D_NORM, D_FC_W, D_FC_B,
       D_OUT_NORM, D_VAL_W, D_VAL_B, D_AUX_W, D_AUX_B };
constexpr int numel_of(int k)
{
    return k == P_FC_W || k == D_POOL_W || k == D_FC_W ? SQ : k == P_GATE_B || k == P_OUT_B || k == D_AUX_B ? 1 :
           k == D_VAL_W ? 3 * CH : k == D_VAL_B ? 3 : CH;
}
constexpr int offset_of(int k) { return k == 0 ? 0 : offset_of(k - 1) + numel_of(k - 1); }
template <int K> constexpr int OFF = offset_of(K);      // a compile-time constant wherever a kernel names it
constexpr int ROW_USED = offset_of(NPARAM);     // 13126
constexpr int ROW_FLOATS = (ROW_USED + 3) / 4 * 4;
static_assert(ROW_USED == 13126 && ROW_FLOATS == 13128, "the partial row is part of the ABI");
static_assert(sizeof(az_train_heads_params) == NPARAM * sizeof(void *), "eighteen parameters");

// the 64-vectors and the scalars among the parameters, as LDS holds them
enum { V_PNORM, V_GATE, V_PFCB, V_OUTW, V_POOLNORM, V_POOLB, V_NORM, V_FCB, V_OUTNORM, V_VAL0, V_VAL1, V_VAL2, V_AUX, NVEC };
enum { SC_GATE_B, SC_OUT_B, SC_VAL_B, SC_AUX_B = SC_VAL_B + 3, NSC = 8 };

struct HeadsArgs {
    const float *p[NPARAM];
    const float *tokens, *keep_policy, *keep_pool, *d_log_p, *d_value, *d_steps;
    const uint8_t *legal;
    float *log_p, *value, *steps, *d_tokens, *ws;
    float *g[NPARAM];
    int64_t N, per;                             // per: the run of samples a backward workgroup walks
    int rows;                                   // backward workgroups = partial rows
    float eps;
};

struct Shared {
    alignas(16) float W[3][CH * WS];            // policy fc, pool_fc, dual fc
    alignas(16) float tok[TOK * TS];
    alignas(16) float vec[NVEC][CH];
    alignas(16) float colf[8][CH], u[8][CH], a[8][CH], du[8][CH], dcolf[8][CH];
    alignas(16) float pn[CH], hn[CH], dz1[CH], dz2[CH], dmv[CH];
    float r[CH], s[CH], w[CH], dwv[CH];
    float sc[NSC], logit[8], logp[8];
};

// what wave 0, lane = channel, keeps of the value head between the passes
struct Val {
    float m, mn, rp, z1, kp, x1, x1n, rn, z2, gn, ro, h, value[3], steps;
};

__device__ __forceinline__ float rinv(float sum_sq, float eps) { return 1.0f / sqrtf(sum_sq * (1.0f / CH) + eps); }

// Over the wavefront as a __shfl_xor butterfly, every lane its own total.  NOT nn_common.h's wave_sum (a DPP chain read from
// lane 63): that one adds in another order and gives other bits, so this file does not include it and the name differs.
__device__ __forceinline__ float butterfly_sum(float v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ float quad_sum(float v)
{
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    return v;
}

// sum_i w[i * stride] * x[i] over 64 terms, four interleaved chains; x is read as float4 (the same address in every lane)
__device__ __forceinline__ float dot64(const float *w, int stride, const float *x)
{
    float part[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
    for (int i = 0; i < CH; i += 4) {
        const float4 xv = *reinterpret_cast<const float4 *>(x + i);
        part[0] = fmaf(w[(i + 0) * stride], xv.x, part[0]);
        part[1] = fmaf(w[(i + 1) * stride], xv.y, part[1]);
        part[2] = fmaf(w[(i + 2) * stride], xv.z, part[2]);
        part[3] = fmaf(w[(i + 3) * stride], xv.w, part[3]);
    }
    return (part[0] + part[1]) + (part[2] + part[3]);
}

__device__ __forceinline__ void load_params(const HeadsArgs &a, Shared &S)
{
    const int tid = threadIdx.x;
    for (int e = tid; e < SQ; e += BLOCK) {
        const int at = (e >> 6) * WS + (e & 63);
        S.W[0][at] = a.p[P_FC_W][e];
        S.W[1][at] = a.p[D_POOL_W][e];
        S.W[2][at] = a.p[D_FC_W][e];
    }
    if (tid < CH) {
        S.vec[V_PNORM][tid] = a.p[P_NORM][tid];
        S.vec[V_GATE][tid] = a.p[P_GATE_W][tid];
        S.vec[V_PFCB][tid] = a.p[P_FC_B][tid];
        S.vec[V_OUTW][tid] = a.p[P_OUT_W][tid];
        S.vec[V_POOLNORM][tid] = a.p[D_POOL_NORM][tid];
        S.vec[V_POOLB][tid] = a.p[D_POOL_B][tid];
        S.vec[V_NORM][tid] = a.p[D_NORM][tid];
        S.vec[V_FCB][tid] = a.p[D_FC_B][tid];
        S.vec[V_OUTNORM][tid] = a.p[D_OUT_NORM][tid];
        S.vec[V_VAL0][tid] = a.p[D_VAL_W][tid];
        S.vec[V_VAL1][tid] = a.p[D_VAL_W][CH + tid];
        S.vec[V_VAL2][tid] = a.p[D_VAL_W][2 * CH + tid];
        S.vec[V_AUX][tid] = a.p[D_AUX_W][tid];
    }
    if (tid == 0) {
        S.sc[SC_GATE_B] = a.p[P_GATE_B][0];
        S.sc[SC_OUT_B] = a.p[P_OUT_B][0];
        S.sc[SC_VAL_B] = a.p[D_VAL_B][0];
        S.sc[SC_VAL_B + 1] = a.p[D_VAL_B][1];
        S.sc[SC_VAL_B + 2] = a.p[D_VAL_B][2];
        S.sc[SC_AUX_B] = a.p[D_AUX_B][0];
    }
}

// Both heads of sample n.  Left in LDS: tok, r, w, colf, u, a, logp, pn, hn; in wave 0's registers: v.  Ends behind a
// barrier; the caller has one between its last use of LDS and the next call.
__device__ __forceinline__ void forward_sample(const HeadsArgs &a, Shared &S, int64_t n, Val &v)
{
    const int tid = threadIdx.x;
    const int t = tid >> 2, sub = tid & 3;
    const bool live = t < TOK;
    const int tt = live ? t : 0;                // the lanes past the last token read token 0 and store nothing

    const float4 *src = reinterpret_cast<const float4 *>(a.tokens + n * SAMPLE);
    for (int e = tid; e < SAMPLE / 4; e += BLOCK)
        *reinterpret_cast<float4 *>(&S.tok[(e >> 4) * TS + 4 * (e & 15)]) = src[e];
    __syncthreads();

    {   // a token's rms factor and row score: four lanes a token
        float x[16], ss = 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            x[j] = S.tok[tt * TS + sub + 4 * j];
            ss = fmaf(x[j], x[j], ss);
        }
        const float r = rinv(quad_sum(ss), a.eps);
        float score = 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = sub + 4 * j;
            score = fmaf((x[j] * r) * S.vec[V_PNORM][c], S.vec[V_GATE][c], score);
        }
        score = quad_sum(score) + S.sc[SC_GATE_B];
        if (live && sub == 0) {
            S.r[t] = r;
            S.s[t] = score;
        }
    }
    if (tid < CH) {                             // the mean token and its pool norm
        float sum = 0.0f;
        for (int k = 0; k < TOK; ++k) sum += S.tok[k * TS + tid];
        v.m = sum / static_cast<float>(TOK);
        v.rp = rinv(butterfly_sum(v.m * v.m), a.eps);
        v.mn = v.m * v.rp;
        S.pn[tid] = v.mn * S.vec[V_POOLNORM][tid];
    }
    __syncthreads();

    if (tid >= CH && tid < CH + COLS) {         // the softmax over a column's six rows, its maximum taken out
        const int c = tid - CH;
        float sv[ROWS], mx = S.s[c];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            sv[r] = S.s[COLS * r + c];
            mx = fmaxf(mx, sv[r]);
        }
        float sum = 0.0f;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            sv[r] = expf(sv[r] - mx);
            sum += sv[r];
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) S.w[COLS * r + c] = sv[r] / sum;
    }
    if (tid < CH) {
        v.z1 = dot64(&S.W[1][tid * WS], 1, S.pn) + S.vec[V_POOLB][tid];
        v.kp = a.keep_pool != nullptr ? a.keep_pool[n * CH + tid] : 1.0f;
        v.x1 = v.m + v.kp * (v.z1 * sigmoid(v.z1));
        v.rn = rinv(butterfly_sum(v.x1 * v.x1), a.eps);
        v.x1n = v.x1 * v.rn;
        S.hn[tid] = v.x1n * S.vec[V_NORM][tid];
    }
    __syncthreads();

    for (int e = tid; e < COLS * CH; e += BLOCK) {      // the column features
        const int c = e >> 6, i = e & 63;
        const float nw = S.vec[V_PNORM][i];
        float acc = 0.0f;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            const int k = COLS * r + c;
            acc = fmaf(S.w[k], (S.tok[k * TS + i] * S.r[k]) * nw, acc);
        }
        S.colf[c][i] = acc;
    }
    if (tid < CH) {
        v.z2 = dot64(&S.W[2][tid * WS], 1, S.hn) + S.vec[V_FCB][tid];
        const float g = v.z2 * sigmoid(v.z2);
        v.ro = rinv(butterfly_sum(g * g), a.eps);
        v.gn = g * v.ro;
        v.h = v.gn * S.vec[V_OUTNORM][tid];
        float zv[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) zv[j] = butterfly_sum(v.h * S.vec[V_VAL0 + j][tid]) + S.sc[SC_VAL_B + j];
        const float mx = fmaxf(fmaxf(zv[0], zv[1]), zv[2]);
        const float lse = logf((expf(zv[0] - mx) + expf(zv[1] - mx)) + expf(zv[2] - mx));
#pragma unroll
        for (int j = 0; j < 3; ++j) v.value[j] = (zv[j] - mx) - lse;
        v.steps = sigmoid(butterfly_sum(v.h * S.vec[V_AUX][tid]) + S.sc[SC_AUX_B]);
    }
    __syncthreads();

    {   // the columns' 64 x 64 product, SiLU, keep, and the logit: lane = output channel, wave g takes columns g and g + 4
        const int o = tid & 63;
        for (int c = tid >> 6; c < COLS; c += BLOCK / CH) {
            const float u = dot64(&S.W[0][o * WS], 1, S.colf[c]) + S.vec[V_PFCB][o];
            const float keep = a.keep_policy != nullptr ? a.keep_policy[(n * COLS + c) * CH + o] : 1.0f;
            const float act = (u * sigmoid(u)) * keep;
            S.u[c][o] = u;
            S.a[c][o] = act;
            const float logit = butterfly_sum(act * S.vec[V_OUTW][o]) + S.sc[SC_OUT_B];
            if (o == 0) S.logit[c] = (a.legal == nullptr || a.legal[n * COLS + c] != 0) ? logit : -1e9f;
        }
    }
    __syncthreads();

    if (tid < COLS) {                           // the log-softmax over the seven columns, the maximum taken out
        float mx = S.logit[0];
#pragma unroll
        for (int k = 1; k < COLS; ++k) mx = fmaxf(mx, S.logit[k]);
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < COLS; ++k) sum += expf(S.logit[k] - mx);
        S.logp[tid] = (S.logit[tid] - mx) - logf(sum);
    }
    __syncthreads();
}

__global__ void __launch_bounds__(BLOCK) k_heads_fwd(HeadsArgs a)
{
    __shared__ Shared S;
    const int tid = threadIdx.x;
    load_params(a, S);
    __syncthreads();
    for (int64_t n = blockIdx.x; n < a.N; n += gridDim.x) {
        Val v;
        forward_sample(a, S, n, v);
        if (tid < COLS) a.log_p[n * COLS + tid] = S.logp[tid];
        if (tid < 3) a.value[n * 3 + tid] = tid == 0 ? v.value[0] : tid == 1 ? v.value[1] : v.value[2];
        if (tid == 0) a.steps[n] = v.steps;
        // logp is written again only behind the next sample's barriers
    }
}

__global__ void __launch_bounds__(BLOCK) k_heads_bwd(HeadsArgs a)
{
    __shared__ Shared S;
    const int tid = threadIdx.x;
    const int t = tid >> 2, sub = tid & 3;
    const bool live = t < TOK;
    const int tt = live ? t : 0, col = tt % COLS;
    const int oo = tid >> 2, i0 = 16 * (tid & 3);       // this lane's piece of the three outer products
    load_params(a, S);
    __syncthreads();

    float accP[16], accQ[16], accF[16];         // d policy fc, d pool_fc, d dual fc: [oo][i0 ..]
    float accGW[16], accNW[16], accGB = 0.0f;   // this token's share of d row_gate.weight, d norm.weight (policy), d row_gate.bias
#pragma unroll
    for (int k = 0; k < 16; ++k) accP[k] = accQ[k] = accF[k] = accGW[k] = accNW[k] = 0.0f;
    // wave 0, lane = channel: the value head's vectors; wave 1, lane = 64 + channel: the policy tail's
    float aPoolNorm = 0.0f, aPoolB = 0.0f, aNorm = 0.0f, aFcB = 0.0f, aOutNorm = 0.0f, aVal[3] = {0.0f, 0.0f, 0.0f}, aAux = 0.0f;
    float aValB[3] = {0.0f, 0.0f, 0.0f}, aAuxB = 0.0f;
    float aOutW = 0.0f, aPfcB = 0.0f, aOutB = 0.0f;

    const int64_t n0 = static_cast<int64_t>(blockIdx.x) * a.per;
    const int64_t n1 = n0 + a.per < a.N ? n0 + a.per : a.N;
    for (int64_t n = n0; n < n1; ++n) {
        Val v;
        forward_sample(a, S, n, v);

        float dx1 = 0.0f;
        if (tid < CH) {                         // the value head from its outputs down to dz2
            const float dv0 = a.d_value[n * 3], dv1 = a.d_value[n * 3 + 1], dv2 = a.d_value[n * 3 + 2];
            const float sdv = (dv0 + dv1) + dv2;
            const float dzv[3] = {dv0 - expf(v.value[0]) * sdv, dv1 - expf(v.value[1]) * sdv, dv2 - expf(v.value[2]) * sdv};
            const float dza = a.d_steps[n] * v.steps * (1.0f - v.steps);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                aVal[j] = fmaf(dzv[j], v.h, aVal[j]);
                aValB[j] += dzv[j];
            }
            aAux = fmaf(dza, v.h, aAux);
            aAuxB += dza;
            float dh = S.vec[V_VAL0][tid] * dzv[0];
            dh = fmaf(S.vec[V_VAL1][tid], dzv[1], dh);
            dh = fmaf(S.vec[V_VAL2][tid], dzv[2], dh);
            dh = fmaf(S.vec[V_AUX][tid], dza, dh);
            aOutNorm = fmaf(dh, v.gn, aOutNorm);
            const float gw = dh * S.vec[V_OUTNORM][tid];
            const float mean = butterfly_sum(gw * v.gn) * (1.0f / CH);
            const float dz2 = (v.ro * (gw - v.gn * mean)) * dsilu(v.z2);
            aFcB += dz2;
            S.dz2[tid] = dz2;
        } else if (tid < 2 * CH) {              // the policy tail: d_logit, d out, du
            const int o = tid - CH;
            float dlp[COLS], sum = 0.0f;
#pragma unroll
            for (int c = 0; c < COLS; ++c) {
                dlp[c] = a.d_log_p[n * COLS + c];
                sum += dlp[c];                  // over ALL seven entries, the illegal ones too
            }
            const float ow = S.vec[V_OUTW][o];
#pragma unroll
            for (int c = 0; c < COLS; ++c) {
                const bool legal = a.legal == nullptr || a.legal[n * COLS + c] != 0;
                const float dl = legal ? dlp[c] - expf(S.logp[c]) * sum : 0.0f;
                aOutB += dl;
                aOutW = fmaf(dl, S.a[c][o], aOutW);
                const float keep = a.keep_policy != nullptr ? a.keep_policy[(n * COLS + c) * CH + o] : 1.0f;
                const float du = ((dl * ow) * keep) * dsilu(S.u[c][o]);
                aPfcB += du;
                S.du[c][o] = du;
            }
        }
        __syncthreads();

#pragma unroll
        for (int c = 0; c < COLS; ++c) {        // d policy fc += du (x) colf
            const float d = S.du[c][oo];
#pragma unroll
            for (int k = 0; k < 16; k += 4) {
                const float4 x = *reinterpret_cast<const float4 *>(&S.colf[c][i0 + k]);
                accP[k] = fmaf(d, x.x, accP[k]);
                accP[k + 1] = fmaf(d, x.y, accP[k + 1]);
                accP[k + 2] = fmaf(d, x.z, accP[k + 2]);
                accP[k + 3] = fmaf(d, x.w, accP[k + 3]);
            }
        }
        {                                       // d dual fc += dz2 (x) hn
            const float d = S.dz2[oo];
#pragma unroll
            for (int k = 0; k < 16; ++k) accF[k] = fmaf(d, S.hn[i0 + k], accF[k]);
        }
        {                                       // dcolf = fc_w^T du: lane = input channel, wave g takes columns g and g + 4
            const int i = tid & 63;
            for (int c = tid >> 6; c < COLS; c += BLOCK / CH) S.dcolf[c][i] = dot64(&S.W[0][i], WS, S.du[c]);
        }
        if (tid < CH) {                         // through the dual fc and its norm to dx1, then dz1
            const float dhn = dot64(&S.W[2][tid], WS, S.dz2);
            aNorm = fmaf(dhn, v.x1n, aNorm);
            const float gw = dhn * S.vec[V_NORM][tid];
            const float mean = butterfly_sum(gw * v.x1n) * (1.0f / CH);
            dx1 = v.rn * (gw - v.x1n * mean);
            const float dz1 = (dx1 * v.kp) * dsilu(v.z1);
            aPoolB += dz1;
            S.dz1[tid] = dz1;
        }
        __syncthreads();

        {                                       // d pool_fc += dz1 (x) pn
            const float d = S.dz1[oo];
#pragma unroll
            for (int k = 0; k < 16; ++k) accQ[k] = fmaf(d, S.pn[i0 + k], accQ[k]);
        }
        float x[16];                            // this lane's 16 values of its token, normalised: vn = tok * r
        const float r = S.r[tt];
        {                                       // dw[t] = dcolf[col] . xn[t]
            float part = 0.0f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int c = sub + 4 * j;
                x[j] = S.tok[tt * TS + c] * r;
                part = fmaf(S.dcolf[col][c], x[j] * S.vec[V_PNORM][c], part);
            }
            part = quad_sum(part);
            if (live && sub == 0) S.dwv[t] = part;
        }
        if (tid < CH) {                         // through pool_fc and the pool norm to the mean token's gradient
            const float dpn = dot64(&S.W[1][tid], WS, S.dz1);
            aPoolNorm = fmaf(dpn, v.mn, aPoolNorm);
            const float gw = dpn * S.vec[V_POOLNORM][tid];
            const float mean = butterfly_sum(gw * v.mn) * (1.0f / CH);
            const float dm = dx1 + v.rp * (gw - v.mn * mean);
            S.dmv[tid] = dm / static_cast<float>(TOK);
        }
        __syncthreads();

        {                                       // the row softmax, the row gate and the policy norm of this lane's token
            const float wt = S.w[tt];
            float inner = 0.0f;
#pragma unroll
            for (int rr = 0; rr < ROWS; ++rr) inner = fmaf(S.w[COLS * rr + col], S.dwv[COLS * rr + col], inner);
            const float ds = wt * (S.dwv[tt] - inner);
            float gwn[16], part = 0.0f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int c = sub + 4 * j;
                const float nw = S.vec[V_PNORM][c];
                const float dxn = fmaf(wt, S.dcolf[col][c], ds * S.vec[V_GATE][c]);
                if (live) {
                    accGW[j] = fmaf(ds, x[j] * nw, accGW[j]);
                    accNW[j] = fmaf(dxn, x[j], accNW[j]);
                }
                gwn[j] = dxn * nw;
                part = fmaf(gwn[j], x[j], part);
            }
            if (live) accGB += ds;
            const float mean = quad_sum(part) * (1.0f / CH);
            if (live) {
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int c = sub + 4 * j;
                    S.tok[t * TS + c] = r * (gwn[j] - x[j] * mean) + S.dmv[c];      // only this lane reads these 16
                }
            }
        }
        __syncthreads();

        float4 *dst = reinterpret_cast<float4 *>(a.d_tokens + n * SAMPLE);
        for (int e = tid; e < SAMPLE / 4; e += BLOCK)
            dst[e] = *reinterpret_cast<const float4 *>(&S.tok[(e >> 4) * TS + 4 * (e & 15)]);
        __syncthreads();                        // the next sample's tokens go in behind this
    }

    // the partial row
    float *row = a.ws + static_cast<size_t>(blockIdx.x) * ROW_FLOATS;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        row[OFF<P_FC_W> + oo * CH + i0 + k] = accP[k];
        row[OFF<D_POOL_W> + oo * CH + i0 + k] = accQ[k];
        row[OFF<D_FC_W> + oo * CH + i0 + k] = accF[k];
    }
    if (tid < CH) {
        row[OFF<D_POOL_NORM> + tid] = aPoolNorm;
        row[OFF<D_POOL_B> + tid] = aPoolB;
        row[OFF<D_NORM> + tid] = aNorm;
        row[OFF<D_FC_B> + tid] = aFcB;
        row[OFF<D_OUT_NORM> + tid] = aOutNorm;
#pragma unroll
        for (int j = 0; j < 3; ++j) row[OFF<D_VAL_W> + j * CH + tid] = aVal[j];
        row[OFF<D_AUX_W> + tid] = aAux;
        if (tid == 0) {
#pragma unroll
            for (int j = 0; j < 3; ++j) row[OFF<D_VAL_B> + j] = aValB[j];
            row[OFF<D_AUX_B>] = aAuxB;
        }
    } else if (tid < 2 * CH) {
        row[OFF<P_OUT_W> + tid - CH] = aOutW;
        row[OFF<P_FC_B> + tid - CH] = aPfcB;
        if (tid == CH) row[OFF<P_OUT_B>] = aOutB;
    }
    // the per-token shares, added in token order through the tokens' place in LDS (free behind the walk's last barrier)
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        if (live) {
#pragma unroll
            for (int j = 0; j < 16; ++j) S.tok[t * TS + sub + 4 * j] = pass == 0 ? accGW[j] : accNW[j];
            if (pass == 0 && sub == 0) S.dwv[t] = accGB;
        }
        __syncthreads();
        if (tid < CH) {
            float sum = 0.0f;
            for (int k = 0; k < TOK; ++k) sum += S.tok[k * TS + tid];
            row[(pass == 0 ? OFF<P_GATE_W> : OFF<P_NORM>) + tid] = sum;
        } else if (pass == 0 && tid == CH) {
            float sum = 0.0f;
            for (int k = 0; k < TOK; ++k) sum += S.dwv[k];
            row[OFF<P_GATE_B>] = sum;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(BLOCK) k_heads_reduce(HeadsArgs a)
{
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= ROW_USED) return;
    float v = 0.0f;
    for (int r = 0; r < a.rows; ++r) v += a.ws[static_cast<size_t>(r) * ROW_FLOATS + i];
    int k = 0, at = 0;
    while (i >= at + numel_of(k)) at += numel_of(k++);
    a.g[k][i - at] = v;
}

}  // namespace
}  // namespace az

using namespace az::host;

namespace {

// which of the eighteen tensors are the 64 x 64 ones: 16-byte aligned, the rest 4-byte
bool heads_square(int k) { return k == az::P_FC_W || k == az::D_POOL_W || k == az::D_FC_W; }

void heads_inputs(const std::string &w, const az_train_heads_params *p, const float *tokens, const float *keep_policy,
                  const float *keep_pool, int64_t N, float eps, az::HeadsArgs &a)
{
    require(n_ok(N), w + ": N must be positive (and at most 2^30)");
    require(p != nullptr, w + ": null argument");
    require(eps > 0.0f && std::isfinite(eps), w + ": eps must be positive and finite");
    require(aligned(tokens, 16), w + ": null tokens or tokens that are not 16-byte aligned");
    require((keep_policy == nullptr || aligned(keep_policy, 16)) && (keep_pool == nullptr || aligned(keep_pool, 16)),
            w + ": keep_policy or keep_pool not 16-byte aligned");
    const float *const *ptr = reinterpret_cast<const float *const *>(p);
    for (int k = 0; k < az::NPARAM; ++k) {
        require(aligned(ptr[k], heads_square(k) ? 16 : 4), w + ": a parameter null or misaligned (the 64 x 64 weights: 16 bytes, the rest: 4)");
        a.p[k] = ptr[k];
    }
    a.tokens = tokens; a.keep_policy = keep_policy; a.keep_pool = keep_pool; a.N = N; a.eps = eps;
}

}  // namespace

extern "C" {

int64_t az_train_heads_workspace_bytes(int64_t N, int max_workgroups)
{
    if (!n_ok(N) || max_workgroups < 0) return -1;
    return rows_bytes(partition(N, max_workgroups).rows, az::ROW_FLOATS);
}

int az_train_dev_heads_fwd(const az_train_heads_params *params, const float *tokens, const uint8_t *legal,
                           const float *keep_policy, const float *keep_pool, int64_t N, float eps,
                           float *log_p, float *value, float *steps, void *stream)
{
    return guarded([&] {
        const std::string w("az_train_dev_heads_fwd");
        az::HeadsArgs a{};
        heads_inputs(w, params, tokens, keep_policy, keep_pool, N, eps, a);
        require(aligned(log_p, 4) && aligned(value, 4) && aligned(steps, 4), w + ": log_p, value or steps null or misaligned");
        a.legal = legal; a.log_p = log_p; a.value = value; a.steps = steps;
        hipLaunchKernelGGL(az::k_heads_fwd, dim3(fwd_grid(N, az::FWD_GRID)), dim3(az::BLOCK), 0, static_cast<hipStream_t>(stream), a);
        HIP_OK(hipGetLastError());
    });
}

int az_train_dev_heads_bwd(const az_train_heads_params *params, const float *tokens, const uint8_t *legal,
                           const float *keep_policy, const float *keep_pool,
                           const float *d_log_p, const float *d_value, const float *d_steps,
                           int64_t N, float eps, int max_workgroups, const az_train_heads_grads *grads, void *stream)
{
    return guarded([&] {
        const std::string w("az_train_dev_heads_bwd");
        az::HeadsArgs a{};
        heads_inputs(w, params, tokens, keep_policy, keep_pool, N, eps, a);
        require(max_workgroups >= 0, w + ": max_workgroups must not be negative");
        require(grads != nullptr, w + ": null argument");
        require(aligned(d_log_p, 4) && aligned(d_value, 4) && aligned(d_steps, 4), w + ": d_log_p, d_value or d_steps null or misaligned");
        require(aligned(grads->d_tokens, 16) && aligned(grads->workspace, 16), w + ": d_tokens or workspace null or not 16-byte aligned");
        float *const *ptr = &grads->d_policy_norm_weight;
        for (int k = 0; k < az::NPARAM; ++k) {
            require(aligned(ptr[k], heads_square(k) ? 16 : 4), w + ": a gradient null or misaligned (the 64 x 64 ones: 16 bytes, the rest: 4)");
            a.g[k] = ptr[k];
        }
        const Runs runs = partition(N, max_workgroups);
        a.per = runs.per; a.rows = runs.rows;
        require(grads->workspace_bytes >= rows_bytes(a.rows, az::ROW_FLOATS), w + ": a workspace smaller than az_train_heads_workspace_bytes says");
        a.legal = legal; a.d_log_p = d_log_p; a.d_value = d_value; a.d_steps = d_steps;
        a.d_tokens = grads->d_tokens; a.ws = static_cast<float *>(grads->workspace);
        const hipStream_t s = static_cast<hipStream_t>(stream);
        hipLaunchKernelGGL(az::k_heads_bwd, dim3(a.rows), dim3(az::BLOCK), 0, s, a);
        hipLaunchKernelGGL(az::k_heads_reduce, dim3((az::ROW_USED + az::BLOCK - 1) / az::BLOCK), dim3(az::BLOCK), 0, s, a);
        HIP_OK(hipGetLastError());
    });
}

}  // extern "C"
