// train_kernels.hip - the learner's loss side: the training losses of one batch and their gradients with respect to the
// network's three head outputs (az_train_dev_loss and az_train_dev_loss_grad in az_train.h), kernels and host entry
// points in this one unit.  What the reference does in 60 to 100 element-wise launches forward and as many backward
// (src/environments/NetworkBase.py:30-192) is three launches:
//
//   k_train_loss    one lane group per sample - 8 lanes for Connect4 (lane a owns action a), a wavefront for Othello
//                   (lane a owns action a, the pass rides with lane 0).  Per-sample sums over the actions go through
//                   sum8 / wave_sum (nn_common.h); the per-sample scalars (value, distillation, td, aux: three or
//                   fewer entries each) are computed by every lane of the group.  A block is one wavefront; it walks
//                   a contiguous run of groups and leaves ONE row of partial sums and counts in the workspace.
//   k_train_reduce  one wavefront adds the rows in a fixed order (lane l takes rows l, l + 64, ...; then the
//                   wavefront's DPP sum), forms the batch means and the value mixing and writes losses[4] and
//                   counts[11].
//   k_train_grad    the same mapping as k_train_loss; every sample's gradients need only its own data, the three
//                   upstream scalars and the td row count that k_train_reduce left in counts[10].
//
// No LDS, no atomics: the counts are partial rows too, so the workspace needs no clearing.  Two calls on the same
// inputs give the same bytes.  Plain C++ and vector stores only.
#include "engine_internal.h"

#include "az_train.h"
#include "nn_common.h"

namespace az {
namespace {

constexpr int WAVE = 64;
constexpr int MAX_ROWS = 2048;          // partial rows (= blocks of k_train_loss) at most
constexpr int ROW_WORDS = 20;           // 7 float sums, 11 counts, 2 spare
enum { S_KL = 0, S_HM, S_H, S_VB, S_DIST, S_TD, S_AUX, N_SUMS };
constexpr int N_COUNTS = 11;            // confusion[3][3], policy rows, td rows
constexpr int C_POLICY = 9, C_TD = 10;
static_assert(N_SUMS + N_COUNTS <= ROW_WORDS, "a partial row holds the sums and the counts");

// What the kernels read.  The scalars a Python double enters the reference's float32 arithmetic with are rounded
// once, on the host, from the double expression (NetworkBase.py multiplies tensors by Python floats).
struct TrainArgs {
    const float *state, *prob, *root_wdl, *future_root_wdl;
    const int8_t *winner;
    const int16_t *steps_to_end, *aux_target;
    const float *log_p, *value, *steps;
    int64_t N;
    int64_t groups, per_block;          // lane groups in all, and the run of groups one block walks
    int rows;                           // blocks of k_train_loss = partial rows
    float value_decay, third;           // third: 1 / 3 rounded
    float distill_alpha, one_m_distill, distill_temp, distill_t2;
    float psw_beta, entropy_lambda;
    float td_alpha, one_m_td, td_keep, td_flat;      // target = td_keep * t + td_flat when value_decay < 1
    int td_steps;
    float aux_offset;
    bool soft, distill, psw, entropy, td;
    // outputs
    uint32_t *partials;                 // [rows][ROW_WORDS]
    float *losses;
    int32_t *counts;
    const float *upstream;
    float *d_log_p, *d_value, *d_steps;
};

template <class G> __device__ __forceinline__ float group_sum(float v)
{
    if constexpr (G::LANES == 8) return sum8(v);
    else return wave_sum(v);
}

__device__ __forceinline__ float xlogx(float t) { return t > 0.0f ? t * logf(t) : 0.0f; }

// [draw, p1, p2] -> [draw, win, loss] of the side to move
__device__ __forceinline__ void relative(const float *wdl, bool plus, float r[3])
{
    r[0] = wdl[0];
    r[1] = plus ? wdl[1] : wdl[2];
    r[2] = plus ? wdl[2] : wdl[1];
}

// One sample as one lane of its group sees it: the derived quantities, the per-action pieces of this lane and the
// per-sample scalars.  Everything both passes need, so that they cannot drift apart.
struct Sample {
    int cls, pred;
    float mask;                 // 0 / 1
    float kl, weight, H;        // policy: group sums, uniform in the group
    float p[2], lp[2], pe[2];   // this lane's action, and the tail action (Othello's pass, lane 0 only)
    float v[3], z[3];
    float vb;                   // -sum z v
    float has_q, t[3], sm[3], tsum, dist;       // distillation: teacher, student softmax, sum of the teacher, KL
    bool counted;               // td row
    float ft[3], tdkl;
    float diff, aux;
};

template <class G>
__device__ __forceinline__ void load_sample(const TrainArgs &a, size_t n, int act, bool live, Sample &s)
{
    constexpr int A = G::ACTIONS, AL = A < WAVE ? A : WAVE;
    constexpr bool TAIL = A > WAVE;
    const bool plus = a.state[n * (3 * G::CELLS) + 2 * G::CELLS] >= 0.0f;
    const int sign = plus ? 1 : -1;
    const int win = a.winner[n];
    s.cls = win == 0 ? 0 : (win == sign ? 1 : 2);
    const int st = a.steps_to_end[n];

    // ---- policy
    const bool own = live && act < AL;
    const bool tail = TAIL && live && act == 0;
    s.p[0] = own ? a.prob[n * A + act] : 0.0f;
    s.lp[0] = own ? a.log_p[n * A + act] : 0.0f;
    s.p[1] = tail ? a.prob[n * A + A - 1] : 0.0f;
    s.lp[1] = tail ? a.log_p[n * A + A - 1] : 0.0f;
    float psum = 0.0f, kl = 0.0f, plogp = 0.0f;
#pragma unroll
    for (int j = 0; j < (TAIL ? 2 : 1); ++j) {
        const bool on = j == 0 ? own : tail;
        s.pe[j] = on ? expf(s.lp[j]) : 0.0f;
        psum += s.p[j];
        kl += s.p[j] != 0.0f ? s.p[j] * logf(s.p[j]) - s.p[j] * s.lp[j] : 0.0f;
        plogp += s.pe[j] != 0.0f ? s.pe[j] * s.lp[j] : 0.0f;
    }
    s.mask = group_sum<G>(psum) > 0.0f ? 1.0f : 0.0f;
    s.kl = group_sum<G>(kl);
    s.H = -group_sum<G>(plogp);
    s.weight = a.psw ? 1.0f + a.psw_beta * s.kl : 1.0f;

    // ---- value
#pragma unroll
    for (int i = 0; i < 3; ++i) s.v[i] = a.value[n * 3 + i];
    s.pred = s.v[1] > s.v[0] ? (s.v[2] > s.v[1] ? 2 : 1) : (s.v[2] > s.v[0] ? 2 : 0);
    if (a.soft) {
        const float d = powf(a.value_decay, static_cast<float>(st));
        const float flat = (1.0f - d) * a.third;
#pragma unroll
        for (int i = 0; i < 3; ++i) s.z[i] = d * (i == s.cls ? 1.0f : 0.0f) + flat;
        s.vb = -((s.z[0] * s.v[0] + s.z[1] * s.v[1]) + s.z[2] * s.v[2]);
    } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) s.z[i] = i == s.cls ? 1.0f : 0.0f;
        s.vb = -(s.cls == 0 ? s.v[0] : s.cls == 1 ? s.v[1] : s.v[2]);
    }

    // ---- distillation towards the root's WDL
    s.has_q = 0.0f; s.dist = 0.0f; s.tsum = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) s.t[i] = s.sm[i] = 0.0f;
    if (a.distill) {
        float w[3], rel[3], tl[3], sv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = a.root_wdl[n * 3 + i];
        relative(w, plus, rel);
        s.has_q = (rel[0] + rel[1]) + rel[2] > 0.0f ? 1.0f : 0.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            tl[i] = logf(fmaxf(rel[i], 1e-8f)) / a.distill_temp;
            sv[i] = s.v[i] / a.distill_temp;
        }
        const float mt = fmaxf(fmaxf(tl[0], tl[1]), tl[2]), ms = fmaxf(fmaxf(sv[0], sv[1]), sv[2]);
        float et[3], es[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) { et[i] = expf(tl[i] - mt); es[i] = expf(sv[i] - ms); }
        const float st_sum = (et[0] + et[1]) + et[2], ss_sum = (es[0] + es[1]) + es[2];
        const float lse = logf(ss_sum);
        float klq = 0.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            s.t[i] = et[i] / st_sum;
            s.sm[i] = es[i] / ss_sum;
            klq += xlogx(s.t[i]) - s.t[i] * ((sv[i] - ms) - lse);
        }
        s.tsum = (s.t[0] + s.t[1]) + s.t[2];
        s.dist = klq * s.has_q;
    }

    // ---- n-step consistency with the later root's WDL
    s.counted = false; s.tdkl = 0.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) s.ft[i] = 0.0f;
    if (a.td) {
        float w[3], rel[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = a.future_root_wdl[n * 3 + i];
        relative(w, plus, rel);
        const float mass = (rel[0] + rel[1]) + rel[2];
        s.counted = live && st > a.td_steps && mass > 0.0f;
        const float den = fmaxf(mass, 1e-8f);
        float klt = 0.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float t = rel[i] / den;
            if (a.soft) t = a.td_keep * t + a.td_flat;
            s.ft[i] = t;
            klt += xlogx(t) - t * s.v[i];
        }
        s.tdkl = s.counted ? klt : 0.0f;
    }

    // ---- auxiliary head
    s.aux = static_cast<float>(a.aux_target[n]) / a.aux_offset;
    s.diff = a.steps[n] - s.aux;
}

// the run of lane groups a block walks, and this lane's place in a group
template <class G>
__device__ __forceinline__ void my_run(const TrainArgs &a, int64_t &g0, int64_t &g1, int &sub, int &act)
{
    const int lane = threadIdx.x;
    sub = G::LANES == WAVE ? 0 : lane / G::LANES;
    act = G::LANES == WAVE ? lane : lane % G::LANES;
    g0 = static_cast<int64_t>(blockIdx.x) * a.per_block;
    g1 = g0 + a.per_block < a.groups ? g0 + a.per_block : a.groups;
}

template <class G>
__global__ void __launch_bounds__(WAVE) k_train_loss(TrainArgs a)
{
    constexpr int PER_WAVE = WAVE / G::LANES;       // samples a wavefront holds at a time
    int64_t g0, g1;
    int sub, act;
    my_run<G>(a, g0, g1, sub, act);
    float sums[N_SUMS];
    int cnt[N_COUNTS];
#pragma unroll
    for (int i = 0; i < N_SUMS; ++i) sums[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < N_COUNTS; ++i) cnt[i] = 0;

    // all 64 lanes stay in step (the DPP sums read their neighbours): a sample past the end is the last one, unlive
    for (int64_t g = g0; g < g1; g += PER_WAVE) {
        const int64_t at = g + sub;
        const bool live = at < g1;                  // g1 <= N
        const size_t n = static_cast<size_t>(at < a.N ? at : a.N - 1);
        Sample s;
        load_sample<G>(a, n, act, live, s);
        sums[S_KL] += live ? s.kl * s.weight * s.mask : 0.0f;
        sums[S_HM] += live ? s.H * s.mask : 0.0f;
        sums[S_H] += live ? s.H : 0.0f;
        sums[S_VB] += live ? s.vb : 0.0f;
        sums[S_DIST] += live ? s.dist : 0.0f;
        sums[S_TD] += s.tdkl;
        const float ad = fabsf(s.diff);
        sums[S_AUX] += live ? (ad < 1.0f ? 0.5f * s.diff * s.diff : ad - 0.5f) : 0.0f;
        if (live) {
#pragma unroll
            for (int i = 0; i < 9; ++i) cnt[i] += (s.cls * 3 + s.pred == i) ? 1 : 0;
            cnt[C_POLICY] += s.mask > 0.0f ? 1 : 0;
            cnt[C_TD] += s.counted ? 1 : 0;
        }
    }
    // one value per group sits in each of its lanes: keep the group's first lane, add the groups in the DPP order
    const bool first = act == 0;
    uint32_t *row = a.partials + static_cast<size_t>(blockIdx.x) * ROW_WORDS;
#pragma unroll
    for (int i = 0; i < N_SUMS; ++i) {
        const float total = PER_WAVE == 1 ? sums[i] : wave_sum(first ? sums[i] : 0.0f);
        if (threadIdx.x == 0) row[i] = __float_as_uint(total);
    }
#pragma unroll
    for (int i = 0; i < N_COUNTS; ++i) {
        // a block counts at most 2^19 rows (N <= 2^30 over 2048 blocks): the float sum of its 8 groups is exact
        const int total = PER_WAVE == 1 ? cnt[i] : static_cast<int>(wave_sum(first ? static_cast<float>(cnt[i]) : 0.0f));
        if (threadIdx.x == 0) row[N_SUMS + i] = static_cast<uint32_t>(total);
    }
}

__global__ void __launch_bounds__(WAVE) k_train_reduce(TrainArgs a)
{
    const int lane = threadIdx.x;
    float sums[N_SUMS];
    int cnt[N_COUNTS];
#pragma unroll
    for (int i = 0; i < N_SUMS; ++i) sums[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < N_COUNTS; ++i) cnt[i] = 0;
    for (int r = lane; r < a.rows; r += WAVE) {
        const uint32_t *row = a.partials + static_cast<size_t>(r) * ROW_WORDS;
#pragma unroll
        for (int i = 0; i < N_SUMS; ++i) sums[i] += __uint_as_float(row[i]);
#pragma unroll
        for (int i = 0; i < N_COUNTS; ++i) cnt[i] += static_cast<int>(row[N_SUMS + i]);
    }
#pragma unroll
    for (int i = 0; i < N_SUMS; ++i) sums[i] = wave_sum(sums[i]);
    // integer totals up to 2^30 are not exact in float: add them with the integer form of the same lane movement
#pragma unroll
    for (int i = 0; i < N_COUNTS; ++i) {
        int v = cnt[i];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
        cnt[i] = v;
    }
    if (lane != 0) return;
    const float n = static_cast<float>(a.N);
    float policy = sums[S_KL] / n;
    if (a.entropy) policy = policy - a.entropy_lambda * (sums[S_HM] / n);
    float value = sums[S_VB] / n;
    if (a.distill) value = a.one_m_distill * value + a.distill_alpha * ((sums[S_DIST] / n) * a.distill_t2);
    if (a.td && cnt[C_TD] > 0) value = a.one_m_td * value + a.td_alpha * (sums[S_TD] / static_cast<float>(cnt[C_TD]));
    a.losses[0] = policy;
    a.losses[1] = value;
    a.losses[2] = sums[S_AUX] / n;
    a.losses[3] = sums[S_H] / n;
#pragma unroll
    for (int i = 0; i < N_COUNTS; ++i) a.counts[i] = cnt[i];
}

template <class G>
__global__ void __launch_bounds__(WAVE) k_train_grad(TrainArgs a)
{
    constexpr int PER_WAVE = WAVE / G::LANES, A = G::ACTIONS, AL = A < WAVE ? A : WAVE;
    constexpr bool TAIL = A > WAVE;
    int64_t g0, g1;
    int sub, act;
    my_run<G>(a, g0, g1, sub, act);
    const float up = a.upstream[0], uv = a.upstream[1], ua = a.upstream[2];
    const int td_rows = a.td ? a.counts[C_TD] : 0;
    const bool td_on = td_rows > 0;
    const float n = static_cast<float>(a.N), td_n = static_cast<float>(td_on ? td_rows : 1);

    for (int64_t g = g0; g < g1; g += PER_WAVE) {
        const int64_t at = g + sub;
        const bool live = at < g1;
        const size_t row = static_cast<size_t>(at < a.N ? at : a.N - 1);
        Sample s;
        load_sample<G>(a, row, act, live, s);
        if (!live) continue;                        // only in a block's last round, after the group sums
        // ---- policy: d/d log_p_a of  mask w kl - lambda mask H,  dH / d log_p_a = -p_a (log_p_a + 1)
        const float kw = s.mask * s.weight;
#pragma unroll
        for (int j = 0; j < (TAIL ? 2 : 1); ++j) {
            if (j == 0 ? act >= AL : act != 0) continue;
            float d = -(kw * s.p[j]);
            if (a.entropy) d = d + (a.entropy_lambda * s.mask) * (s.pe[j] * (s.lp[j] + 1.0f));
            a.d_log_p[row * A + (j == 0 ? act : A - 1)] = up * (d / n);
        }
        // ---- value
        if (act < 3) {
            const float z = act == 0 ? s.z[0] : act == 1 ? s.z[1] : s.z[2];
            float d = -z;
            if (a.distill) {
                const float t = act == 0 ? s.t[0] : act == 1 ? s.t[1] : s.t[2];
                const float sm = act == 0 ? s.sm[0] : act == 1 ? s.sm[1] : s.sm[2];
                d = a.one_m_distill * d + a.distill_alpha * ((a.distill_t2 * s.has_q) * ((sm * s.tsum - t) / a.distill_temp));
            }
            d = d / n;
            if (td_on) {
                const float ft = act == 0 ? s.ft[0] : act == 1 ? s.ft[1] : s.ft[2];
                d = a.one_m_td * d + a.td_alpha * (s.counted ? -ft / td_n : 0.0f);
            }
            a.d_value[row * 3 + act] = uv * d;
        }
        // ---- aux: smooth-L1, beta 1
        if (act == 0) {
            const float d = s.diff < -1.0f ? -1.0f : s.diff > 1.0f ? 1.0f : s.diff;
            a.d_steps[row] = ua * (d / n);
        }
    }
}

// blocks of the loss and gradient kernels: every block walks per_block groups, a multiple of what a wavefront holds
void shape(int game, int64_t N, TrainArgs &a)
{
    const int per_wave = game == Connect4Dev::GAME_ID ? WAVE / Connect4Dev::LANES : WAVE / OthelloDev::LANES;
    a.groups = N;                                                         // a lane group is a sample
    const int64_t waves = (a.groups + per_wave - 1) / per_wave;           // wavefront-loads of samples
    const int64_t per_row = (waves + MAX_ROWS - 1) / MAX_ROWS;            // loads one block walks
    a.per_block = per_row * per_wave;
    a.rows = static_cast<int>((waves + per_row - 1) / per_row);
}

}  // namespace
}  // namespace az

using namespace az::host;

namespace {

// every check of az_train.h, before anything is enqueued
az::TrainArgs train_args(const std::string &w, int game, const az_replay_batch *b, const az_train_heads *h, int64_t N,
                         const az_train_loss_config *c, const az_train_loss_out *o, bool need_workspace)
{
    require(known_game(game), w + ": unknown game");
    require(N > 0 && N <= (int64_t(1) << 30), w + ": N must be positive (and at most 2^30)");
    require(b != nullptr && h != nullptr && c != nullptr && o != nullptr, w + ": null argument");
    const void *q16[] = {b->state, b->prob, b->winner, b->steps_to_end, b->aux_target, b->root_wdl, b->future_root_wdl,
                         h->log_p, h->value};
    for (const void *q : q16)
        require(aligned(q, 16), w + ": a null tensor or one that is not 16-byte aligned");
    require(aligned(h->steps, 4) && aligned(o->losses, 4) && aligned(o->counts, 4), w + ": steps, losses or counts null or misaligned");
    if (need_workspace) require(aligned(o->workspace, 16), w + ": a null workspace or one that is not 16-byte aligned");
    require(c->value_decay > 0.0 && c->value_decay <= 1.0, w + ": value_decay must lie in (0, 1]");
    require(c->distill_alpha >= 0.0 && c->distill_alpha <= 1.0, w + ": distill_alpha must lie in [0, 1]");
    require(c->td_alpha >= 0.0 && c->td_alpha <= 1.0, w + ": td_alpha must lie in [0, 1]");
    require(c->distill_temp > 0.0, w + ": distill_temp must be positive");
    require(c->psw_beta >= 0.0 && c->entropy_lambda >= 0.0 && c->td_steps >= 0, w + ": psw_beta, entropy_lambda and td_steps must not be negative");
    require(c->aux_target_offset > 0.0, w + ": aux_target_offset must be positive");

    az::TrainArgs a{};
    a.state = b->state; a.prob = b->prob; a.root_wdl = b->root_wdl; a.future_root_wdl = b->future_root_wdl;
    a.winner = b->winner; a.steps_to_end = b->steps_to_end; a.aux_target = b->aux_target;
    a.log_p = h->log_p; a.value = h->value; a.steps = h->steps;
    a.N = N;
    az::shape(game, N, a);
    a.value_decay = static_cast<float>(c->value_decay);
    a.third = static_cast<float>(1.0 / 3.0);
    a.distill_alpha = static_cast<float>(c->distill_alpha);
    a.one_m_distill = static_cast<float>(1.0 - c->distill_alpha);
    a.distill_temp = static_cast<float>(c->distill_temp);
    a.distill_t2 = static_cast<float>(c->distill_temp * c->distill_temp);
    a.psw_beta = static_cast<float>(c->psw_beta);
    a.entropy_lambda = static_cast<float>(c->entropy_lambda);
    a.td_alpha = static_cast<float>(c->td_alpha);
    a.one_m_td = static_cast<float>(1.0 - c->td_alpha);
    const double keep = std::pow(c->value_decay, static_cast<double>(c->td_steps));
    a.td_keep = static_cast<float>(keep);
    a.td_flat = static_cast<float>((1.0 - keep) / 3.0);
    a.td_steps = c->td_steps;
    a.aux_offset = static_cast<float>(c->aux_target_offset);
    a.soft = c->value_decay < 1.0;
    a.distill = c->distill_alpha > 0.0;
    a.psw = c->psw_beta > 0.0;
    a.entropy = c->entropy_lambda > 0.0;
    a.td = c->td_alpha > 0.0;
    a.partials = static_cast<uint32_t *>(o->workspace);
    a.losses = o->losses;
    a.counts = o->counts;
    return a;
}

}  // namespace

extern "C" {

int64_t az_train_loss_workspace_bytes(int game, int64_t N)
{
    if (!known_game(game) || N <= 0 || N > (int64_t(1) << 30)) return -1;
    az::TrainArgs a{};
    az::shape(game, N, a);
    return static_cast<int64_t>(a.rows) * az::ROW_WORDS * static_cast<int64_t>(sizeof(uint32_t));
}

int az_train_dev_loss(int game, const az_replay_batch *batch, const az_train_heads *heads, int64_t N,
                      const az_train_loss_config *config, const az_train_loss_out *out, void *stream)
{
    return guarded([&] {
        const az::TrainArgs a = train_args("az_train_dev_loss", game, batch, heads, N, config, out, true);
        const hipStream_t s = static_cast<hipStream_t>(stream);
        if (game == az::Connect4Dev::GAME_ID) hipLaunchKernelGGL(az::k_train_loss<az::Connect4Dev>, dim3(a.rows), dim3(az::WAVE), 0, s, a);
        else hipLaunchKernelGGL(az::k_train_loss<az::OthelloDev>, dim3(a.rows), dim3(az::WAVE), 0, s, a);
        hipLaunchKernelGGL(az::k_train_reduce, dim3(1), dim3(az::WAVE), 0, s, a);
        HIP_OK(hipGetLastError());
    });
}

int az_train_dev_loss_grad(int game, const az_replay_batch *batch, const az_train_heads *heads, int64_t N,
                           const az_train_loss_config *config, const az_train_loss_out *out, const float *upstream,
                           const az_train_grads *grads, void *stream)
{
    return guarded([&] {
        const std::string w("az_train_dev_loss_grad");
        az::TrainArgs a = train_args(w, game, batch, heads, N, config, out, false);
        require(aligned(upstream, 4), w + ": a null or misaligned upstream");
        require(grads != nullptr, w + ": null argument");
        require(aligned(grads->d_log_p, 16) && aligned(grads->d_value, 16), w + ": a null gradient or one that is not 16-byte aligned");
        require(aligned(grads->d_steps, 4), w + ": a null or misaligned d_steps");
        a.upstream = upstream;
        a.d_log_p = grads->d_log_p; a.d_value = grads->d_value; a.d_steps = grads->d_steps;
        const hipStream_t s = static_cast<hipStream_t>(stream);
        if (game == az::Connect4Dev::GAME_ID) hipLaunchKernelGGL(az::k_train_grad<az::Connect4Dev>, dim3(a.rows), dim3(az::WAVE), 0, s, a);
        else hipLaunchKernelGGL(az::k_train_grad<az::OthelloDev>, dim3(a.rows), dim3(az::WAVE), 0, s, a);
        HIP_OK(hipGetLastError());
    });
}

}  // extern "C"
