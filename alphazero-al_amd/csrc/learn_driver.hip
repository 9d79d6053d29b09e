// learn_driver.hip - the native learner (az_learn_* in az_train.h): a Connect4 training batch, or an epoch of them, driven
// from C.  The host side calls the entry points of the five training units (train_stem_kernels.hip, train_block_kernels.hip,
// train_attn_kernels.hip, train_heads_kernels.hip, train_kernels.hip) and az_opt_dev_step (optim_kernels.hip) in the order
// the Python route's autograd graph runs them, on buffers allocated once at az_learn_create; none of their kernels is
// touched.  Two small kernels of its own:
//
//   k_learn_keep   every dropout input of a batch in one launch, under the contract az_train.h states.  The launch is a
//                  flat range of 16-byte stores: the blocks' factors, the attention block's words, the policy head's
//                  factors, the pool factors, one after the other; a tensor at rate 0 has no stores.  A lane of a factor
//                  tensor forms its group's stream state and four consecutive draws and stores one float4; a lane of the
//                  attention block assembles two whole words (2 x 42 draws) in registers and stores them as one 16-byte
//                  pair - no read-modify-write, no atomics, no LDS, no scratch.  The generator is counter-based
//                  (dev_rng.h), so any lane computes any draw.
//   k_learn_tail   one wavefront: the running sums take the batch's three losses, the batch count goes up, the entropy
//                  is copied out of the loss pass's way.  Plain vector loads and stores.
#include "engine_internal.h"

#include "az_train.h"
#include "dev_rng.h"

namespace az {
namespace {

constexpr int KEEP_BLOCK = 256;
constexpr int CH = 64;                                  // channels: the size of a factor group
constexpr int CELLS = 42, HEADS = 4, COLS = 7;
constexpr int IMAGE = CH * CELLS;                       // floats of a sample between the stem and the heads
constexpr int STORES_PER_GROUP = CH / 4;                // float4 stores of a group of 64 factors
constexpr int ATTN_WORDS = HEADS * CELLS;               // words of a sample
static_assert(ATTN_WORDS % 2 == 0, "a sample's words are whole 16-byte pairs");

struct KeepArgs {
    float *blocks;                  // block k at blocks + k * block_stride
    uint64_t *attn;
    float *policy, *pool;
    int64_t block_stride;           // floats
    uint32_t per_block;             // stores of one block's tensor: N * 16
    uint32_t end_blocks, end_attn, end_policy, end_pool;    // where each tensor's stores end in the launch's flat range
    uint32_t thr_block, thr_attn, thr_policy, thr_pool;
    float f_block, f_policy, f_pool;
    uint64_t seed, call;
};

// draw number j of a stream: what the (j + 1)-th DevRng::next() returns
__device__ __forceinline__ uint32_t draw_at(const DevRng &r, uint32_t j)
{
    return static_cast<uint32_t>(mix64(r.s + (static_cast<uint64_t>(j) + 1) * 0x9E3779B97F4A7C15ull) >> 32);
}

__device__ __forceinline__ uint64_t keep_word(const KeepArgs &a, uint64_t word)
{
    const DevRng r(a.seed, a.call, word, LEARN_STREAM + AZ_LEARN_KEEP_ATTN);
    uint64_t bits = 0;
#pragma unroll
    for (uint32_t j = 0; j < CELLS; ++j)
        bits |= static_cast<uint64_t>(draw_at(r, j) >= a.thr_attn) << j;
    return bits;
}

__global__ void __launch_bounds__(KEEP_BLOCK) k_learn_keep(const KeepArgs a)
{
    const uint32_t i = blockIdx.x * KEEP_BLOCK + threadIdx.x;
    if (i >= a.end_pool) return;
    if (i >= a.end_blocks && i < a.end_attn) {
        const uint64_t pair = i - a.end_blocks;
        ulonglong2 w;
        w.x = keep_word(a, 2 * pair);
        w.y = keep_word(a, 2 * pair + 1);
        *reinterpret_cast<ulonglong2 *>(a.attn + 2 * pair) = w;
        return;
    }
    uint32_t r, thr;
    uint64_t t;
    float *base, f;
    if (i < a.end_blocks) {
        const uint32_t k = i / a.per_block;
        r = i - k * a.per_block; t = k; base = a.blocks + k * a.block_stride; thr = a.thr_block; f = a.f_block;
    } else if (i < a.end_policy) {
        r = i - a.end_attn; t = AZ_LEARN_KEEP_POLICY; base = a.policy; thr = a.thr_policy; f = a.f_policy;
    } else {
        r = i - a.end_policy; t = AZ_LEARN_KEEP_POOL; base = a.pool; thr = a.thr_pool; f = a.f_pool;
    }
    const DevRng g(a.seed, a.call, r / STORES_PER_GROUP, LEARN_STREAM + t);
    const uint32_t j = (r % STORES_PER_GROUP) * 4;
    float4 v;
    v.x = draw_at(g, j) >= thr ? f : 0.0f;
    v.y = draw_at(g, j + 1) >= thr ? f : 0.0f;
    v.z = draw_at(g, j + 2) >= thr ? f : 0.0f;
    v.w = draw_at(g, j + 3) >= thr ? f : 0.0f;
    *reinterpret_cast<float4 *>(base + static_cast<int64_t>(r) * 4) = v;
}

// tally: [0..2] the running sums, [3] the last training batch's entropy, [4] the batch count (int32)
constexpr int TALLY_ENTROPY = 3, TALLY_BATCHES = 4;

__global__ void __launch_bounds__(64) k_learn_tail(const float *__restrict__ losses, float *__restrict__ tally)
{
    const int lane = threadIdx.x;
    if (lane < 3) tally[lane] += losses[lane];
    else if (lane == TALLY_ENTROPY) tally[lane] = losses[lane];
    else if (lane == TALLY_BATCHES) reinterpret_cast<int32_t *>(tally)[lane] += 1;
}

}  // namespace
}  // namespace az

namespace {

constexpr int64_t MAX_LEARN_ROWS = int64_t(1) << 20;
constexpr int GAME = AZ_GAME_CONNECT4;
// where the small outputs sit in one buffer of floats
constexpr int AT_LOSSES = 0, AT_COUNTS = 16, AT_UPSTREAM = 32, AT_TALLY = 40, AT_NORM = 48, SMALL_FLOATS = 64;

// numel and the alignment (bytes) param and grad of a role need
struct RoleShape { int64_t numel; int align; };

RoleShape role_shape(int role)
{
    static const RoleShape stem[4] = {{2 * 32, 4}, {24 * 32, 4}, {64 * 32 * 9, 4}, {64, 4}};
    static const RoleShape block[4] = {{64, 4}, {64, 4}, {64 * 64 * 9, 16}, {64, 4}};
    static const RoleShape attn[6] = {{64, 4}, {192 * 64, 16}, {4 * 64, 4}, {64 * 64, 16}, {16, 4}, {16, 4}};
    static const RoleShape heads[18] = {{64, 4}, {64, 4}, {1, 4}, {4096, 16}, {64, 4}, {64, 4}, {1, 4}, {64, 4}, {4096, 16},
                                        {64, 4}, {64, 4}, {4096, 16}, {64, 4}, {64, 4}, {192, 4}, {3, 4}, {64, 4}, {1, 4}};
    if (role < AZ_LEARN_ROLE_BLOCK) return stem[role];
    if (role < AZ_LEARN_ROLE_ATTN) return block[(role - AZ_LEARN_ROLE_BLOCK) % 4];
    if (role < AZ_LEARN_ROLE_HEADS) return attn[role - AZ_LEARN_ROLE_ATTN];
    return heads[role - AZ_LEARN_ROLE_HEADS];
}

uint32_t threshold(double p)
{
    const double v = std::floor(p * 4294967296.0 + 0.5);
    return v >= 4294967295.0 ? 0xFFFFFFFFu : static_cast<uint32_t>(v);
}

float factor(double p) { return 1.0f / (1.0f - static_cast<float>(p)); }

}  // namespace

struct az_learn {
    az_learn_config c{};
    bool bound = false;
    int64_t n_tensors = 0;
    int32_t n_groups = 0;
    az_opt *opt = nullptr;
    void *param[AZ_LEARN_ROLES] = {};
    void *grad[AZ_LEARN_ROLES] = {};
    std::vector<const void *> grad_flat;        // in the optimiser's order
    std::vector<int64_t> step_no;               // an epoch's step numbers, batch by batch
    int64_t workspace_bytes = 0;
    // activations: x[0] the stem's output, x[k + 1] block k's y; z, stats per block; the tokens; the head outputs
    DevBuf<float> x[AZ_LEARN_MAX_BLOCKS + 1], z[AZ_LEARN_MAX_BLOCKS], stats[AZ_LEARN_MAX_BLOCKS], tokens, log_p, value, steps;
    DevBuf<float> d_log_p, d_value, d_steps, d_a, d_b;
    DevBuf<float> keep_blocks, keep_policy, keep_pool;
    DevBuf<uint64_t> keep_attn;
    DevBuf<uint8_t> workspace, table;
    DevBuf<float> small;
    // batch tensors of its own, for az_learn_dev_epoch
    DevBuf<float> b_state, b_prob, b_root, b_future;
    DevBuf<int8_t> b_winner;
    DevBuf<int16_t> b_to_end, b_aux;
    DevBuf<uint8_t> b_mask;
    ~az_learn() { az_opt_destroy(opt); }

    float *losses() { return small.p + AT_LOSSES; }
    int32_t *counts() { return reinterpret_cast<int32_t *>(small.p + AT_COUNTS); }
    float *upstream() { return small.p + AT_UPSTREAM; }
    float *tally() { return small.p + AT_TALLY; }
    float *norm() { return small.p + AT_NORM; }
    bool any_rate() const { return c.p_block > 0.0 || c.p_attn > 0.0 || c.p_policy > 0.0 || c.p_pool > 0.0; }
    az_replay_batch own_batch()
    {
        return az_replay_batch{b_state.p, b_prob.p, b_winner.p, b_to_end.p, b_aux.p, b_root.p, b_mask.p, b_future.p};
    }
};

namespace {

// ---- every check of a step, before anything is enqueued

void check_batch(const std::string &w, const az_learn *l, const az_replay_batch *b, int64_t N, const az_train_loss_config *c)
{
    require(l != nullptr && b != nullptr && c != nullptr, w + ": null argument");
    require(l->bound, w + ": called before az_learn_bind");
    require(N > 0 && N <= l->c.max_rows, w + ": N must lie in [1, max_rows]");
    const void *q16[] = {b->state, b->prob, b->winner, b->steps_to_end, b->aux_target, b->root_wdl, b->future_root_wdl};
    for (const void *q : q16)
        require(aligned(q, 16), w + ": a null batch tensor or one that is not 16-byte aligned");
    require(b->valid_mask != nullptr, w + ": a null valid_mask");
    require(c->value_decay > 0.0 && c->value_decay <= 1.0, w + ": value_decay must lie in (0, 1]");
    require(c->distill_alpha >= 0.0 && c->distill_alpha <= 1.0, w + ": distill_alpha must lie in [0, 1]");
    require(c->td_alpha >= 0.0 && c->td_alpha <= 1.0, w + ": td_alpha must lie in [0, 1]");
    require(c->distill_temp > 0.0, w + ": distill_temp must be positive");
    require(c->psw_beta >= 0.0 && c->entropy_lambda >= 0.0 && c->td_steps >= 0, w + ": psw_beta, entropy_lambda and td_steps must not be negative");
    require(c->aux_target_offset > 0.0, w + ": aux_target_offset must be positive");
    const int mw = l->c.max_workgroups;
    const int64_t need = std::max({az_train_loss_workspace_bytes(GAME, N), az_train_block_workspace_bytes(N, mw),
                                   az_train_attn_workspace_bytes(N, mw), az_train_stem_workspace_bytes(N, mw),
                                   az_train_heads_workspace_bytes(N, mw)});
    require(need > 0 && need <= l->workspace_bytes, w + ": the workspace does not serve this N");
}

void check_optimiser(const std::string &w, const az_learn *l, const int64_t *step, const double *group_hp, int32_t n_groups)
{
    require(step != nullptr && group_hp != nullptr, w + ": null argument");
    for (int64_t i = 0; i < l->n_tensors; ++i)
        require(step[i] >= 1 && step[i] < (int64_t(1) << 62), w + ": every tensor takes a step: step[i] >= 1");
    for (int g = 0; g < n_groups; ++g) {
        const double *h = group_hp + g * AZ_OPT_GROUP_HP;
        require(h[0] >= 0.0 && std::isfinite(h[0]), w + ": lr must not be negative");
        require(h[1] >= 0.0 && h[1] < 1.0 && h[2] >= 0.0 && h[2] < 1.0, w + ": a beta outside [0, 1)");
        require(h[3] >= 0.0 && std::isfinite(h[3]), w + ": eps must not be negative");
        require(h[4] >= 0.0 && std::isfinite(h[4]), w + ": weight_decay must not be negative");
    }
}

// ---- the launches

az_train_stem_params stem_params(az_learn *l)
{
    auto p = [&](int r) { return static_cast<const float *>(l->param[r]); };
    return az_train_stem_params{p(AZ_LEARN_ROLE_PIECE_EMB), p(AZ_LEARN_ROLE_POS_EMB), p(AZ_LEARN_ROLE_STEM_CONV_WEIGHT),
                                p(AZ_LEARN_ROLE_STEM_CONV_BIAS)};
}

az_train_block_params block_params(az_learn *l, int k)
{
    auto p = [&](int f) { return static_cast<const float *>(l->param[AZ_LEARN_ROLE_BLOCK + 4 * k + f]); };
    return az_train_block_params{p(0), p(1), p(2), p(3)};
}

az_train_attn_params attn_params(az_learn *l)
{
    auto p = [&](int f) { return static_cast<const float *>(l->param[AZ_LEARN_ROLE_ATTN + f]); };
    return az_train_attn_params{p(0), p(1), p(2), p(3), p(4), p(5)};
}

az_train_heads_params heads_params(az_learn *l)
{
    az_train_heads_params hp;
    const float **f = reinterpret_cast<const float **>(&hp);        // eighteen pointers, in the roles' order
    for (int i = 0; i < 18; ++i) f[i] = static_cast<const float *>(l->param[AZ_LEARN_ROLE_HEADS + i]);
    return hp;
}
static_assert(sizeof(az_train_heads_params) == 18 * sizeof(float *), "az_train_heads_params is eighteen pointers");
static_assert(sizeof(az_train_heads_grads) == 21 * sizeof(float *), "az_train_heads_grads: d_tokens, eighteen pointers, the workspace and its size");

struct Keeps {
    const float *blocks[AZ_LEARN_MAX_BLOCKS];
    const uint64_t *attn;
    float scale;
    const float *policy, *pool;
};

void launch_keep(az_learn *l, int64_t N, uint64_t call, hipStream_t s)
{
    const az_learn_config &c = l->c;
    az::KeepArgs a{};
    a.blocks = l->keep_blocks.p; a.attn = l->keep_attn.p; a.policy = l->keep_policy.p; a.pool = l->keep_pool.p;
    a.block_stride = az::CH * c.max_rows;
    const uint32_t n = static_cast<uint32_t>(N);
    a.per_block = n * az::STORES_PER_GROUP;
    a.end_blocks = c.p_block > 0.0 ? a.per_block * static_cast<uint32_t>(c.n_blocks) : 0u;
    a.end_attn = a.end_blocks + (c.p_attn > 0.0 ? n * (az::ATTN_WORDS / 2) : 0u);
    a.end_policy = a.end_attn + (c.p_policy > 0.0 ? n * az::COLS * az::STORES_PER_GROUP : 0u);
    a.end_pool = a.end_policy + (c.p_pool > 0.0 ? n * az::STORES_PER_GROUP : 0u);
    a.thr_block = threshold(c.p_block); a.thr_attn = threshold(c.p_attn);
    a.thr_policy = threshold(c.p_policy); a.thr_pool = threshold(c.p_pool);
    a.f_block = factor(c.p_block); a.f_policy = factor(c.p_policy); a.f_pool = factor(c.p_pool);
    a.seed = c.seed; a.call = call;
    hipLaunchKernelGGL(az::k_learn_keep, dim3((a.end_pool + az::KEEP_BLOCK - 1) / az::KEEP_BLOCK), dim3(az::KEEP_BLOCK), 0, s, a);
}

// stem, blocks, attention, heads; `train`: with the keeps, z and stats saved
void forward(az_learn *l, const az_replay_batch *b, int64_t N, const Keeps &keep, bool train, void *stream)
{
    const az_learn_config &c = l->c;
    const az_train_stem_params sp = stem_params(l);
    check_rc(az_train_dev_stem_fwd(&sp, b->state, N, l->x[0].p, l->table.p, AZ_TRAIN_STEM_TABLE_BYTES, stream));
    for (int k = 0; k < c.n_blocks; ++k) {
        const az_train_block_params bp = block_params(l, k);
        const az_train_block_saved saved{l->z[k].p, l->stats[k].p};
        check_rc(az_train_dev_block_fwd(&bp, l->x[k].p, keep.blocks[k], N, c.eps_block, l->x[k + 1].p, train ? &saved : nullptr, stream));
    }
    const az_train_attn_params ap = attn_params(l);
    check_rc(az_train_dev_attn_fwd(&ap, l->x[c.n_blocks].p, 0, keep.attn, keep.scale, N, c.eps_attn, l->tokens.p, stream));
    const az_train_heads_params hp = heads_params(l);
    check_rc(az_train_dev_heads_fwd(&hp, l->tokens.p, b->valid_mask, keep.policy, keep.pool, N, c.eps_heads, l->log_p.p,
                                    l->value.p, l->steps.p, stream));
}

void loss(az_learn *l, const az_replay_batch *b, int64_t N, const az_train_loss_config *cfg, void *stream)
{
    const az_train_heads h{l->log_p.p, l->value.p, l->steps.p};
    const az_train_loss_out o{l->losses(), l->counts(), l->workspace.p};
    check_rc(az_train_dev_loss(GAME, b, &h, N, cfg, &o, stream));
}

// one training batch; everything was checked
void train_batch(az_learn *l, const az_replay_batch *b, int64_t N, const az_train_loss_config *cfg, const int64_t *step,
                 const double *group_hp, uint64_t call, void *stream)
{
    const az_learn_config &c = l->c;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int mw = c.max_workgroups;
    Keeps keep{};
    keep.scale = 1.0f;
    if (l->any_rate()) {
        launch_keep(l, N, call, s);
        for (int k = 0; k < c.n_blocks; ++k)
            keep.blocks[k] = c.p_block > 0.0 ? l->keep_blocks.p + k * az::CH * c.max_rows : nullptr;
        if (c.p_attn > 0.0) { keep.attn = l->keep_attn.p; keep.scale = factor(c.p_attn); }
        keep.policy = c.p_policy > 0.0 ? l->keep_policy.p : nullptr;
        keep.pool = c.p_pool > 0.0 ? l->keep_pool.p : nullptr;
    }
    forward(l, b, N, keep, true, stream);
    loss(l, b, N, cfg, stream);
    const az_train_heads h{l->log_p.p, l->value.p, l->steps.p};
    const az_train_loss_out o{l->losses(), l->counts(), nullptr};
    const az_train_grads lg{l->d_log_p.p, l->d_value.p, l->d_steps.p};
    check_rc(az_train_dev_loss_grad(GAME, b, &h, N, cfg, &o, l->upstream(), &lg, stream));

    auto g = [&](int r) { return static_cast<float *>(l->grad[r]); };
    const az_train_heads_params hp = heads_params(l);
    az_train_heads_grads hg;
    float **hf = reinterpret_cast<float **>(&hg);
    hf[0] = l->d_a.p;
    for (int i = 0; i < 18; ++i) hf[1 + i] = g(AZ_LEARN_ROLE_HEADS + i);
    hg.workspace = l->workspace.p; hg.workspace_bytes = l->workspace_bytes;
    check_rc(az_train_dev_heads_bwd(&hp, l->tokens.p, b->valid_mask, keep.policy, keep.pool, l->d_log_p.p, l->d_value.p,
                                    l->d_steps.p, N, c.eps_heads, mw, &hg, stream));
    float *dy = l->d_a.p, *dx = l->d_b.p;
    const az_train_attn_params ap = attn_params(l);
    const az_train_attn_grads ag{dx, g(AZ_LEARN_ROLE_ATTN), g(AZ_LEARN_ROLE_ATTN + 1), g(AZ_LEARN_ROLE_ATTN + 2), g(AZ_LEARN_ROLE_ATTN + 3),
                                 g(AZ_LEARN_ROLE_ATTN + 4), g(AZ_LEARN_ROLE_ATTN + 5), l->workspace.p, l->workspace_bytes};
    check_rc(az_train_dev_attn_bwd(&ap, l->x[c.n_blocks].p, 0, keep.attn, keep.scale, dy, N, c.eps_attn, mw, &ag, stream));
    std::swap(dy, dx);
    for (int k = c.n_blocks - 1; k >= 0; --k) {
        const az_train_block_params bp = block_params(l, k);
        const az_train_block_saved saved{l->z[k].p, l->stats[k].p};
        const int r = AZ_LEARN_ROLE_BLOCK + 4 * k;
        const az_train_block_grads bg{dx, g(r), g(r + 1), g(r + 2), g(r + 3), l->workspace.p, l->workspace_bytes};
        check_rc(az_train_dev_block_bwd(&bp, l->x[k].p, keep.blocks[k], dy, &saved, N, mw, &bg, stream));
        std::swap(dy, dx);
    }
    const az_train_stem_params sp = stem_params(l);
    const az_train_stem_grads sg{g(AZ_LEARN_ROLE_PIECE_EMB), g(AZ_LEARN_ROLE_POS_EMB), g(AZ_LEARN_ROLE_STEM_CONV_WEIGHT),
                                 g(AZ_LEARN_ROLE_STEM_CONV_BIAS), l->workspace.p, l->workspace_bytes};
    check_rc(az_train_dev_stem_bwd(&sp, b->state, reinterpret_cast<const float *>(l->table.p), dy, N, mw, &sg, stream));

    check_rc(az_opt_dev_step(l->opt, l->grad_flat.data(), step, group_hp, c.max_norm, l->norm(), stream));
    hipLaunchKernelGGL(az::k_learn_tail, dim3(1), dim3(64), 0, s, l->losses(), l->tally());
    HIP_OK(hipGetLastError());
}

}  // namespace

extern "C" {

int az_learn_create(const az_learn_config *config, az_learn **out)
{
    return guarded([&] {
        const std::string w("az_learn_create");
        require(out != nullptr, w + ": null argument");
        *out = nullptr;
        require(config != nullptr, w + ": null argument");
        const az_learn_config &c = *config;
        require(c.max_rows >= 1 && c.max_rows <= MAX_LEARN_ROWS, w + ": max_rows must lie in [1, 2^20]");
        require(c.n_blocks >= 1 && c.n_blocks <= AZ_LEARN_MAX_BLOCKS, w + ": n_blocks must lie in [1, 8]");
        require(c.max_workgroups >= 0, w + ": max_workgroups must not be negative");
        for (float eps : {c.eps_block, c.eps_attn, c.eps_heads})
            require(eps > 0.0f && std::isfinite(eps), w + ": an eps that is not positive and finite");
        for (double p : {c.p_block, c.p_attn, c.p_policy, c.p_pool})
            require(p >= 0.0 && p < 1.0 && static_cast<float>(p) < 1.0f, w + ": a dropout rate outside [0, 1)");
        require(!std::isnan(c.max_norm), w + ": max_norm is not a number");

        auto l = std::make_unique<az_learn>();
        l->c = c;
        const size_t R = static_cast<size_t>(c.max_rows);
        // the largest workspace any batch of 1 .. max_rows rows asks of the five units (their sizes are not monotone in N)
        for (int64_t n = 1; n <= c.max_rows; ++n)
            l->workspace_bytes = std::max({l->workspace_bytes, az_train_loss_workspace_bytes(GAME, n),
                                           az_train_block_workspace_bytes(n, c.max_workgroups), az_train_attn_workspace_bytes(n, c.max_workgroups),
                                           az_train_stem_workspace_bytes(n, c.max_workgroups), az_train_heads_workspace_bytes(n, c.max_workgroups)});
        for (int k = 0; k <= c.n_blocks; ++k) l->x[k].ensure(R * az::IMAGE);
        for (int k = 0; k < c.n_blocks; ++k) { l->z[k].ensure(R * az::IMAGE); l->stats[k].ensure(R * 2); }
        l->tokens.ensure(R * az::IMAGE);
        l->log_p.ensure(R * az::COLS); l->value.ensure(R * 3); l->steps.ensure(R);
        l->d_log_p.ensure(R * az::COLS); l->d_value.ensure(R * 3); l->d_steps.ensure(R);
        l->d_a.ensure(R * az::IMAGE); l->d_b.ensure(R * az::IMAGE);
        l->keep_blocks.ensure(R * az::CH * c.n_blocks);
        l->keep_attn.ensure(R * az::ATTN_WORDS);
        l->keep_policy.ensure(R * az::COLS * az::CH);
        l->keep_pool.ensure(R * az::CH);
        l->workspace.ensure(static_cast<size_t>(l->workspace_bytes));
        l->table.ensure(AZ_TRAIN_STEM_TABLE_BYTES);
        l->small.ensure(SMALL_FLOATS, true);
        const float ones[3] = {1.0f, 1.0f, 1.0f};
        HIP_OK(hipMemcpy(l->upstream(), ones, sizeof(ones), hipMemcpyHostToDevice));
        l->b_state.ensure(R * 3 * az::CELLS); l->b_prob.ensure(R * az::COLS); l->b_winner.ensure(R); l->b_to_end.ensure(R);
        l->b_aux.ensure(R); l->b_root.ensure(R * 3); l->b_mask.ensure(R * az::COLS); l->b_future.ensure(R * 3);
        *out = l.release();
    });
}

void az_learn_destroy(az_learn *l) { delete l; }

int az_learn_bind(az_learn *l, int64_t n_tensors, const int32_t *role, const int32_t *group, int32_t n_groups,
                  void *const *param, void *const *grad, void *const *exp_avg, void *const *exp_avg_sq)
{
    return guarded([&] {
        const std::string w("az_learn_bind");
        require(l != nullptr && role != nullptr && group != nullptr && param != nullptr && grad != nullptr && exp_avg != nullptr &&
                exp_avg_sq != nullptr, w + ": null argument");
        const int64_t want = 28 + 4 * l->c.n_blocks;
        require(n_tensors == want, w + ": the network has 28 + 4 n_blocks tensors");
        void *p_of[AZ_LEARN_ROLES] = {}, *g_of[AZ_LEARN_ROLES] = {};
        bool seen[AZ_LEARN_ROLES] = {};
        std::vector<int64_t> numel(static_cast<size_t>(n_tensors));
        for (int64_t i = 0; i < n_tensors; ++i) {
            const int r = role[i];
            const bool known = r >= 0 && r < AZ_LEARN_ROLES &&
                               (r < AZ_LEARN_ROLE_BLOCK || r >= AZ_LEARN_ROLE_ATTN || r < AZ_LEARN_ROLE_BLOCK + 4 * l->c.n_blocks);
            require(known, w + ": a role outside this network's");
            require(!seen[r], w + ": a role given twice");
            seen[r] = true;                 // n_tensors roles, all different, all of this network's: none is missing
            const RoleShape shape = role_shape(r);
            require(aligned(param[i], shape.align) && aligned(grad[i], shape.align),
                    w + ": a null parameter or gradient, or one that is not aligned as its unit asks");
            require(aligned(exp_avg[i], 4) && aligned(exp_avg_sq[i], 4), w + ": a null or misaligned moment");
            p_of[r] = param[i]; g_of[r] = grad[i];
            numel[i] = shape.numel;
        }
        az_opt *opt = nullptr;
        check_rc(az_opt_create(n_tensors, numel.data(), group, n_groups, &opt));
        const int rc = az_opt_bind(opt, param, exp_avg, exp_avg_sq);
        if (rc != AZ_OK) { az_opt_destroy(opt); check_rc(rc); }
        az_opt_destroy(l->opt);
        l->opt = opt;
        l->n_tensors = n_tensors;
        std::memcpy(l->param, p_of, sizeof(p_of));
        std::memcpy(l->grad, g_of, sizeof(g_of));
        l->grad_flat.assign(grad, grad + n_tensors);
        l->step_no.assign(static_cast<size_t>(n_tensors), 0);
        l->n_groups = n_groups;
        l->bound = true;
    });
}

int az_learn_dev_step(az_learn *l, const az_replay_batch *batch, int64_t N, const az_train_loss_config *config,
                      const int64_t *step, const double *group_hp, uint64_t call, void *stream)
{
    return guarded([&] {
        const std::string w("az_learn_dev_step");
        check_batch(w, l, batch, N, config);
        check_optimiser(w, l, step, group_hp, l->n_groups);
        train_batch(l, batch, N, config, step, group_hp, call, stream);
    });
}

int az_learn_dev_epoch(az_learn *l, const az_replay_tensors *ring, const int64_t *idx, const int64_t *order, int64_t n,
                       int64_t B, int drop_last, const az_train_loss_config *config, const int64_t *step,
                       const double *group_hp, uint64_t first_call, int64_t *n_batches, void *stream)
{
    return guarded([&] {
        const std::string w("az_learn_dev_epoch");
        require(n_batches != nullptr, w + ": null argument");
        *n_batches = 0;
        require(l != nullptr && ring != nullptr && idx != nullptr, w + ": null argument");
        require(n > 0 && B > 0 && n <= (int64_t(1) << 40), w + ": n and B must be positive");
        require(2 * B <= l->c.max_rows, w + ": a batch of 2 B rows is more than max_rows");
        const int64_t count = drop_last ? n / B : (n + B - 1) / B;
        require(count > 0, w + ": the sample gives no batch");
        const az_replay_batch own = l->own_batch();
        check_batch(w, l, &own, 2 * std::min(B, n), config);
        if (!drop_last && n % B != 0) check_batch(w, l, &own, 2 * (n % B), config);
        check_optimiser(w, l, step, group_hp, l->n_groups);
        for (int64_t k = 0; k < count; ++k) {
            const int64_t first = k * B, size = std::min(B, n - first);
            // the first of these calls checks the ring before anything is enqueued
            check_rc(az_replay_dev_batch(GAME, ring, idx, order, first, size, &own, stream));
            for (int64_t i = 0; i < l->n_tensors; ++i) l->step_no[i] = step[i] + k;
            train_batch(l, &own, 2 * size, config, l->step_no.data(), group_hp, first_call + static_cast<uint64_t>(k), stream);
            *n_batches = k + 1;
        }
    });
}

int az_learn_dev_eval(az_learn *l, const az_replay_batch *batch, int64_t N, const az_train_loss_config *config, void *stream)
{
    return guarded([&] {
        check_batch("az_learn_dev_eval", l, batch, N, config);
        Keeps none{};
        none.scale = 1.0f;
        forward(l, batch, N, none, false, stream);
        loss(l, batch, N, config, stream);
    });
}

int az_learn_dev_keep(az_learn *l, int64_t N, uint64_t call, void *stream)
{
    return guarded([&] {
        require(l != nullptr, "az_learn_dev_keep: null argument");
        require(N > 0 && N <= l->c.max_rows, "az_learn_dev_keep: N must lie in [1, max_rows]");
        if (!l->any_rate()) return;
        launch_keep(l, N, call, static_cast<hipStream_t>(stream));
        HIP_OK(hipGetLastError());
    });
}

int az_learn_outputs(az_learn *l, az_learn_out *out)
{
    return guarded([&] {
        require(l != nullptr && out != nullptr, "az_learn_outputs: null argument");
        out->sums = l->tally();
        out->batches = reinterpret_cast<int32_t *>(l->tally()) + az::TALLY_BATCHES;
        out->entropy = l->tally() + az::TALLY_ENTROPY;
        out->losses = l->losses();
        out->counts = l->counts();
        out->grad_norm = l->norm();
        out->keep_blocks = l->keep_blocks.p;
        out->keep_block_stride = az::CH * l->c.max_rows;
        out->keep_attn = l->keep_attn.p;
        out->keep_policy = l->keep_policy.p;
        out->keep_pool = l->keep_pool.p;
        out->batch = l->own_batch();
    });
}

int az_learn_reset_sums(az_learn *l, void *stream)
{
    return guarded([&] {
        require(l != nullptr, "az_learn_reset_sums: null argument");
        HIP_OK(hipMemsetAsync(l->tally(), 0, 8 * sizeof(float), static_cast<hipStream_t>(stream)));
    });
}

int az_learn_publish(az_learn *l, struct az_nn_model *m, float *scalars_dev, void *stream)
{
    return guarded([&] {
        const std::string w("az_learn_publish");
        require(l != nullptr && m != nullptr && scalars_dev != nullptr, w + ": null argument");
        require(l->bound, w + ": called before az_learn_bind");
        auto p = [&](int r) { return static_cast<const float *>(l->param[r]); };
        az_nn_publish_src s{};
        s.piece_emb = p(AZ_LEARN_ROLE_PIECE_EMB); s.pos_emb = p(AZ_LEARN_ROLE_POS_EMB);
        s.stem_conv_weight = p(AZ_LEARN_ROLE_STEM_CONV_WEIGHT); s.stem_conv_bias = p(AZ_LEARN_ROLE_STEM_CONV_BIAS);
        s.n_blocks = l->c.n_blocks;
        for (int k = 0; k < l->c.n_blocks; ++k) {
            s.block_norm_weight[k] = p(AZ_LEARN_ROLE_BLOCK + 4 * k); s.block_norm_bias[k] = p(AZ_LEARN_ROLE_BLOCK + 4 * k + 1);
            s.block_conv_weight[k] = p(AZ_LEARN_ROLE_BLOCK + 4 * k + 2); s.block_conv_bias[k] = p(AZ_LEARN_ROLE_BLOCK + 4 * k + 3);
        }
        // the six attention tensors and the eighteen head tensors follow in the roles' order
        static_assert(offsetof(az_nn_publish_src, aux_out_bias) - offsetof(az_nn_publish_src, prenorm_weight) == 23 * sizeof(float *) &&
                      AZ_LEARN_ROLE_HEADS == AZ_LEARN_ROLE_ATTN + 6, "az_nn_publish_src ends in 24 pointers in the roles' order");
        const float **f = &s.prenorm_weight;
        for (int i = 0; i < 6 + 18; ++i) f[i] = p(AZ_LEARN_ROLE_ATTN + i);
        const int rc = az_nn_model_publish(m, &s, scalars_dev, stream);
        if (rc != 0) throw AzError(rc, w + ": az_nn_model_publish refused the call (the model's kind or n_blocks, an alignment, a capturing stream)");
    });
}

}  // extern "C"
