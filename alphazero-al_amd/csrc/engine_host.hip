// engine_host.hip - the reference-compatible host entry points of include/az_mcts.h: synchronous, on the NULL
// stream (they mirror the reference's blocking pybind calls, mcts_bindings.cpp:126-131 etc.), with the host
// generator's draws in the reference's order.
#include "engine_internal.h"

namespace {

// Shared body of search_batch / search_batch_vl (BatchedMCTS.h:119-171, 227-286)
void host_search(az_mcts *m, int K, bool vl, const int8_t *boards, const int32_t *turns,
                 int8_t *out_boards, float *out_d, float *out_p1w, float *out_p2w,
                 uint8_t *out_is_term, int32_t *out_turns, int32_t *out_sym, uint8_t *out_mask)
{
    HIP_OK(hipSetDevice(m->device));
    const int B = m->B;
    const size_t total = static_cast<size_t>(B) * K;
    hipStream_t s = nullptr;
    m->flush_resets(s);

    const int A = m->geo.actions, CELLS = m->geo.cells;
    m->io_boards_in.ensure(static_cast<size_t>(B) * CELLS);
    m->io_turns_in.ensure(B);
    HIP_OK(hipMemcpy(m->io_boards_in.p, boards, static_cast<size_t>(B) * CELLS, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(m->io_turns_in.p, turns, sizeof(int32_t) * B, hipMemcpyHostToDevice));
    az::launch_import(m->game, m->io_boards_in.p, m->io_turns_in.p, m->roots(), B, s);

    LeafStore &ls = vl ? m->vl_leaf : m->plain_leaf;
    ls.ensure(total);
    if (vl) m->vl_stride = K;
    m->last_select_vl = vl;
    const az::SearchParams p = m->params();
    az::launch_select(m->game, m->arena(), m->roots(), ls.view(), p, K, vl, m->counters.p, s);
    ++m->select_launches;

    std::vector<uint8_t> flags(total), nvalid(total);
    HIP_OK(hipMemcpy(flags.data(), ls.flags.p, total, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(nvalid.data(), ls.nvalid.p, total, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out_turns, ls.turn.p, sizeof(int32_t) * total, hipMemcpyDeviceToHost));

    // symmetry ids in env order, one draw per NON-terminal leaf (BatchedMCTS.h:148-158,261-271)
    std::vector<int32_t> sym(total, 0);
    const bool use_sym = m->cfg.use_symmetry != 0;
    for (size_t f = 0; f < total; ++f) {
        const bool term = (flags[f] & az::LEAF_TERMINAL) != 0;
        const int code = (flags[f] >> az::LEAF_RESULT_SHIFT) & 3;
        out_is_term[f] = term ? 1 : 0;
        out_d[f] = (term && code == 0) ? 1.0f : 0.0f;
        out_p1w[f] = (term && code == 1) ? 1.0f : 0.0f;
        out_p2w[f] = (term && code == 2) ? 1.0f : 0.0f;
        if (!term && use_sym) {               // Connect4: id in {0,1}; Othello: {0,2,6,7}[index] (Othello.h:363-367)
            const int choice = m->rng.uniform_int(m->geo.sym_choices - 1);
            static const int ot_ids[4] = {0, 2, 6, 7};
            sym[f] = m->game == AZ_GAME_OTHELLO ? ot_ids[choice] : choice;
        }
    }
    if (out_sym) std::memcpy(out_sym, sym.data(), sizeof(int32_t) * total);
    HIP_OK(hipMemcpy(ls.sym.p, sym.data(), sizeof(int32_t) * total, hipMemcpyHostToDevice));

    m->io_boards_out.ensure(total * CELLS);
    m->io_mask_out.ensure(total * A);
    az::launch_export(m->game, ls.view(), p, static_cast<int>(total), false, m->io_boards_out.p,
                      m->io_mask_out.p, nullptr, s);
    HIP_OK(hipMemcpy(out_boards, m->io_boards_out.p, total * CELLS, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(out_mask, m->io_mask_out.p, total * A, hipMemcpyDeviceToHost));

    // what the host generator needs at expansion time: which leaves are unexpanded roots and how
    // many legal moves (= noise draws) such a root has
    for (int i = 0; i < B; ++i)
        for (int k = 0; k < K; ++k) {
            const size_t f = static_cast<size_t>(i) * K + k;
            if (flags[f] & az::LEAF_ROOT_UNEXPANDED) { m->stash_root_nv[i] = nvalid[f]; break; }
        }
    (vl ? m->stash_flags_vl : m->stash_flags_plain) = std::move(flags);
}

// Shared body of backprop_batch / backprop_batch_vl (BatchedMCTS.h:176-199, 296-332)
void host_backprop(az_mcts *m, int K, bool vl, const float *policy, const float *d, const float *p1w,
                   const float *p2w, const float *ml, const uint8_t *is_term, const int32_t *sym_ids)
{
    HIP_OK(hipSetDevice(m->device));
    const int B = m->B;
    const int A = m->geo.actions;
    hipStream_t s = nullptr;
    m->flush_resets(s);
    LeafStore &ls = vl ? m->vl_leaf : m->plain_leaf;
    if (vl) require(m->vl_stride == K, "backprop_batch_vl: K differs from the preceding search_batch_vl");
    const size_t total = static_cast<size_t>(B) * K;
    ls.ensure(total);
    m->ensure_room(static_cast<int64_t>(K) * m->geo.max_edges);

    // Dirichlet noise for roots expanded by this call, drawn in env order (MCTS.h:347-363)
    m->io_noise.ensure(static_cast<size_t>(B) * A, true);
    const std::vector<uint8_t> &fl = vl ? m->stash_flags_vl : m->stash_flags_plain;
    if (m->cfg.dirichlet_alpha > 0.0f && fl.size() == total) {
        std::vector<float> noise(static_cast<size_t>(B) * A, 0.0f);
        bool any = false;
        for (int i = 0; i < B; ++i)
            for (int k = 0; k < K; ++k) {
                const size_t f = static_cast<size_t>(i) * K + k;
                if ((fl[f] & az::LEAF_ROOT_UNEXPANDED) && !is_term[f]) {
                    m->rng.dirichlet(m->cfg.dirichlet_alpha, &noise[static_cast<size_t>(i) * A],
                                     m->stash_root_nv[i]);
                    any = true;
                    break;   // later k find the root expanded (MCTS.h:601-607)
                }
            }
        if (any)
            HIP_OK(hipMemcpy(m->io_noise.p, noise.data(), sizeof(float) * noise.size(), hipMemcpyHostToDevice));
    }
    (vl ? m->stash_flags_vl : m->stash_flags_plain).clear();

    m->io_policy.ensure(total * A); m->io_d.ensure(total); m->io_p1.ensure(total);
    m->io_p2.ensure(total); m->io_ml.ensure(total); m->io_is_term.ensure(total);
    HIP_OK(hipMemcpy(m->io_policy.p, policy, sizeof(float) * total * A, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(m->io_d.p, d, sizeof(float) * total, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(m->io_p1.p, p1w, sizeof(float) * total, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(m->io_p2.p, p2w, sizeof(float) * total, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(m->io_ml.p, ml, sizeof(float) * total, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(m->io_is_term.p, is_term, total, hipMemcpyHostToDevice));
    az::EvalIn in{};
    in.policy = m->io_policy.p; in.d = m->io_d.p; in.p1w = m->io_p1.p; in.p2w = m->io_p2.p;
    in.is_term = m->io_is_term.p; in.moves_left = m->io_ml.p; in.wdl_rel = nullptr;
    in.root_noise = m->io_noise.p;
    in.sym = nullptr;   // plain: the ids stored by search_batch (pending_sym_ids_, BatchedMCTS.h:152)
    if (vl) {
        m->io_sym_in.ensure(total);
        HIP_OK(hipMemcpy(m->io_sym_in.p, sym_ids, sizeof(int32_t) * total, hipMemcpyHostToDevice));
        in.sym = m->io_sym_in.p;
    }
    az::launch_backprop(m->game, m->arena(), ls.view(), m->params(), K, vl, false, in, m->counters.p, m->err.p, s);
    ++m->backprop_launches;
    HIP_OK(hipStreamSynchronize(s));
    m->check_device_error();
}

// RolloutEvaluator::evaluate_single (RolloutEvaluator.h:23-48) on the host: result of a uniformly
// random playout from `s` - 0 draw, 1 P1 wins, 2 P2 wins - with one uniform_int(0, nv-1) draw per move
template <class G>
int host_playout(az::GameState s, az::HostRng &rng)
{
    for (;;) {
        const int res = G::result(s);
        if (res >= 0) return res;
        const int nv = G::num_valid(s);
        if (nv <= 0) return 0;
        G::step(s, G::nth_valid(s, rng.uniform_int(nv - 1)));
    }
}

void rollout_common_begin(az_mcts *m, const int8_t *boards, const int32_t *turns, int64_t n, int n_playout, hipStream_t s)
{
    require(n == m->B, "search: input_boards batch size (" + std::to_string(n) + ") must match n_envs (" +
                           std::to_string(m->B) + ")");
    require(n_playout >= 0, "search: n_playout must be >= 0");
    HIP_OK(hipSetDevice(m->device));
    const int B = m->B;
    const int A = m->geo.actions, CELLS = m->geo.cells;
    m->flush_resets(s);
    m->io_boards_in.ensure(static_cast<size_t>(B) * CELLS);
    m->io_turns_in.ensure(B);
    HIP_OK(hipMemcpy(m->io_boards_in.p, boards, static_cast<size_t>(B) * CELLS, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(m->io_turns_in.p, turns, sizeof(int32_t) * B, hipMemcpyHostToDevice));
    az::launch_import(m->game, m->io_boards_in.p, m->io_turns_in.p, m->roots(), B, s);
    m->plain_leaf.ensure(B);
    HIP_OK(hipMemset(m->plain_leaf.sym.p, 0, sizeof(int32_t) * B));
    m->io_policy.ensure(static_cast<size_t>(B) * A); m->io_d.ensure(B); m->io_p1.ensure(B);
    m->io_p2.ensure(B); m->io_ml.ensure(B); m->io_is_term.ensure(B);
    m->ensure_room(static_cast<int64_t>(n_playout) * m->geo.max_edges);
    m->last_select_vl = false;
}
}  // namespace

extern "C" {

int az_mcts_prune_roots(az_mcts *m, const int32_t *actions, int64_t n)
{
    return guarded([&] {
        require(n == m->B, "prune_roots: actions size (" + std::to_string(n) + ") must match n_envs (" +
                               std::to_string(m->B) + ")");
        HIP_OK(hipSetDevice(m->device));
        hipStream_t s = nullptr;
        m->flush_resets(s);
        const int B = m->B;
        const int A = m->geo.actions;
        m->io_actions.ensure(B); m->io_noise_req.ensure(B, true);
        HIP_OK(hipMemcpy(m->io_actions.p, actions, sizeof(int32_t) * B, hipMemcpyHostToDevice));
        m->prune_on(m->io_actions.p, m->io_noise_req.p, false, nullptr, s);
        if (m->cfg.dirichlet_alpha > 0.0f) {  // apply_root_noise, env order (MCTS.h:113-132)
            std::vector<int32_t> req(B);
            HIP_OK(hipMemcpy(req.data(), m->io_noise_req.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
            std::vector<float> noise(static_cast<size_t>(B) * A, 0.0f);
            bool any = false;
            for (int i = 0; i < B; ++i)
                if (req[i] > 0) {
                    m->rng.dirichlet(m->cfg.dirichlet_alpha, &noise[static_cast<size_t>(i) * A], req[i]);
                    any = true;
                }
            if (any) {
                m->io_noise.ensure(static_cast<size_t>(B) * A);
                HIP_OK(hipMemcpy(m->io_noise.p, noise.data(), sizeof(float) * noise.size(), hipMemcpyHostToDevice));
                az::launch_apply_noise(m->game, m->arena(), m->io_noise_req.p, m->io_noise.p, s);
            }
        }
        HIP_OK(hipStreamSynchronize(s));
    });
}

int az_mcts_search_batch(az_mcts *m, const int8_t *boards, const int32_t *turns, int64_t n,
                         int8_t *out_boards, float *out_term_d, float *out_term_p1w,
                         float *out_term_p2w, uint8_t *out_is_term, int32_t *out_turns,
                         uint8_t *out_valid_mask)
{
    return guarded([&] {
        require(n == m->B, "search_batch: input_boards batch size (" + std::to_string(n) +
                               ") must match n_envs (" + std::to_string(m->B) + ")");
        host_search(m, 1, false, boards, turns, out_boards, out_term_d, out_term_p1w, out_term_p2w,
                    out_is_term, out_turns, nullptr, out_valid_mask);
    });
}

int az_mcts_backprop_batch(az_mcts *m, const float *policy, const float *d, const float *p1w,
                           const float *p2w, const float *moves_left, const uint8_t *is_term,
                           int64_t n)
{
    return guarded([&] {
        require(n == m->B, "backprop_batch: policy_logits batch size (" + std::to_string(n) +
                               ") must match n_envs (" + std::to_string(m->B) + ")");
        host_backprop(m, 1, false, policy, d, p1w, p2w, moves_left, is_term, nullptr);
    });
}

int az_mcts_remove_all_vl(az_mcts *m, int K)
{
    return guarded([&] {
        HIP_OK(hipSetDevice(m->device));
        if (m->vl_stride <= 0 || K <= 0) return;
        const int kk = std::min(K, m->vl_stride);          // safe_K, MCTS.h:563
        az::launch_remove_vl(m->game, m->arena(), m->vl_leaf.view(), m->params(), kk, m->vl_stride, nullptr);
        HIP_OK(hipStreamSynchronize(nullptr));
    });
}

int az_mcts_search_batch_vl(az_mcts *m, int K, const int8_t *boards, const int32_t *turns,
                            int64_t n, int8_t *out_boards, float *out_term_d,
                            float *out_term_p1w, float *out_term_p2w, uint8_t *out_is_term,
                            int32_t *out_turns, int32_t *out_sym_ids, uint8_t *out_valid_mask)
{
    return guarded([&] {
        require(n == m->B, "search_batch_vl: input batch (" + std::to_string(n) + ") != n_envs (" +
                               std::to_string(m->B) + ")");
        require(K >= 1, "search_batch_vl: K must be >= 1");
        host_search(m, K, true, boards, turns, out_boards, out_term_d, out_term_p1w, out_term_p2w,
                    out_is_term, out_turns, out_sym_ids, out_valid_mask);
    });
}

int az_mcts_backprop_batch_vl(az_mcts *m, int K, const float *policy, const float *d,
                              const float *p1w, const float *p2w, const float *moves_left,
                              const uint8_t *is_term, const int32_t *sym_ids, int64_t total)
{
    return guarded([&] {
        require(K >= 1, "backprop_batch_vl: K must be >= 1");
        require(total == static_cast<int64_t>(m->B) * K,
                "backprop_batch_vl: policy batch (" + std::to_string(total) + ") != N*K (" +
                    std::to_string(static_cast<int64_t>(m->B) * K) + ")");
        host_backprop(m, K, true, policy, d, p1w, p2w, moves_left, is_term, sym_ids);
    });
}

// BatchedMCTS::search with RolloutEvaluator (BatchedMCTS.h:339-407, RolloutEvaluator.h:23-48) in the
// REFERENCE'S random stream: per playout, selection on the device; then the playout moves of the
// non-terminal leaves in env order and the root-noise rows of the expansions in env order, both from
// the host mt19937 exactly as the reference (OMP_NUM_THREADS=1) consumes them; expansion and backup on
// the device.  Bit-exact against the reference (fixture G9); one host round trip per playout.
int az_mcts_search_rollout(az_mcts *m, const int8_t *boards, const int32_t *turns, int64_t n, int n_playout)
{
    return guarded([&] {
        hipStream_t s = nullptr;
        rollout_common_begin(m, boards, turns, n, n_playout, s);
        const int B = m->B, A = m->geo.actions;
        const az::SearchParams p = m->params();
        m->io_noise.ensure(static_cast<size_t>(B) * A, true);
        az::EvalIn in{};
        in.policy = m->io_policy.p; in.d = m->io_d.p; in.p1w = m->io_p1.p; in.p2w = m->io_p2.p;
        in.is_term = m->io_is_term.p; in.moves_left = m->io_ml.p; in.sym = nullptr; in.root_noise = m->io_noise.p;
        HIP_OK(hipMemset(m->io_ml.p, 0, sizeof(float) * B));
        std::vector<uint8_t> flags(B), nvalid(B), is_term(B);
        std::vector<uint64_t> bb0(B), bb1(B);
        std::vector<int32_t> turn(B), aux(B);
        std::vector<float> pol(static_cast<size_t>(B) * A), d(B), p1(B), p2(B), noise(static_cast<size_t>(B) * A);
        LeafStore &ls = m->plain_leaf;
        for (int it = 0; it < n_playout; ++it) {
            az::launch_select(m->game, m->arena(), m->roots(), ls.view(), p, 1, false, m->counters.p, s);
            HIP_OK(hipMemcpy(flags.data(), ls.flags.p, B, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(nvalid.data(), ls.nvalid.p, B, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(bb0.data(), ls.bb0.p, sizeof(uint64_t) * B, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(bb1.data(), ls.bb1.p, sizeof(uint64_t) * B, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(turn.data(), ls.turn.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
            HIP_OK(hipMemcpy(aux.data(), ls.aux.p, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
            // phase 2: evaluate_batch over the non-terminal leaves, in order
            for (int i = 0; i < B; ++i) {
                const bool term = (flags[i] & az::LEAF_TERMINAL) != 0;
                int code = (flags[i] >> az::LEAF_RESULT_SHIFT) & 3;
                if (!term) {
                    az::GameState st{bb0[i], bb1[i], turn[i], aux[i]};
                    code = m->game == AZ_GAME_OTHELLO ? host_playout<az::OthelloDev>(st, m->rng)
                                                      : host_playout<az::Connect4Dev>(st, m->rng);
                }
                is_term[i] = term ? 1 : 0;
                d[i] = code == 0 ? 1.0f : 0.0f; p1[i] = code == 1 ? 1.0f : 0.0f; p2[i] = code == 2 ? 1.0f : 0.0f;
                std::fill(pol.begin() + static_cast<size_t>(i) * A, pol.begin() + static_cast<size_t>(i + 1) * A, term ? 0.0f : 1.0f);
            }
            // phase 3: root expansions draw their noise in env order (MCTS.h:347-363)
            bool any_noise = false;
            if (m->cfg.dirichlet_alpha > 0.0f)
                for (int i = 0; i < B; ++i)
                    if ((flags[i] & az::LEAF_ROOT_UNEXPANDED) && !is_term[i]) {
                        m->rng.dirichlet(m->cfg.dirichlet_alpha, &noise[static_cast<size_t>(i) * A], nvalid[i]);
                        any_noise = true;
                    }
            if (any_noise) HIP_OK(hipMemcpy(m->io_noise.p, noise.data(), sizeof(float) * noise.size(), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(m->io_policy.p, pol.data(), sizeof(float) * pol.size(), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(m->io_d.p, d.data(), sizeof(float) * B, hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(m->io_p1.p, p1.data(), sizeof(float) * B, hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(m->io_p2.p, p2.data(), sizeof(float) * B, hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(m->io_is_term.p, is_term.data(), B, hipMemcpyHostToDevice));
            az::launch_backprop(m->game, m->arena(), ls.view(), p, 1, false, false, in, m->counters.p, m->err.p, s);
        }
        m->select_launches += n_playout;
        m->backprop_launches += n_playout;
        HIP_OK(hipStreamSynchronize(s));
        m->check_device_error();
    });
}

// The same search with the playouts on the device (k_rollout: one thread per tree, moves and root noise
// from the device generator): no host round trip inside the loop, same distribution, a different stream.
int az_mcts_search_rollout_dev(az_mcts *m, const int8_t *boards, const int32_t *turns, int64_t n, int n_playout)
{
    return guarded([&] {
        hipStream_t s = nullptr;
        rollout_common_begin(m, boards, turns, n, n_playout, s);
        const int B = m->B;
        const az::SearchParams p = m->params();
        az::EvalIn in{};
        in.policy = m->io_policy.p; in.d = m->io_d.p; in.p1w = m->io_p1.p; in.p2w = m->io_p2.p;
        in.is_term = m->io_is_term.p; in.moves_left = m->io_ml.p; in.sym = nullptr; in.root_noise = nullptr;
        for (int it = 0; it < n_playout; ++it) {
            az::launch_select(m->game, m->arena(), m->roots(), m->plain_leaf.view(), p, 1, false, m->counters.p, s);
            az::launch_rollout(m->game, m->plain_leaf.view(), p, B, m->io_policy.p, m->io_d.p, m->io_p1.p, m->io_p2.p,
                               m->io_ml.p, m->io_is_term.p, s);
            az::launch_backprop(m->game, m->arena(), m->plain_leaf.view(), p, 1, false, false, in, m->counters.p, m->err.p, s);
            az::launch_bump_call(m->call_ctr.p, s);
        }
        m->select_launches += n_playout;
        m->backprop_launches += n_playout;
        HIP_OK(hipStreamSynchronize(s));
        m->check_device_error();
    });
}

int az_mcts_get_all_counts(az_mcts *m, int32_t *out)
{
    return guarded([&] {
        HIP_OK(hipSetDevice(m->device));
        m->flush_resets(nullptr);
        const int A = m->geo.actions;
        m->io_counts.ensure(static_cast<size_t>(m->B) * A);
        az::launch_counts(m->game, m->arena(), m->io_counts.p, nullptr);
        HIP_OK(hipMemcpy(out, m->io_counts.p, sizeof(int32_t) * m->B * A, hipMemcpyDeviceToHost));
    });
}

int az_mcts_get_all_root_stats(az_mcts *m, float *out)
{
    return guarded([&] {
        HIP_OK(hipSetDevice(m->device));
        m->flush_resets(nullptr);
        const int STATS = m->geo.stats;
        m->io_stats.ensure(static_cast<size_t>(m->B) * STATS);
        az::launch_root_stats(m->game, m->arena(), m->io_stats.p, nullptr);
        HIP_OK(hipMemcpy(out, m->io_stats.p, sizeof(float) * m->B * STATS, hipMemcpyDeviceToHost));
    });
}

}  // extern "C"
