// engine_dev.hip - the device entry points of include/az_mcts.h (they only enqueue work on the caller's stream),
// the native search loop with the evaluator inside it, and the host side of the device transposition table.
#include "engine_internal.h"

namespace {
// stream == nullptr with whole_device: everything on the device is waited for (callers that do not
// say which stream their trees are being worked on)
void dev_prepare(az_mcts *m, int K, int64_t sims_per_tree, hipStream_t s, bool whole_device)
{
    require(K >= 1, "dev_prepare: K must be >= 1");
    HIP_OK(hipSetDevice(m->device));
    const size_t total = static_cast<size_t>(m->B) * K;
    const int64_t extra = sims_per_tree * m->geo.max_edges;
    // Reading the trees' fill (`used`), moving the arenas or the leaf buffers, refreshing the tables:
    // all of that must see what the kernels already enqueued have done, and must not pull memory
    // from under them.  Wait for them first - once per many calls (the host-side bound `used_bound`
    // runs ahead of the real fill by at most one call's worth).
    const bool touches = m->any_pending_reset || total > m->vl_leaf.slot.n || static_cast<size_t>(m->B) > m->plain_leaf.slot.n ||
                         !m->tab.p || !m->term_tab.p || m->cfg.c_init != m->tab_c_init || m->cfg.c_base != m->tab_c_base ||
                         m->cfg.score_scale != m->term_tab_scale || m->room_needs_device(extra);
    if (touches) {
        if (whole_device) HIP_OK(hipDeviceSynchronize());
        else HIP_OK(hipStreamSynchronize(s));
    }
    m->flush_resets(s);
    if (total > m->vl_leaf.slot.n) ++m->epoch;
    m->vl_leaf.ensure(total);
    m->plain_leaf.ensure(m->B);
    m->ensure_table();
    m->ensure_room(extra);
}

// One selection step on `stream`: the selection launch (inside the profiling bracket), the leaves' symmetry ids
// from the replay tape where one is set, then `tail(ls, p, total, gen_sym, s)` - the one launch in which the two
// forms of the step below differ.  Enqueued in exactly that order; the whole step is captured into graphs.
// zero_count: an int64 in device memory that the selection launch clears on its way (the
// live-leaf count of az_mcts_dev_search: saves the memset in front of the listing kernel)
template <class Tail>
void select_step(az_mcts *m, int K, int vl, void *stream, int64_t *zero_count, Tail &&tail)
{
    require(K >= 1 && (vl || K == 1), "dev_select: K must be 1 without virtual loss");
    LeafStore &ls = vl ? m->vl_leaf : m->plain_leaf;
    const size_t total = static_cast<size_t>(m->B) * K;
    require(ls.slot.n >= total && m->tab.p, "dev_select: call az_mcts_dev_prepare first");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (vl) m->vl_stride = K;
    m->last_select_vl = vl != 0;
    const az::SearchParams p = m->params();
    const bool timed = m->profiling && (m->profile_seen[0]++ % m->profile_stride) == 0 && m->ev_select.begin(s);
    const char *kn = az::launch_select(m->game, m->arena(), m->roots(), ls.view(), p, K, vl != 0, m->counters.p, s, m->call_ctr.p, zero_count);
    if (timed) { m->ev_select.end(s); m->timed_select_kernel = kn; }
    bool gen_sym = true;
    if (m->replay_sym != nullptr) {             // recorded symmetry ids instead of the generator's
        if (m->replay_next >= m->replay_calls || static_cast<int64_t>(total) > m->replay_stride)
            throw AzError(AZ_ERR_STATE, "dev_select: the replay tape (az_mcts_dev_replay) is exhausted or too narrow");
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
            throw AzError(AZ_ERR_STATE, "dev_select: a replay tape cannot be captured into a graph (its position moves per call)");
        HIP_OK(hipMemcpyAsync(ls.sym.p, m->replay_sym + m->replay_next * m->replay_stride, sizeof(int32_t) * total,
                              hipMemcpyDeviceToDevice, s));
        ++m->replay_next;
        gen_sym = false;
    }
    tail(ls, p, static_cast<int>(total), gen_sym, s);
    ++m->select_launches;
}

// selection, then the gather of the leaves into feature planes and action masks
void select_and_gather(az_mcts *m, int K, int vl, float *features, uint8_t *valid_mask, void *stream, int64_t *zero_count)
{
    select_step(m, K, vl, stream, zero_count, [&](LeafStore &ls, const az::SearchParams &p, int total, bool gen_sym, hipStream_t s) {
        az::launch_export(m->game, ls.view(), p, total, gen_sym, nullptr, valid_mask, features, s);
    });
}

// The native loop's form of the same step: selection, then - instead of the gather into feature planes - the
// leaves' symmetry ids, action masks and (unless the table's lookup builds it) the compact list of leaves to
// evaluate, for an evaluator that reads the leaf positions themselves (az_nn_model_forward_positions).
void select_and_prep(az_mcts *m, int K, int vl, uint8_t *valid_mask, int32_t *rows, int64_t *n_rows, void *stream)
{
    select_step(m, K, vl, stream, n_rows, [&](LeafStore &ls, const az::SearchParams &p, int total, bool gen_sym, hipStream_t s) {
        az::launch_leaf_prep(m->game, ls.view(), p, total, gen_sym, valid_mask, rows, n_rows, m->err.p, s);
    });
}

// the evaluator model must be one for the engine's game (w: the entry point's name in its error texts)
void require_model_for(const az_mcts *m, const az_nn_model *model, const std::string &w)
{
    require(model != nullptr, w + ": no evaluator model");
    const int kind = az_nn_model_kind(model);
    require(kind == (m->game == AZ_GAME_CONNECT4 ? AZ_NN_KIND_HASH_CONNECT4 : AZ_NN_KIND_HASH_OTHELLO) ||
                (kind == AZ_NN_KIND_CONNECT4_CNN && m->game == AZ_GAME_CONNECT4) ||
                (kind == AZ_NN_KIND_OTHELLO_CNN && m->game == AZ_GAME_OTHELLO),
            w + ": the evaluator model does not belong to this engine's game");
}

// The reference's iteration schedule (MCTS_cpp.py:110-113, 217-264: one plain simulation that
// expands every root, then ceil((n_playout-1)/K) virtual-loss batches) with the evaluator in the
// loop, issued from native code: per iteration selection + gather, the list of leaves to evaluate,
// the six evaluator launches, backup.  Nothing here waits for the device once the buffers exist.
// warmup: the schedule of a whole search (one plain simulation first, MCTS_cpp.py:217-248); without it the call
// CONTINUES a search: n_playout more simulations in virtual-loss batches of K (plain ones for K <= 1)
int dev_search_impl(az_mcts *m, const az_nn_model *model, int n_playout, int K, int use_table, bool warmup, void *stream)
{
    return guarded([&] {
        require_model_for(m, model, "dev_search");
        require(K >= 1 && n_playout >= 0, "dev_search: K must be >= 1 and n_playout >= 0");
        require(!use_table || m->tt_entries.p != nullptr, "dev_search: no table (az_mcts_dev_tt_create)");
        hipStream_t s = static_cast<hipStream_t>(stream);
        HIP_OK(hipSetDevice(m->device));
        const size_t total = static_cast<size_t>(m->B) * K;
        const size_t scratch = az_nn_model_scratch_bytes(model, static_cast<int64_t>(total));
        const int64_t extra = static_cast<int64_t>(n_playout) * m->geo.max_edges;
        const bool grows = total > m->vl_leaf.slot.n || total > m->ev_rows.n || scratch > m->ev_scratch.n ||
                           m->room_needs_device(extra) || (use_table && m->tt_keys.n < 2 * total);
        // anything below that allocates, frees or reads a buffer the stream's kernels use waits for them first
        if (grows) HIP_OK(hipStreamSynchronize(s));
        dev_prepare(m, K, n_playout, s, false);
        if (total > m->ev_rows.n) {
            m->ev_feat.ensure(total * 3 * m->geo.cells); m->ev_mask.ensure(total * m->geo.actions);
            m->ev_probs.ensure(total * m->geo.actions); m->ev_wdl.ensure(total * 3); m->ev_ml.ensure(total);
            m->ev_rows.ensure(total); m->ev_nrows.ensure(1, true);
        }
        m->ev_scratch.ensure(scratch);
        if (use_table && m->tt_keys.n < 2 * total) { m->tt_keys.ensure(2 * total); ++m->epoch; }

        auto ok = [&](int rc, const char *what) {
            if (rc != AZ_OK) throw AzError(AZ_ERR_DEVICE, std::string("dev_search: ") + what + ": " + g_last_error);
        };
        // AZ_SEARCH_FEATURES=1: the first form of the loop - leaves gathered into feature planes (k_export), the
        // list from k_live_leaves - kept for A/B runs; default: the evaluator reads the leaf positions
        static const bool via_features = getenv("AZ_SEARCH_FEATURES") != nullptr && getenv("AZ_SEARCH_FEATURES")[0] == '1';
        auto iteration = [&](int k, int vl) {
            const int64_t n = static_cast<int64_t>(m->B) * k;
            LeafStore &ls = vl ? m->vl_leaf : m->plain_leaf;
            if (via_features) {
                select_and_gather(m, k, vl, m->ev_feat.p, m->ev_mask.p, stream, use_table ? nullptr : m->ev_nrows.p);
                if (!use_table)
                    az::launch_live_leaves(ls.view(), static_cast<int>(n), m->ev_rows.p, m->ev_nrows.p, m->err.p, s, false);
            } else {
                // the selection launch clears the count; with the table its lookup builds the list instead
                select_and_prep(m, k, vl, m->ev_mask.p, use_table ? nullptr : m->ev_rows.p, use_table ? nullptr : m->ev_nrows.p, stream);
            }
            if (use_table)
                ok(az_mcts_dev_tt_lookup(m, k, m->ev_probs.p, m->ev_wdl.p, m->ev_ml.p, m->ev_rows.p, m->ev_nrows.p, stream), "tt_lookup");
            int rc;
            if (via_features) {
                rc = az_nn_model_forward(model, m->ev_feat.p, m->ev_mask.p, m->ev_probs.p, m->ev_wdl.p, m->ev_ml.p, n,
                                         m->ev_rows.p, m->ev_nrows.p, m->ev_scratch.p, m->ev_scratch.n, stream);
            } else {
                const az_nn_positions pos{ls.bb0.p, ls.bb1.p, ls.turn.p, ls.sym.p};
                rc = az_nn_model_forward_positions(model, &pos, m->ev_mask.p, m->ev_probs.p, m->ev_wdl.p, m->ev_ml.p, n,
                                                   m->ev_rows.p, m->ev_nrows.p, m->ev_scratch.p, m->ev_scratch.n, stream);
            }
            if (rc != 0) throw AzError(AZ_ERR_ARG, "dev_search: the evaluator model refused its arguments");
            if (use_table)
                ok(az_mcts_dev_tt_insert(m, k, m->ev_rows.p, m->ev_nrows.p, m->ev_probs.p, m->ev_wdl.p, m->ev_ml.p, stream), "tt_insert");
            ok(az_mcts_dev_backprop(m, k, vl, m->ev_probs.p, m->ev_wdl.p, m->ev_ml.p, stream), "backprop");
        };
        int remaining = n_playout;
        if (K <= 1) {
            for (; remaining > 0; --remaining) iteration(1, 0);
            return;
        }
        if (warmup && remaining > 0) { iteration(1, 0); --remaining; }
        while (remaining > 0) {
            const int k = std::min(K, remaining);
            remaining -= k;
            iteration(k, 1);
        }
    });
}
}  // namespace

extern "C" {

int az_mcts_dev_prepare(az_mcts *m, int K, int64_t sims_per_tree)
{
    return guarded([&] { dev_prepare(m, K, sims_per_tree, nullptr, true); });
}

int az_mcts_dev_prepare_stream(az_mcts *m, int K, int64_t sims_per_tree, void *stream)
{
    return guarded([&] { dev_prepare(m, K, sims_per_tree, static_cast<hipStream_t>(stream), false); });
}

int az_mcts_dev_check(az_mcts *m, void *stream)
{
    return guarded([&] {
        const int seen = *static_cast<volatile int *>(m->err_host);
        HIP_OK(hipMemcpyAsync(m->err_host, m->err.p, sizeof(int), hipMemcpyDeviceToHost, static_cast<hipStream_t>(stream)));
        if (seen) throw AzError(AZ_ERR_CAPACITY, az_mcts::device_error_text(seen));
    });
}

int az_mcts_dev_replay(az_mcts *m, const int32_t *sym_ids, int64_t sym_stride, int64_t n_select_calls,
                       const float *root_noise)
{
    return guarded([&] {
        require(sym_ids == nullptr || (sym_stride > 0 && n_select_calls > 0), "dev_replay: a symmetry tape needs a stride and a length");
        m->replay_sym = sym_ids;
        m->replay_stride = sym_ids ? sym_stride : 0;
        m->replay_calls = sym_ids ? n_select_calls : 0;
        m->replay_next = 0;
        m->replay_noise = root_noise;
    });
}

int az_mcts_dev_set_roots(az_mcts *m, const uint64_t *bb_p1, const uint64_t *bb_p2,
                          const int32_t *turns, void *stream)
{
    return guarded([&] {
        az::launch_set_roots(m->game, bb_p1, bb_p2, turns, m->roots(), m->B, static_cast<hipStream_t>(stream));
    });
}

int az_mcts_dev_import_roots(az_mcts *m, const int8_t *boards, const int32_t *turns, void *stream)
{
    return guarded([&] {
        az::launch_import(m->game, boards, turns, m->roots(), m->B, static_cast<hipStream_t>(stream));
    });
}

int az_mcts_dev_select(az_mcts *m, int K, int vl, float *features, uint8_t *valid_mask, void *stream)
{
    return guarded([&] { select_and_gather(m, K, vl, features, valid_mask, stream, nullptr); });
}

int az_mcts_dev_backprop(az_mcts *m, int K, int vl, const float *probs, const float *wdl_rel,
                         const float *moves_left, void *stream)
{
    return guarded([&] {
        require(K >= 1 && (vl || K == 1), "dev_backprop: K must be 1 without virtual loss");
        if (vl) require(m->vl_stride == K, "dev_backprop: K differs from the preceding dev_select");
        LeafStore &ls = vl ? m->vl_leaf : m->plain_leaf;
        az::EvalIn in{};
        in.policy = probs; in.wdl_rel = wdl_rel; in.moves_left = moves_left;
        in.root_noise = m->replay_noise; in.sym = nullptr;
        hipStream_t s = static_cast<hipStream_t>(stream);
        const bool timed = m->profiling && (m->profile_seen[1]++ % m->profile_stride) == 0 && m->ev_backprop.begin(s);
        az::launch_backprop(m->game, m->arena(), ls.view(), m->params(), K, vl != 0, true, in, m->counters.p,
                            m->err.p, s);
        if (timed) m->ev_backprop.end(s);
        ++m->backprop_launches;
    });
}

int az_mcts_dev_set_noise_epsilons(az_mcts *m, const float *per_tree)
{
    return guarded([&] { m->noise_eps_tree = per_tree; });
}

int az_mcts_dev_live_leaves(az_mcts *m, int K, int32_t *leaf_idx, int64_t *leaf_count, void *stream)
{
    return guarded([&] {
        LeafStore &ls = m->last_select_vl ? m->vl_leaf : m->plain_leaf;
        const size_t total = static_cast<size_t>(m->B) * K;
        require(K >= 1 && ls.slot.n >= total, "dev_live_leaves: no selection of that width");
        az::launch_live_leaves(ls.view(), static_cast<int>(total), leaf_idx, leaf_count, m->err.p, static_cast<hipStream_t>(stream));
    });
}

int az_mcts_dev_search(az_mcts *m, const az_nn_model *model, int n_playout, int K, int use_table, void *stream)
{
    return dev_search_impl(m, model, n_playout, K, use_table, true, stream);
}

int az_mcts_dev_search_more(az_mcts *m, const az_nn_model *model, int n_sims, int K, int use_table, void *stream)
{
    return dev_search_impl(m, model, n_sims, K, use_table, false, stream);
}

// One launch of k_rollout_search must stay far below a second for Othello at depth.  Measured on an MI355X
// (profiles/r21_measure_elo.jsonl: 1000 playouts from the initial position, the longest playouts a game has): a
// simulation costs a launch 114 us with 1 or 256 Othello trees and 329 us with 4096 (four wavefronts per SIMD, each
// playing its tree's playout in every lane); Connect4 15-25 us.  256 x 329 us = 84 ms per launch at the worst measured
// point, and a 1000-playout move is four launches and the bump instead of 4000.
constexpr int kRolloutChunk = 256;

int az_mcts_dev_rollout_search(az_mcts *m, int n_playout, int sims_per_launch, void *stream)
{
    return guarded([&] {
        require(m != nullptr, "dev_rollout_search: null engine");
        require(n_playout >= 0, "dev_rollout_search: n_playout must be >= 0");
        hipStream_t s = static_cast<hipStream_t>(stream);
        // what rollout_common_begin does for the host route, minus the upload: pending resets, the leaf store (its
        // path rows take the depths past a lane group; the kernel shows every leaf under symmetry id 0 and reads no
        // id), the tables, room for n_playout expansions per tree - waiting for `s` only when one of them touches
        // memory the stream's kernels use
        dev_prepare(m, 1, n_playout, s, false);
        m->last_select_vl = false;
        const az::SearchParams p = m->params();
        const int chunk = sims_per_launch > 0 ? sims_per_launch : kRolloutChunk;
        for (int at = 0; at < n_playout; at += chunk)
            az::launch_rollout_search(m->game, m->arena(), m->roots(), m->plain_leaf.view(), p, std::min(chunk, n_playout - at),
                                      static_cast<uint64_t>(at), m->counters.p, m->err.p, s);
        if (n_playout > 0) az::launch_bump_call(m->call_ctr.p, s, static_cast<uint64_t>(n_playout));
    });
}

// ---- device transposition table ------------------------------------------------------------
int az_mcts_dev_tt_create(az_mcts *m, int log2_entries)
{
    return guarded([&] {
        require(log2_entries >= 2 && log2_entries <= 28, "dev_tt_create: log2_entries must be in [2, 28]");
        HIP_OK(hipSetDevice(m->device));
        HIP_OK(hipDeviceSynchronize());
        const size_t n = (static_cast<size_t>(1) << log2_entries) * az::tt_entry_bytes(m->game);
        if (n != m->tt_entries.n) {
            if (m->tt_entries.p) { HIP_OK(hipFree(m->tt_entries.p)); m->tt_entries.p = nullptr; m->tt_entries.n = 0; }
            m->tt_entries.ensure(n);
            ++m->epoch;
        }
        HIP_OK(hipMemset(m->tt_entries.p, 0, n));
        m->tt_stats.ensure(4, true);
        HIP_OK(hipMemset(m->tt_stats.p, 0, 4 * sizeof(unsigned long long)));
        m->tt_mask = (static_cast<uint64_t>(1) << log2_entries) - 1;
    });
}

int az_mcts_dev_tt_clear(az_mcts *m, void *stream)
{
    return guarded([&] {
        require(m->tt_entries.p != nullptr, "dev_tt_clear: no table (az_mcts_dev_tt_create)");
        HIP_OK(hipMemsetAsync(m->tt_entries.p, 0, m->tt_entries.n, static_cast<hipStream_t>(stream)));
    });
}

int az_mcts_dev_tt_lookup(az_mcts *m, int K, float *probs, float *wdl_rel, float *moves_left, int32_t *miss_idx,
                          int64_t *miss_count, void *stream)
{
    return guarded([&] {
        require(m->tt_entries.p != nullptr, "dev_tt_lookup: no table (az_mcts_dev_tt_create)");
        LeafStore &ls = m->last_select_vl ? m->vl_leaf : m->plain_leaf;
        const size_t total = static_cast<size_t>(m->B) * K;
        require(K >= 1 && ls.slot.n >= total, "dev_tt_lookup: no selection of that width");
        if (m->tt_keys.n < 2 * total) {
            HIP_OK(hipDeviceSynchronize());
            m->tt_keys.ensure(2 * total);
            ++m->epoch;
        }
        az::TtTable t{m->tt_entries.p, m->tt_mask, m->tt_stats.p};
        az::launch_tt_lookup(m->game, ls.view(), static_cast<int>(total), t, m->call_ctr.p, probs, wdl_rel, moves_left, miss_idx,
                             miss_count, m->tt_keys.p, m->err.p, static_cast<hipStream_t>(stream));
    });
}

int az_mcts_dev_tt_insert(az_mcts *m, int K, const int32_t *miss_idx, const int64_t *miss_count, const float *probs,
                          const float *wdl_rel, const float *moves_left, void *stream)
{
    return guarded([&] {
        require(m->tt_entries.p != nullptr, "dev_tt_insert: no table (az_mcts_dev_tt_create)");
        const size_t total = static_cast<size_t>(m->B) * K;
        require(K >= 1 && m->tt_keys.n >= 2 * total, "dev_tt_insert: call az_mcts_dev_tt_lookup on this selection first");
        az::TtTable t{m->tt_entries.p, m->tt_mask, m->tt_stats.p};
        az::launch_tt_insert(m->game, static_cast<int>(total), t, m->call_ctr.p, miss_idx, miss_count, m->tt_keys.p, probs, wdl_rel,
                             moves_left, static_cast<hipStream_t>(stream));
    });
}

int az_mcts_dev_tt_refresh(az_mcts *m, const az_nn_model *model, void *stream)
{
    return guarded([&] {
        require(m->tt_entries.p != nullptr, "dev_tt_refresh: no table (az_mcts_dev_tt_create)");
        require_model_for(m, model, "dev_tt_refresh");
        HIP_OK(hipSetDevice(m->device));
        hipStream_t s = static_cast<hipStream_t>(stream);
        const int64_t chunk = 16384;
        const int A = m->geo.actions;
        const size_t scratch = az_nn_model_scratch_bytes(model, chunk);
        if (m->rf_rows.n < static_cast<size_t>(chunk) || m->rf_scratch.n < scratch) {
            HIP_OK(hipStreamSynchronize(s));
            m->rf_bb0.ensure(chunk); m->rf_bb1.ensure(chunk); m->rf_turn.ensure(chunk); m->rf_sym.ensure(chunk);
            m->rf_mask.ensure(chunk * A); m->rf_probs.ensure(chunk * A);
            m->rf_wdl.ensure(chunk * 3); m->rf_ml.ensure(chunk); m->rf_rows.ensure(chunk); m->rf_keys.ensure(2 * chunk);
            m->rf_count.ensure(1, true); m->rf_scratch.ensure(scratch);
        }
        az::TtTable t{m->tt_entries.p, m->tt_mask, m->tt_stats.p};
        const int64_t entries = static_cast<int64_t>(m->tt_mask) + 1;
        const az_nn_positions pos{m->rf_bb0.p, m->rf_bb1.p, m->rf_turn.p, m->rf_sym.p};
        for (int64_t e0 = 0; e0 < entries; e0 += chunk) {
            const int n = static_cast<int>(std::min<int64_t>(chunk, entries - e0));
            az::launch_tt_refresh_gather(m->game, t, static_cast<uint64_t>(e0), n, m->rf_bb0.p, m->rf_bb1.p, m->rf_turn.p, m->rf_sym.p,
                                         m->rf_mask.p, m->rf_rows.p, m->rf_count.p, m->rf_keys.p, s);
            if (az_nn_model_forward_positions(model, &pos, m->rf_mask.p, m->rf_probs.p, m->rf_wdl.p, m->rf_ml.p, n, m->rf_rows.p,
                                              m->rf_count.p, m->rf_scratch.p, m->rf_scratch.n, stream) != 0)
                throw AzError(AZ_ERR_ARG, "dev_tt_refresh: the evaluator model refused its arguments");
            az::launch_tt_refresh_store(m->game, t, static_cast<uint64_t>(e0), n, m->rf_rows.p, m->rf_count.p, m->rf_keys.p, m->rf_probs.p,
                                        m->rf_wdl.p, m->rf_ml.p, s);
        }
    });
}

int az_mcts_dev_tt_stats(az_mcts *m, int64_t out[4])
{
    return guarded([&] {
        require(m->tt_entries.p != nullptr && out != nullptr, "dev_tt_stats: no table (az_mcts_dev_tt_create)");
        HIP_OK(hipSetDevice(m->device));
        HIP_OK(hipDeviceSynchronize());
        unsigned long long h[4];
        HIP_OK(hipMemcpy(h, m->tt_stats.p, sizeof(h), hipMemcpyDeviceToHost));
        for (int i = 0; i < 4; ++i) out[i] = static_cast<int64_t>(h[i]);
    });
}

int az_mcts_dev_leaves(az_mcts *m, int K, uint64_t *bb_p1, uint64_t *bb_p2, int32_t *turns,
                       uint8_t *flags, void *stream)
{
    return guarded([&] {
        LeafStore &ls = m->last_select_vl ? m->vl_leaf : m->plain_leaf;
        const size_t total = static_cast<size_t>(m->B) * K;
        require(ls.slot.n >= total, "dev_leaves: no selection of that width");
        hipStream_t s = static_cast<hipStream_t>(stream);
        if (bb_p1) HIP_OK(hipMemcpyAsync(bb_p1, ls.bb0.p, 8 * total, hipMemcpyDeviceToDevice, s));
        if (bb_p2) HIP_OK(hipMemcpyAsync(bb_p2, ls.bb1.p, 8 * total, hipMemcpyDeviceToDevice, s));
        if (turns) HIP_OK(hipMemcpyAsync(turns, ls.turn.p, 4 * total, hipMemcpyDeviceToDevice, s));
        if (flags) HIP_OK(hipMemcpyAsync(flags, ls.flags.p, total, hipMemcpyDeviceToDevice, s));
    });
}

int az_mcts_dev_leaf_syms(az_mcts *m, int K, int32_t *sym_ids, void *stream)
{
    return guarded([&] {
        LeafStore &ls = m->last_select_vl ? m->vl_leaf : m->plain_leaf;
        const size_t total = static_cast<size_t>(m->B) * K;
        require(ls.slot.n >= total && sym_ids != nullptr, "dev_leaf_syms: no selection of that width");
        HIP_OK(hipMemcpyAsync(sym_ids, ls.sym.p, 4 * total, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(stream)));
    });
}

int az_mcts_dev_counts(az_mcts *m, int32_t *counts, void *stream)
{
    return guarded([&] { az::launch_counts(m->game, m->arena(), counts, static_cast<hipStream_t>(stream)); });
}

int az_mcts_dev_root_stats(az_mcts *m, float *stats, void *stream)
{
    return guarded([&] { az::launch_root_stats(m->game, m->arena(), stats, static_cast<hipStream_t>(stream)); });
}

int az_mcts_dev_prune_roots(az_mcts *m, const int32_t *actions, void *stream)
{
    return guarded([&] {
        hipStream_t s = static_cast<hipStream_t>(stream);
        HIP_OK(hipSetDevice(m->device));
        m->prune_on(actions, nullptr, true, m->replay_noise, s);
        az::launch_bump_call(m->call_ctr.p, s);
    });
}

int az_mcts_dev_reset_masked(az_mcts *m, const uint8_t *mask, void *stream)
{
    return guarded([&] { az::launch_reset_masked(m->arena(), mask, static_cast<hipStream_t>(stream)); });
}

}  // extern "C"
