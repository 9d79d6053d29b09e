// selfplay_driver.hip - the self-play driver (az_selfplay_*) and the replay export/batch entry points (az_replay_dev_*).
// Whole plies from native code: the search (az_mcts_dev_search) and the ply tail of selfplay_kernels.hip.
// Everything a driver needs between calls lives in its object - no function-level statics - so that
// drivers on different engines, streams and host threads run side by side.
#include "engine_internal.h"

namespace {
template <class T>
void fetch(std::vector<T> &h, const T *dev, size_t n)
{
    h.resize(n);
    if (n) HIP_OK(hipMemcpy(h.data(), dev, n * sizeof(T), hipMemcpyDeviceToHost));
}

// the per-game figures of the finished store on the host, and the order the games are handed out in
struct FinishedGames {
    std::vector<int32_t> slot, len, win;
    std::vector<int64_t> fply, row0;
    std::vector<size_t> order;
};

// the eight tensors of an az_replay_tensors or an az_replay_batch: none null, all 16-byte aligned (w: the message's prefix)
template <class Tensors>
void require_tensors(const Tensors &t, const std::string &w)
{
    const void *q8[8] = {t.state, t.prob, t.winner, t.steps_to_end, t.aux_target, t.root_wdl, t.valid_mask, t.future_root_wdl};
    for (const void *q : q8) {
        require(q != nullptr, w + ": a null tensor");
        require(reinterpret_cast<uintptr_t>(q) % 16 == 0, w + ": a tensor is not 16-byte aligned");
    }
}

az::SpExport export_args(const az_replay_tensors *dst, int64_t ptr, int td_steps, const std::string &w)
{
    require(dst != nullptr, w + ": null tensors");
    require(dst->capacity > 0, w + ": capacity must be positive");
    require(ptr >= 0 && td_steps >= 0, w + ": ptr and td_steps must not be negative");
    require_tensors(*dst, w);
    az::SpExport a{};
    a.state = dst->state; a.prob = dst->prob; a.out_winner = dst->winner; a.steps_to_end = dst->steps_to_end;
    a.aux_target = dst->aux_target; a.root_wdl = dst->root_wdl; a.valid_mask = dst->valid_mask;
    a.future_root_wdl = dst->future_root_wdl; a.capacity = dst->capacity; a.ptr = ptr; a.td_steps = td_steps;
    return a;
}
}  // namespace

struct az_selfplay {
    az_mcts *m = nullptr;
    az_selfplay_config c;
    int B = 0, A = 0;              // B: games
    int T = 1, ens = 0;            // trees per game (tree j of game g is the engine's tree g * T + j), symmetry ensemble
    DevBuf<uint64_t> bb0, bb1;
    DevBuf<int32_t> turn, aux, ply, actions, winner, counts;      // actions, counts: per TREE
    DevBuf<int32_t> game_actions;  // teams: the move per game, in the game's frame (k_game_step reads it)
    DevBuf<uint8_t> done, dead;    // per game
    DevBuf<uint8_t> tree_done;     // teams: per tree (the trees' reset reads it)
    DevBuf<float> stats, eps;      // per tree
    DevBuf<unsigned long long> totals, alloc;      // alloc: [0] games asked for, [1] rows handed out
    // trajectories of the games in progress and the packed store of finished games
    struct Rows {
        DevBuf<uint64_t> bb0, bb1;
        DevBuf<int8_t> turn;
        DevBuf<float> prob, wdl;
        DevBuf<uint8_t> mask;
        void ensure(size_t rows, int A)
        {
            bb0.ensure(rows); bb1.ensure(rows); turn.ensure(rows); prob.ensure(rows * A); wdl.ensure(rows * 3); mask.ensure(rows * A);
        }
        az::SpRows view() { return az::SpRows{bb0.p, bb1.p, turn.p, prob.p, wdl.p, mask.p}; }
    } rec, fin;
    DevBuf<int32_t> fin_slot, fin_len, fin_winner;
    DevBuf<int64_t> fin_ply, fin_row0;
    // az_selfplay_export: the games' figures in export order, as the kernel reads them
    DevBuf<int32_t> exp_len, exp_winner;
    DevBuf<int64_t> exp_src, exp_dst;
    int64_t capacity = 0;
    int64_t driver_ply = 0;        // plies finished: the sampler's call counter
    int64_t dropped = 0;           // games dropped before the last drain
    PlyDriver drv;

    void begin_ply(hipStream_t s)
    {
        drv.require("az_selfplay");
        HIP_OK(hipSetDevice(m->device));
        if (T == 1) az::launch_set_roots(m->game, bb0.p, bb1.p, turn.p, m->roots(), B, s);
        else az::launch_match_team_roots(m->game, bb0.p, bb1.p, turn.p, T, ens, m->roots(), B, s);
    }

    void finish_ply(void *stream)
    {
        hipStream_t s = static_cast<hipStream_t>(stream);
        HIP_OK(hipSetDevice(m->device));
        drv.require("az_selfplay");
        az::launch_counts(m->game, m->arena(), counts.p, s);
        if (c.record) az::launch_root_stats(m->game, m->arena(), stats.p, s);
        az::SpPick p{};
        p.counts = counts.p; p.stats = stats.p; p.ply = ply.p; p.dead = dead.p;
        p.tape = drv.row(B);
        p.actions = actions.p; p.bb0 = bb0.p; p.bb1 = bb1.p; p.turn = turn.p; p.aux = aux.p;
        p.rec = rec.view(); p.rows_per_game = m->geo.max_plies;
        p.temperature = c.temperature; p.temp_endgame = c.temp_endgame; p.temp_decay_moves = c.temp_decay_moves;
        p.seed = m->dev_seed; p.call = static_cast<uint64_t>(driver_ply); p.n = B;
        const bool team = T > 1;
        if (team) { p.trees = T; p.ensemble = ens; p.game_actions = game_actions.p; p.tree_done = tree_done.p; }
        az::launch_sp_pick(m->game, p, c.record != 0, s);
        drv.advance();
        m->prune_on(actions.p, nullptr, true, m->replay_noise, s);
        az::launch_bump_call(m->call_ctr.p, s);
        // the end state has to survive the step (it is the last row of a recorded game): k_sp_advance refills
        az::launch_game_step(m->game, bb0.p, bb1.p, turn.p, aux.p, team ? game_actions.p : actions.p, done.p, winner.p, B, false, s);
        az::launch_reset_masked(m->arena(), team ? tree_done.p : done.p, s);
        az::SpAdvance a{};
        a.bb0 = bb0.p; a.bb1 = bb1.p; a.turn = turn.p; a.aux = aux.p; a.ply = ply.p; a.dead = dead.p;
        a.done = done.p; a.winner = winner.p; a.n = B; a.refill = c.refill; a.record = c.record;
        a.rec = rec.view(); a.fin = fin.view(); a.rows_per_game = m->geo.max_plies;
        a.fin_slot = fin_slot.p; a.fin_len = fin_len.p; a.fin_winner = fin_winner.p; a.fin_ply = fin_ply.p; a.fin_row0 = fin_row0.p;
        a.n_alloc = alloc.p; a.n_rows = alloc.p + 1; a.capacity = capacity; a.driver_ply = driver_ply;
        a.trees = T; a.eps = c.noise_steps > 0 ? eps.p : nullptr;
        a.noise_steps = c.noise_steps; a.noise_eps_init = c.noise_eps_init; a.noise_eps_min = c.noise_eps_min;
        a.totals = totals.p;
        az::launch_sp_advance(m->game, a, s);
        ++driver_ply;
        check_rc(az_mcts_dev_check(m, stream));
        drv.mark(driver_ply, s);
    }

    // games and rows in the store, games dropped so far: selects the engine's device and waits for all of it first
    void store_figures(int64_t &n_games, int64_t &n_rows, int64_t &n_dropped)
    {
        HIP_OK(hipSetDevice(m->device));
        HIP_OK(hipDeviceSynchronize());
        n_games = n_rows = 0;
        n_dropped = dropped;
        if (!c.record) return;
        unsigned long long h[2];
        HIP_OK(hipMemcpy(h, alloc.p, sizeof h, hipMemcpyDeviceToHost));
        n_games = std::min<int64_t>(static_cast<int64_t>(h[0]), capacity);
        n_rows = static_cast<int64_t>(h[1]);
        n_dropped = dropped + static_cast<int64_t>(h[0]) - n_games;
    }

    // the store's first G games: it fills in no particular order, they are handed out by (finishing ply, slot)
    FinishedGames finished_games(size_t G)
    {
        FinishedGames f;
        fetch(f.slot, fin_slot.p, G); fetch(f.len, fin_len.p, G); fetch(f.win, fin_winner.p, G);
        fetch(f.fply, fin_ply.p, G); fetch(f.row0, fin_row0.p, G);
        f.order.resize(G);
        for (size_t i = 0; i < G; ++i) f.order[i] = i;
        std::sort(f.order.begin(), f.order.end(), [&](size_t x, size_t y) {
            return f.fply[x] != f.fply[y] ? f.fply[x] < f.fply[y] : f.slot[x] < f.slot[y];
        });
        return f;
    }
};

static void create_selfplay(const char *who, az_mcts *m, const az_selfplay_config *c, const az_selfplay_teams *t, az_selfplay **out)
{
    const std::string w = std::string(who) + ": ";
    require(m != nullptr && c != nullptr && t != nullptr && out != nullptr, w + "null argument");
    require(t->trees >= 1, w + "a game needs at least one tree");
    require(m->B % t->trees == 0, w + "the engine's n_envs is no multiple of the trees per game");
    require(t->ensemble == 0 || t->trees == az::replay_num_augment(m->game),
            w + "a symmetry ensemble has one tree per symmetry of the game (az_game_num_augment)");
    HIP_OK(hipSetDevice(m->device));
    auto sp = std::make_unique<az_selfplay>();
    sp->m = m; sp->c = *c; sp->T = t->trees; sp->ens = t->ensemble != 0; sp->B = m->B / t->trees; sp->A = m->geo.actions;
    const size_t B = static_cast<size_t>(sp->B), trees = static_cast<size_t>(m->B);
    const az::GameState st = start_state(m->game);
    sp->bb0.ensure(B); sp->bb1.ensure(B); sp->turn.ensure(B);
    const std::vector<uint64_t> h0(B, st.bb0), h1(B, st.bb1);
    const std::vector<int32_t> ht(B, 1);
    HIP_OK(hipMemcpy(sp->bb0.p, h0.data(), B * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(sp->bb1.p, h1.data(), B * sizeof(uint64_t), hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(sp->turn.p, ht.data(), B * sizeof(int32_t), hipMemcpyHostToDevice));
    sp->aux.ensure(B, true); sp->ply.ensure(B, true); sp->actions.ensure(trees, true); sp->winner.ensure(B, true);
    sp->done.ensure(B, true); sp->dead.ensure(B, true);
    if (sp->T > 1) { sp->game_actions.ensure(B, true); sp->tree_done.ensure(trees, true); }
    sp->counts.ensure(trees * sp->A, true);
    sp->totals.ensure(5, true); sp->alloc.ensure(2, true);
    if (c->noise_steps > 0) {
        const std::vector<float> he(trees, static_cast<float>(c->noise_eps_min + (c->noise_eps_init - c->noise_eps_min) * 1.0));
        sp->eps.ensure(trees);
        HIP_OK(hipMemcpy(sp->eps.p, he.data(), trees * sizeof(float), hipMemcpyHostToDevice));
        m->noise_eps_tree = sp->eps.p;
    }
    if (c->record) {
        sp->stats.ensure(trees * m->geo.stats, true);
        sp->capacity = c->max_finished_games > 0 ? c->max_finished_games : std::max<int64_t>(4 * sp->B, 1024);
        sp->rec.ensure(B * m->geo.max_plies, sp->A);
        sp->fin.ensure(static_cast<size_t>(sp->capacity) * (m->geo.max_plies + 1), sp->A);
        const size_t G = static_cast<size_t>(sp->capacity);
        sp->fin_slot.ensure(G); sp->fin_len.ensure(G); sp->fin_winner.ensure(G); sp->fin_ply.ensure(G); sp->fin_row0.ensure(G);
        sp->exp_len.ensure(G); sp->exp_winner.ensure(G); sp->exp_src.ensure(G); sp->exp_dst.ensure(G);
    }
    sp->drv.create_events();
    // the games start over: so do the trees (flushed by the first search's az_mcts_dev_prepare)
    m->reset_all_trees();
    *out = sp.release();
}

extern "C" {

int az_selfplay_create(az_mcts *m, const az_selfplay_config *c, az_selfplay **out)
{
    return guarded([&] {
        const az_selfplay_teams single{1, 0};
        create_selfplay("az_selfplay_create", m, c, &single, out);
    });
}

int az_selfplay_create_teams(az_mcts *m, const az_selfplay_config *c, const az_selfplay_teams *t, az_selfplay **out)
{
    return guarded([&] { create_selfplay("az_selfplay_create_teams", m, c, t, out); });
}

void az_selfplay_destroy(az_selfplay *sp)
{
    if (!sp) return;
    (void)hipSetDevice(sp->m->device);
    (void)hipDeviceSynchronize();
    if (sp->eps.p != nullptr && sp->m->noise_eps_tree == sp->eps.p) sp->m->noise_eps_tree = nullptr;
    delete sp;
}

int az_selfplay_step(az_selfplay *sp, const az_nn_model *model, int n_playout, int K, int use_table, int n_plies, void *stream)
{
    return guarded([&] {
        require(sp != nullptr && model != nullptr && n_plies >= 0, "az_selfplay_step: bad argument");
        for (int i = 0; i < n_plies; ++i) {
            sp->begin_ply(static_cast<hipStream_t>(stream));
            check_rc(az_mcts_dev_search(sp->m, model, n_playout, K, use_table, stream));
            sp->finish_ply(stream);
        }
    });
}

int az_selfplay_begin_ply(az_selfplay *sp, void *stream)
{
    return guarded([&] {
        require(sp != nullptr, "az_selfplay_begin_ply: null driver");
        sp->begin_ply(static_cast<hipStream_t>(stream));
    });
}

int az_selfplay_finish_ply(az_selfplay *sp, void *stream)
{
    return guarded([&] {
        require(sp != nullptr, "az_selfplay_finish_ply: null driver");
        sp->finish_ply(stream);
    });
}

int az_selfplay_set_action_tape(az_selfplay *sp, const int32_t *actions, int64_t n_plies)
{
    return guarded([&] {
        require(sp != nullptr && (actions == nullptr || n_plies > 0), "az_selfplay_set_action_tape: a tape needs a length");
        sp->drv.set(actions, n_plies);
    });
}

int az_selfplay_totals(az_selfplay *sp, int64_t out[5])
{
    return guarded([&] {
        require(sp != nullptr && out != nullptr, "az_selfplay_totals: null argument");
        HIP_OK(hipSetDevice(sp->m->device));
        HIP_OK(hipDeviceSynchronize());
        unsigned long long h[5];
        HIP_OK(hipMemcpy(h, sp->totals.p, sizeof h, hipMemcpyDeviceToHost));
        for (int i = 0; i < 5; ++i) out[i] = static_cast<int64_t>(h[i]);
    });
}

int az_selfplay_positions(az_selfplay *sp, uint64_t *bb_p1, uint64_t *bb_p2, int32_t *turns, int32_t *ply)
{
    return guarded([&] {
        require(sp != nullptr, "az_selfplay_positions: null driver");
        HIP_OK(hipSetDevice(sp->m->device));
        HIP_OK(hipDeviceSynchronize());
        const size_t B = static_cast<size_t>(sp->B);
        if (bb_p1) HIP_OK(hipMemcpy(bb_p1, sp->bb0.p, B * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (bb_p2) HIP_OK(hipMemcpy(bb_p2, sp->bb1.p, B * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (turns) HIP_OK(hipMemcpy(turns, sp->turn.p, B * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (ply) HIP_OK(hipMemcpy(ply, sp->ply.p, B * sizeof(int32_t), hipMemcpyDeviceToHost));
    });
}

int az_selfplay_finished(az_selfplay *sp, int64_t *n_games, int64_t *n_rows, int64_t *n_dropped)
{
    return guarded([&] {
        require(sp != nullptr, "az_selfplay_finished: null driver");
        int64_t g, r, d;
        sp->store_figures(g, r, d);
        if (n_games) *n_games = g;
        if (n_rows) *n_rows = r;
        if (n_dropped) *n_dropped = d;
    });
}

int az_selfplay_drain(az_selfplay *sp, const az_selfplay_games *out, int64_t n_games, int64_t n_rows)
{
    return guarded([&] {
        require(sp != nullptr && out != nullptr, "az_selfplay_drain: null argument");
        require(sp->c.record != 0, "az_selfplay_drain: the driver does not record");
        int64_t g, r, d;
        sp->store_figures(g, r, d);
        require(g == n_games && r == n_rows, "az_selfplay_drain: sizes differ from what az_selfplay_finished reports");
        const size_t G = static_cast<size_t>(g), R = static_cast<size_t>(r), A = static_cast<size_t>(sp->A);
        const FinishedGames f = sp->finished_games(G);
        std::vector<uint64_t> b0, b1;
        std::vector<int8_t> tn;
        std::vector<float> pr, wd;
        std::vector<uint8_t> mk;
        fetch(b0, sp->fin.bb0.p, R); fetch(b1, sp->fin.bb1.p, R); fetch(tn, sp->fin.turn.p, R);
        fetch(pr, sp->fin.prob.p, R * A); fetch(wd, sp->fin.wdl.p, R * 3); fetch(mk, sp->fin.mask.p, R * A);
        size_t at = 0;
        for (size_t k = 0; k < G; ++k) {
            const size_t i = f.order[k], rows = static_cast<size_t>(f.len[i]) + 1, from = static_cast<size_t>(f.row0[i]);
            if (from + rows > R || at + rows > R) throw AzError(AZ_ERR_STATE, "az_selfplay_drain: the finished store is inconsistent");
            out->slot[k] = f.slot[i]; out->length[k] = f.len[i]; out->winner[k] = f.win[i];
            out->finish_ply[k] = f.fply[i]; out->row_start[k] = static_cast<int64_t>(at);
            std::copy_n(&b0[from], rows, out->bb_p1 + at); std::copy_n(&b1[from], rows, out->bb_p2 + at);
            std::copy_n(&tn[from], rows, out->turn + at);
            std::copy_n(&pr[from * A], rows * A, out->prob + at * A); std::copy_n(&wd[from * 3], rows * 3, out->wdl + at * 3);
            std::copy_n(&mk[from * A], rows * A, out->mask + at * A);
            at += rows;
        }
        sp->dropped = d;
        HIP_OK(hipMemset(sp->alloc.p, 0, 2 * sizeof(unsigned long long)));
    });
}

int az_selfplay_export(az_selfplay *sp, const az_replay_tensors *dst, int64_t ptr, int td_steps, int64_t n_games,
                       int64_t n_rows, const az_selfplay_export_info *info, int64_t *new_ptr, void *stream)
{
    return guarded([&] {
        require(sp != nullptr, "az_selfplay_export: null driver");
        require(sp->c.record != 0, "az_selfplay_export: the driver does not record");
        az::SpExport a = export_args(dst, ptr, td_steps, "az_selfplay_export");
        hipStream_t s = static_cast<hipStream_t>(stream);
        int64_t g, r, d;
        sp->store_figures(g, r, d);
        require(g == n_games && r == n_rows, "az_selfplay_export: sizes differ from what az_selfplay_finished reports");
        const size_t G = static_cast<size_t>(g);
        // per-game figures only: the rows stay where they are
        const FinishedGames f = sp->finished_games(G);
        std::vector<int32_t> e_len(G), e_win(G);
        std::vector<int64_t> e_src(G), e_dst(G);
        int64_t at = 0;
        for (size_t k = 0; k < G; ++k) {
            const size_t i = f.order[k];
            const int64_t rows = static_cast<int64_t>(f.len[i]) + 1;
            if (f.len[i] < 0 || f.row0[i] < 0 || f.row0[i] + rows > r || at + rows > r)
                throw AzError(AZ_ERR_STATE, "az_selfplay_export: the finished store is inconsistent");
            e_len[k] = f.len[i]; e_win[k] = f.win[i]; e_src[k] = f.row0[i]; e_dst[k] = at;
            if (info != nullptr) {
                if (info->slot) info->slot[k] = f.slot[i];
                if (info->length) info->length[k] = f.len[i];
                if (info->winner) info->winner[k] = f.win[i];
                if (info->finish_ply) info->finish_ply[k] = f.fply[i];
            }
            at += rows;
        }
        if (at != r) throw AzError(AZ_ERR_STATE, "az_selfplay_export: the finished store is inconsistent");
        if (G) {
            // the device is idle (waited for above): plain copies, nothing of the driver's reads these buffers now
            HIP_OK(hipMemcpy(sp->exp_len.p, e_len.data(), G * sizeof(int32_t), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(sp->exp_winner.p, e_win.data(), G * sizeof(int32_t), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(sp->exp_src.p, e_src.data(), G * sizeof(int64_t), hipMemcpyHostToDevice));
            HIP_OK(hipMemcpy(sp->exp_dst.p, e_dst.data(), G * sizeof(int64_t), hipMemcpyHostToDevice));
            a.fin = sp->fin.view();
            a.len = sp->exp_len.p; a.winner = sp->exp_winner.p; a.src_row0 = sp->exp_src.p; a.dst_row0 = sp->exp_dst.p;
            a.n_games = g;
            az::launch_sp_export(sp->m->game, a, s);
        }
        // the store empties BEHIND the kernel on the caller's stream: the next ply's k_sp_advance, enqueued after
        // this call on that stream, hands out rows from 0 again only once the kernel has read them
        HIP_OK(hipMemsetAsync(sp->alloc.p, 0, 2 * sizeof(unsigned long long), s));
        sp->dropped = d;
        if (new_ptr) *new_ptr = ptr + r;
    });
}

int az_replay_dev_store(int game, const az_selfplay_games *games_dev, const int64_t *src_row0, const int64_t *dst_row0,
                        int64_t n_games, const az_replay_tensors *dst, int64_t ptr, int td_steps, void *stream)
{
    return guarded([&] {
        require(known_game(game), "az_replay_dev_store: unknown game");
        require(games_dev != nullptr && src_row0 != nullptr && dst_row0 != nullptr && n_games >= 0, "az_replay_dev_store: bad argument");
        require(games_dev->length && games_dev->winner && games_dev->bb_p1 && games_dev->bb_p2 && games_dev->turn &&
                games_dev->prob && games_dev->wdl && games_dev->mask, "az_replay_dev_store: a null array");
        az::SpExport a = export_args(dst, ptr, td_steps, "az_replay_dev_store");
        a.fin = az::SpRows{games_dev->bb_p1, games_dev->bb_p2, games_dev->turn, games_dev->prob, games_dev->wdl, games_dev->mask};
        a.len = games_dev->length; a.winner = games_dev->winner; a.src_row0 = src_row0; a.dst_row0 = dst_row0;
        a.n_games = n_games;
        az::launch_sp_export(game, a, static_cast<hipStream_t>(stream));
    });
}

int az_game_num_augment(int game) { return known_game(game) ? az::replay_num_augment(game) : -1; }

int az_replay_dev_batch(int game, const az_replay_tensors *src, const int64_t *idx, const int64_t *order, int64_t first,
                        int64_t B, const az_replay_batch *out, void *stream)
{
    return guarded([&] {
        const std::string w("az_replay_dev_batch");
        require(known_game(game), w + ": unknown game");
        require(src != nullptr && out != nullptr && idx != nullptr, w + ": null argument");
        require(B > 0 && B <= (int64_t(1) << 30), w + ": B must be positive (and at most 2^30)");
        require(first >= 0, w + ": first must not be negative");
        require(src->capacity > 0, w + ": capacity must be positive");
        require_tensors(*src, w);
        require_tensors(*out, w);
        az::ReplayBatch a{};
        a.state = src->state; a.prob = src->prob; a.winner = src->winner; a.steps_to_end = src->steps_to_end;
        a.aux_target = src->aux_target; a.root_wdl = src->root_wdl; a.future_root_wdl = src->future_root_wdl;
        a.valid_mask = src->valid_mask; a.capacity = src->capacity;
        a.idx = idx; a.order = order; a.first = first; a.B = B;
        a.o_state = out->state; a.o_prob = out->prob; a.o_winner = out->winner; a.o_steps_to_end = out->steps_to_end;
        a.o_aux_target = out->aux_target; a.o_root_wdl = out->root_wdl; a.o_future_root_wdl = out->future_root_wdl;
        a.o_valid_mask = out->valid_mask;
        az::launch_replay_batch(game, a, static_cast<hipStream_t>(stream));
    });
}

int az_replay_dev_sample_indices(uint64_t seed, uint64_t call, int64_t n_valid, int64_t *idx, int64_t n, void *stream)
{
    return guarded([&] {
        require(n_valid > 0, "az_replay_dev_sample_indices: n_valid must be positive");
        require(n >= 0, "az_replay_dev_sample_indices: n must not be negative");
        require(idx != nullptr || n == 0, "az_replay_dev_sample_indices: null idx");
        az::launch_replay_indices(seed, call, n_valid, idx, n, static_cast<hipStream_t>(stream));
    });
}

int az_selfplay_sample(int game, const int32_t *counts, const int32_t *ply, const az_selfplay_config *c, uint64_t seed,
                       uint64_t call, int32_t *actions, int64_t n, void *stream)
{
    return guarded([&] {
        require(known_game(game), "az_selfplay_sample: unknown game");
        require(counts != nullptr && ply != nullptr && c != nullptr && actions != nullptr && n >= 0, "az_selfplay_sample: bad argument");
        az::SpPick p{};
        p.counts = counts; p.ply = ply; p.actions = actions;
        p.temperature = c->temperature; p.temp_endgame = c->temp_endgame; p.temp_decay_moves = c->temp_decay_moves;
        p.seed = seed; p.call = call; p.n = n;
        az::launch_sp_pick(game, p, false, static_cast<hipStream_t>(stream));
    });
}

int az_selfplay_team_sample(int game, const int32_t *counts, const int32_t *ply, const az_selfplay_config *c, int trees, int ensemble,
                            uint64_t seed, uint64_t call, int32_t *summed, int32_t *actions, int32_t *tree_actions, int64_t n, void *stream)
{
    return guarded([&] {
        require(known_game(game), "az_selfplay_team_sample: unknown game");
        require(counts != nullptr && ply != nullptr && c != nullptr && actions != nullptr && n >= 0 && trees >= 1,
                "az_selfplay_team_sample: bad argument");
        require(ensemble == 0 || trees == az::replay_num_augment(game), "az_selfplay_team_sample: an ensemble has one tree per symmetry");
        az::SpPick p{};
        p.counts = counts; p.ply = ply; p.actions = tree_actions; p.game_actions = actions; p.summed = summed;
        p.trees = trees; p.ensemble = ensemble != 0;
        p.temperature = c->temperature; p.temp_endgame = c->temp_endgame; p.temp_decay_moves = c->temp_decay_moves;
        p.seed = seed; p.call = call; p.n = n;
        az::launch_sp_pick(game, p, false, static_cast<hipStream_t>(stream));
    });
}

int az_mcts_dev_team_root_stats(int game, const float *stats, int trees, int ensemble, float *merged, int64_t n, void *stream)
{
    return guarded([&] {
        require(known_game(game), "az_mcts_dev_team_root_stats: unknown game");
        require(stats != nullptr && merged != nullptr && n >= 0 && trees >= 1, "az_mcts_dev_team_root_stats: bad argument");
        require(ensemble == 0 || trees == az::replay_num_augment(game), "az_mcts_dev_team_root_stats: an ensemble has one tree per symmetry");
        az::launch_team_root_stats(game, stats, trees, ensemble != 0, merged, n, static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
