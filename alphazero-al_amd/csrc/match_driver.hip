// match_driver.hip - the evaluation-match driver (az_match_*).
// Two engines, two models, one set of games (pipeline.py:264-335): the side to move searches in its own engine, the
// tail of the ply is k_match_ply (match_kernels.hip), then BOTH engines re-root with the move and reset the trees of
// the games that ended.  Same conventions as the self-play driver (selfplay_driver.hip): everything between calls
// lives in the object.  A player may bring a team of trees per game (root-parallel play, the symmetry ensemble;
// player.py:248-329): engine e then holds B * T[e] trees, tree j of game g is its tree g * T[e] + j.
#include "engine_internal.h"

struct az_match {
    az_mcts *e[2] = {nullptr, nullptr};     // [0] the trees of player +1, [1] of player -1
    az_match_config c;
    int B = 0;                              // games
    int T[2] = {1, 1};                      // trees per game of each player
    int ens[2] = {0, 0};                    // that player's trees are the game's symmetry ensemble
    DevBuf<uint64_t> bb0, bb1;
    DevBuf<int32_t> turn, aux, length, winner, counts, moves;
    DevBuf<int32_t> actions[2];             // per engine and tree: the move in the tree's frame
    DevBuf<uint8_t> done[2], dead;          // done: per engine and tree
    DevBuf<uint8_t> ones;                   // a reset mask that names every tree of either engine (fresh-tree players)
    DevBuf<unsigned long long> totals;      // won by +1, won by -1, drawn, finished
    unsigned long long *fin_host = nullptr; // pinned: `finished` as of the newest ply that has completed
    int64_t ply = 0;                        // plies finished: the sampler's call counter and the move record's row
    int mover = 1;                          // side to move of every game that is still running
    bool ply_open = false;                  // begin_ply has put roots into the mover's engine
    PlyDriver drv;

    ~az_match() { if (fin_host) (void)hipHostFree(fin_host); }

    az_mcts *mover_engine() const { return e[mover > 0 ? 0 : 1]; }

    // nothing left to play: every game is over (as far as the host has been told) or the game's ply bound is reached
    bool finished() const { return ply >= e[0]->geo.max_plies || *static_cast<volatile unsigned long long *>(fin_host) >= static_cast<unsigned long long>(B); }

    // false: the match is over and the ply is not played
    bool begin_ply(hipStream_t s)
    {
        if (finished()) { ply_open = false; return false; }
        drv.require("az_match");
        az_mcts *m = mover_engine();
        HIP_OK(hipSetDevice(m->device));
        const int side = mover > 0 ? 0 : 1;
        if (T[side] == 1 && !ens[side]) az::launch_set_roots(m->game, bb0.p, bb1.p, turn.p, m->roots(), B, s);
        else az::launch_match_team_roots(m->game, bb0.p, bb1.p, turn.p, T[side], ens[side], m->roots(), B, s);
        ply_open = true;
        return true;
    }

    // The mover's trees start this search empty (game.py:41 resets both players after every move).  Enqueued; the
    // host-side occupancy bound starts over with the trees, or it would add a search's worth per ply and grow arenas
    // that never hold more than one search.
    void reset_mover_trees(hipStream_t s)
    {
        az_mcts *m = mover_engine();
        az::launch_reset_masked(m->arena(), ones.p, s);
        m->used_bound = 1;
    }

    void finish_ply(void *stream)
    {
        if (!ply_open) return;
        hipStream_t s = static_cast<hipStream_t>(stream);
        az_mcts *m = mover_engine();
        HIP_OK(hipSetDevice(m->device));
        drv.require("az_match");
        ply_open = false;
        az::launch_counts(m->game, m->arena(), counts.p, s);
        az::MatchPly p{};
        const int side = mover > 0 ? 0 : 1;
        p.counts = counts.p; p.trees = T[side]; p.ensemble = ens[side];
        p.tape = drv.row(B);
        p.bb0 = bb0.p; p.bb1 = bb1.p; p.turn = turn.p; p.aux = aux.p; p.length = length.p; p.dead = dead.p;
        for (int i = 0; i < 2; ++i) p.team[i] = az::MatchTeam{actions[i].p, done[i].p, T[i], ens[i]};
        p.winner = winner.p;
        p.moves = c.record_moves ? moves.p : nullptr;
        p.totals = totals.p; p.temperature = c.temperature;
        p.seed = e[0]->dev_seed; p.ply = static_cast<uint64_t>(ply); p.n = B;
        az::launch_match_ply(m->game, p, s);
        drv.advance();
        for (int i = 0; i < 2; ++i) {
            e[i]->prune_on(actions[i].p, nullptr, true, e[i]->replay_noise, s);
            az::launch_bump_call(e[i]->call_ctr.p, s);
        }
        for (int i = 0; i < 2; ++i) az::launch_reset_masked(e[i]->arena(), done[i].p, s);
        HIP_OK(hipMemcpyAsync(fin_host, totals.p + 3, sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        ++ply;
        mover = -mover;
        for (az_mcts *x : e) check_rc(az_mcts_dev_check(x, stream));
        drv.mark(ply, s);
    }

    // positions (HOST arrays, one side to move) into the match; games that are already over are finished at ply 0
    void load(const uint64_t *h0, const uint64_t *h1, int side)
    {
        const size_t n = static_cast<size_t>(B);
        const int game = e[0]->game;
        std::vector<int32_t> ht(n, side), ha(n), hw(n, 0);
        std::vector<uint8_t> hd(n, 0);
        unsigned long long tot[4] = {0, 0, 0, 0};
        for (size_t i = 0; i < n; ++i) {
            az::GameState st;
            st.bb0 = h0[i]; st.bb1 = h1[i]; st.turn = side;
            st.aux = game == AZ_GAME_CONNECT4 ? az::Connect4Dev::root_aux(h0[i], h1[i]) : az::OthelloDev::root_aux(h0[i], h1[i]);
            ha[i] = st.aux;
            const int res = game == AZ_GAME_CONNECT4 ? az::Connect4Dev::result(st) : az::OthelloDev::result(st);
            if (res >= 0) {
                hd[i] = 1; hw[i] = res == 1 ? 1 : (res == 2 ? -1 : 0);
                ++tot[res == 1 ? 0 : (res == 2 ? 1 : 2)]; ++tot[3];
            }
        }
        HIP_OK(hipSetDevice(e[0]->device));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(bb0.p, h0, n * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(bb1.p, h1, n * sizeof(uint64_t), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(turn.p, ht.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(aux.p, ha.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(winner.p, hw.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(dead.p, hd.data(), n, hipMemcpyHostToDevice));
        HIP_OK(hipMemset(length.p, 0, n * sizeof(int32_t)));
        HIP_OK(hipMemcpy(totals.p, tot, sizeof tot, hipMemcpyHostToDevice));
        *fin_host = tot[3];
        mover = side;
        // the games start over: so do both engines' trees - now, the engine that waits is re-rooted before its first search
        for (az_mcts *x : e) {
            x->reset_all_trees();
            x->flush_resets(nullptr);
        }
        HIP_OK(hipDeviceSynchronize());
    }
};

static void create_match(const char *who, az_mcts *engine_p1, az_mcts *engine_p2, const az_match_config *c, const az_match_teams *t,
                         az_match **out)
{
    const std::string w = std::string(who) + ": ";
    require(engine_p1 != nullptr && engine_p2 != nullptr && c != nullptr && t != nullptr && out != nullptr, w + "null argument");
    require(engine_p1 != engine_p2, w + "the two players need an engine each");
    require(engine_p1->game == engine_p2->game, w + "the engines play different games");
    require(engine_p1->device == engine_p2->device, w + "the engines are on different devices");
    require(t->trees_p1 >= 1 && t->trees_p2 >= 1, w + "a player needs at least one tree per game");
    require(engine_p1->B % t->trees_p1 == 0 && engine_p2->B % t->trees_p2 == 0, w + "an engine's n_envs is no multiple of its trees per game");
    require(engine_p1->B / t->trees_p1 == engine_p2->B / t->trees_p2, w + "the engines differ in n_envs (games)");
    const int n_sym = az::replay_num_augment(engine_p1->game);
    require((t->ensemble_p1 == 0 || t->trees_p1 == n_sym) && (t->ensemble_p2 == 0 || t->trees_p2 == n_sym),
            w + "a symmetry ensemble has one tree per symmetry of the game (az_game_num_augment)");
    HIP_OK(hipSetDevice(engine_p1->device));
    auto mt = std::make_unique<az_match>();
    mt->e[0] = engine_p1; mt->e[1] = engine_p2; mt->c = *c;
    mt->T[0] = t->trees_p1; mt->T[1] = t->trees_p2;
    mt->ens[0] = t->ensemble_p1 != 0; mt->ens[1] = t->ensemble_p2 != 0;
    mt->B = engine_p1->B / t->trees_p1;
    const size_t B = static_cast<size_t>(mt->B);
    const size_t trees = static_cast<size_t>(std::max(engine_p1->B, engine_p2->B));
    mt->bb0.ensure(B); mt->bb1.ensure(B); mt->turn.ensure(B); mt->aux.ensure(B); mt->length.ensure(B);
    mt->winner.ensure(B); mt->dead.ensure(B);
    for (int i = 0; i < 2; ++i) {
        mt->actions[i].ensure(static_cast<size_t>(mt->e[i]->B), true);
        mt->done[i].ensure(static_cast<size_t>(mt->e[i]->B), true);
    }
    mt->counts.ensure(trees * engine_p1->geo.actions, true);
    mt->ones.ensure(trees);
    HIP_OK(hipMemset(mt->ones.p, 1, trees));
    mt->totals.ensure(4);
    if (c->record_moves) {
        mt->moves.ensure(B * engine_p1->geo.max_plies);
        HIP_OK(hipMemset(mt->moves.p, 0xFF, B * engine_p1->geo.max_plies * sizeof(int32_t)));      // -1: nothing played
    }
    HIP_OK(hipHostMalloc(reinterpret_cast<void **>(&mt->fin_host), sizeof(unsigned long long), hipHostMallocDefault));
    mt->drv.create_events();
    const az::GameState st = start_state(engine_p1->game);
    const std::vector<uint64_t> h0(B, st.bb0), h1(B, st.bb1);
    mt->load(h0.data(), h1.data(), 1);
    *out = mt.release();
}

extern "C" {

int az_match_create(az_mcts *engine_p1, az_mcts *engine_p2, const az_match_config *c, az_match **out)
{
    return guarded([&] {
        const az_match_teams single{1, 1, 0, 0};
        create_match("az_match_create", engine_p1, engine_p2, c, &single, out);
    });
}

int az_match_create_teams(az_mcts *engine_p1, az_mcts *engine_p2, const az_match_config *c, const az_match_teams *t, az_match **out)
{
    return guarded([&] { create_match("az_match_create_teams", engine_p1, engine_p2, c, t, out); });
}

void az_match_destroy(az_match *mt)
{
    if (!mt) return;
    (void)hipSetDevice(mt->e[0]->device);
    (void)hipDeviceSynchronize();
    delete mt;
}

int az_match_set_positions(az_match *mt, const uint64_t *bb_p1, const uint64_t *bb_p2, const int32_t *turns)
{
    return guarded([&] {
        require(mt != nullptr && bb_p1 != nullptr && bb_p2 != nullptr && turns != nullptr, "az_match_set_positions: null argument");
        require(mt->ply == 0 && !mt->ply_open, "az_match_set_positions: the match has begun");
        for (int i = 0; i < mt->B; ++i) {
            require(turns[i] == 1 || turns[i] == -1, "az_match_set_positions: a side to move is +1 or -1");
            require(turns[i] == turns[0], "az_match_set_positions: every game needs the same side to move");
            require((bb_p1[i] & bb_p2[i]) == 0, "az_match_set_positions: a cell holds two stones");
        }
        mt->load(bb_p1, bb_p2, turns[0]);
    });
}

int az_match_step(az_match *mt, const az_nn_model *model_p1, const az_nn_model *model_p2, int n_playout, int K, int use_table,
                  int n_plies, void *stream)
{
    return guarded([&] {
        require(mt != nullptr && model_p1 != nullptr && model_p2 != nullptr && n_plies >= 0, "az_match_step: bad argument");
        for (int i = 0; i < n_plies; ++i) {
            if (!mt->begin_ply(static_cast<hipStream_t>(stream))) return;
            check_rc(az_mcts_dev_search(mt->mover_engine(), mt->mover > 0 ? model_p1 : model_p2, n_playout, K, use_table, stream));
            mt->finish_ply(stream);
        }
    });
}

int az_match_step_players(az_match *mt, const az_nn_model *model_p1, const az_nn_model *model_p2, int n_playout_p1, int n_playout_p2,
                          int K, int use_table, int fresh_trees, int n_plies, void *stream)
{
    return guarded([&] {
        require(mt != nullptr && n_plies >= 0 && n_playout_p1 >= 0 && n_playout_p2 >= 0, "az_match_step_players: bad argument");
        for (int i = 0; i < n_plies; ++i) {
            if (!mt->begin_ply(static_cast<hipStream_t>(stream))) return;
            const int side = mt->mover > 0 ? 0 : 1;
            const az_nn_model *model = side == 0 ? model_p1 : model_p2;
            const int n_playout = side == 0 ? n_playout_p1 : n_playout_p2;
            if ((fresh_trees >> side) & 1) mt->reset_mover_trees(static_cast<hipStream_t>(stream));
            if (model != nullptr) check_rc(az_mcts_dev_search(mt->mover_engine(), model, n_playout, K, use_table, stream));
            else check_rc(az_mcts_dev_rollout_search(mt->mover_engine(), n_playout, 0, stream));
            mt->finish_ply(stream);
        }
    });
}

int az_match_begin_ply(az_match *mt, void *stream, int *mover)
{
    return guarded([&] {
        require(mt != nullptr && mover != nullptr, "az_match_begin_ply: null argument");
        require(!mt->ply_open, "az_match_begin_ply: the previous ply is not finished");
        *mover = mt->begin_ply(static_cast<hipStream_t>(stream)) ? mt->mover : 0;
    });
}

int az_match_finish_ply(az_match *mt, void *stream)
{
    return guarded([&] {
        require(mt != nullptr, "az_match_finish_ply: null match");
        mt->finish_ply(stream);
    });
}

int az_match_set_action_tape(az_match *mt, const int32_t *actions, int64_t n_plies)
{
    return guarded([&] {
        require(mt != nullptr && (actions == nullptr || n_plies > 0), "az_match_set_action_tape: a tape needs a length");
        mt->drv.set(actions, n_plies);
    });
}

int az_match_remaining(az_match *mt, int64_t *n)
{
    return guarded([&] {
        require(mt != nullptr && n != nullptr, "az_match_remaining: null argument");
        HIP_OK(hipSetDevice(mt->e[0]->device));
        HIP_OK(hipDeviceSynchronize());
        unsigned long long h[4];
        HIP_OK(hipMemcpy(h, mt->totals.p, sizeof h, hipMemcpyDeviceToHost));
        *mt->fin_host = h[3];
        *n = mt->B - static_cast<int64_t>(h[3]);
    });
}

int az_match_results(az_match *mt, int32_t *winner, int32_t *length, int64_t totals[4])
{
    return guarded([&] {
        require(mt != nullptr, "az_match_results: null match");
        HIP_OK(hipSetDevice(mt->e[0]->device));
        HIP_OK(hipDeviceSynchronize());
        const size_t B = static_cast<size_t>(mt->B);
        if (winner) HIP_OK(hipMemcpy(winner, mt->winner.p, B * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (length) HIP_OK(hipMemcpy(length, mt->length.p, B * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (totals) {
            unsigned long long h[4];
            HIP_OK(hipMemcpy(h, mt->totals.p, sizeof h, hipMemcpyDeviceToHost));
            for (int i = 0; i < 3; ++i) totals[i] = static_cast<int64_t>(h[i]);
            totals[3] = mt->B - static_cast<int64_t>(h[3]);
        }
    });
}

int az_match_moves(az_match *mt, int32_t *actions)
{
    return guarded([&] {
        require(mt != nullptr && actions != nullptr, "az_match_moves: null argument");
        require(mt->c.record_moves != 0, "az_match_moves: the match does not record its moves");
        HIP_OK(hipSetDevice(mt->e[0]->device));
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemcpy(actions, mt->moves.p, static_cast<size_t>(mt->B) * mt->e[0]->geo.max_plies * sizeof(int32_t), hipMemcpyDeviceToHost));
    });
}

int az_match_max_plies(const az_match *mt) { return mt ? mt->e[0]->geo.max_plies : -1; }

int az_match_sample(int game, const int32_t *counts, float temperature, uint64_t seed, uint64_t ply, int32_t *actions, int64_t n,
                    void *stream)
{
    return guarded([&] {
        require(known_game(game), "az_match_sample: unknown game");
        require(counts != nullptr && actions != nullptr && n >= 0, "az_match_sample: bad argument");
        az::launch_match_sample(game, counts, temperature, seed, ply, actions, n, static_cast<hipStream_t>(stream));
    });
}

int az_match_team_roots(int game, const uint64_t *bb_p1, const uint64_t *bb_p2, const int32_t *turns, int trees, int ensemble,
                        uint64_t *out_bb_p1, uint64_t *out_bb_p2, int32_t *out_turns, int64_t n, void *stream)
{
    return guarded([&] {
        require(known_game(game), "az_match_team_roots: unknown game");
        require(bb_p1 != nullptr && bb_p2 != nullptr && turns != nullptr && out_bb_p1 != nullptr && out_bb_p2 != nullptr &&
                out_turns != nullptr && n >= 0 && trees >= 1, "az_match_team_roots: bad argument");
        require(ensemble == 0 || trees == az::replay_num_augment(game), "az_match_team_roots: an ensemble has one tree per symmetry");
        az::RootState rs{out_bb_p1, out_bb_p2, out_turns, nullptr};
        az::launch_match_team_roots(game, bb_p1, bb_p2, turns, trees, ensemble != 0, rs, n, static_cast<hipStream_t>(stream));
    });
}

int az_match_team_sample(int game, const int32_t *counts, int trees, int ensemble, float temperature, uint64_t seed, uint64_t ply,
                         int32_t *summed, int32_t *actions, int out_trees, int out_ensemble, int32_t *tree_actions, int64_t n,
                         void *stream)
{
    return guarded([&] {
        require(known_game(game), "az_match_team_sample: unknown game");
        require(counts != nullptr && actions != nullptr && n >= 0 && trees >= 1, "az_match_team_sample: bad argument");
        const int n_sym = az::replay_num_augment(game);
        require(ensemble == 0 || trees == n_sym, "az_match_team_sample: an ensemble has one tree per symmetry");
        require(tree_actions == nullptr || (out_trees >= 1 && (out_ensemble == 0 || out_trees == n_sym)),
                "az_match_team_sample: bad output team");
        az::launch_match_team_sample(game, counts, trees, ensemble != 0, temperature, seed, ply, summed, actions, out_trees,
                                     out_ensemble != 0, tree_actions, n, static_cast<hipStream_t>(stream));
    });
}

}  // extern "C"
