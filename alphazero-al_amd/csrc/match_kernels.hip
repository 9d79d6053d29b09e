// match_kernels.hip - the ply tail of the evaluation-match driver (az_match_* in az_mcts.h), instantiated per game
// like the tree kernels.
//
//   k_match_ply   the whole tail of a ply in ONE launch: the mover engine's root visit counts -> the move
//                 (pipeline.py:337-351, the pick of sp_pick.h that k_sp_pick uses), the action both engines' re-rooting
//                 reads, the stepped position (games.h), `done` for both engines' resets, winner, length, the dead
//                 flag, the move record and the totals.  The self-play tail is three launches because a finished
//                 slot is refilled: the tree reset needs `done` BEFORE the refill rewrites the slot, and the end state
//                 has to survive for the recorded game's last row.  A match never refills and keeps no rows, so
//                 nothing orders the step against anything else of the ply.
//                 One lane group per game as in kernels.hip (Connect4: 8 lanes, 8 games per wavefront; Othello: a
//                 wavefront): lane e owns action e of the count row, Othello's pass rides with lane 0.  Every lane of
//                 a group steps its game's position in registers (the pick leaves the move in all of them), lane 0 of
//                 the group stores.  No LDS, no barrier.
//                 Teams (player.py:248-329): the mover's `trees` count rows of a game are one row in registers before
//                 the pick - lane e adds up its action's count over the rows, in an ensemble through each tree's
//                 symmetry (team.h, shared with k_sp_pick's team form; plain loads, no cross-lane traffic) - and after the step the group's lanes
//                 write the move, in each tree's own frame, and `done` for every tree of BOTH engines' teams.
//   k_match_sample  the pick alone, for tests (az_match_sample); k_match_team_sample its team form.
//   k_match_team_roots  the games' positions -> the roots of the mover's team, one thread per tree (an ensemble's tree
//                 j sees the position under symmetry j).  A match of single trees uses k_set_roots as before.
//
// Totals: one ballot per figure and wavefront, one atomic per figure per wavefront that has something to add.
#include "kernels.h"

#include "board_sym.h"
#include "dev_rng.h"
#include "games.h"
#include "sp_pick.h"
#include "team.h"

namespace az {
namespace {

constexpr int WAVE = 64;

template <class G>
__global__ void __launch_bounds__(WAVE) k_match_ply(MatchPly a)
{
    constexpr int L = G::LANES, A = G::ACTIONS;
    const int lane = threadIdx.x, sub = lane % L;
    const int64_t game = static_cast<int64_t>(blockIdx.x) * (WAVE / L) + lane / L;
    const bool live = game < a.n;                      // the last wavefront may hold fewer games than groups
    const int64_t g = live ? game : 0;                 // idle groups read game 0 and store nothing
    const bool dead = a.dead[g] != 0;

    int c0, c1;
    team_counts<G>(a.counts, g, a.trees, a.ensemble, live, sub, c0, c1);
    PickLane pl;
    int action = pick_move_counts<G, MATCH_STREAM>(c0, c1, live, lane, a.temperature, a.tape, a.seed, a.ply, g, pl);
    if (dead || action < 0 || action >= A) action = -1;    // a tape's -1: the game does not move

    GameState s;
    s.bb0 = a.bb0[g]; s.bb1 = a.bb1[g]; s.turn = a.turn[g]; s.aux = a.aux[g];
    int res = -1;
    if (action >= 0) {
        G::step(s, action);
        res = G::result(s);
    }
    const bool fin = live && res >= 0;
    const int win = res == 1 ? 1 : (res == 2 ? -1 : 0);
    if (live) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const MatchTeam &t = a.team[e];
            store_team_actions<G>(t.actions, g, t.trees, t.ensemble, sub, action);
            for (int j = sub; j < t.trees; j += L) t.done[g * t.trees + j] = fin ? 1 : 0;
        }
    }
    if (live && sub == 0) {
        if (a.moves != nullptr) a.moves[a.ply * static_cast<uint64_t>(a.n) + g] = action;
        if (action >= 0) {
            a.bb0[g] = s.bb0; a.bb1[g] = s.bb1; a.turn[g] = s.turn; a.aux[g] = s.aux;
            a.length[g] += 1;
        }
        if (fin) { a.winner[g] = win; a.dead[g] = 1; }
    }
    // one vote per game: lane 0 of its group
    const bool vote = fin && sub == 0;
    const unsigned long long w1 = __ballot(vote && win == 1), w2 = __ballot(vote && win == -1), w0 = __ballot(vote && win == 0);
    if (lane == 0) {
        if (w1) atomicAdd(&a.totals[0], static_cast<unsigned long long>(__popcll(w1)));
        if (w2) atomicAdd(&a.totals[1], static_cast<unsigned long long>(__popcll(w2)));
        if (w0) atomicAdd(&a.totals[2], static_cast<unsigned long long>(__popcll(w0)));
        if (w1 | w2 | w0) atomicAdd(&a.totals[3], static_cast<unsigned long long>(__popcll(w1 | w2 | w0)));
    }
}

template <class G>
__global__ void __launch_bounds__(WAVE) k_match_sample(const int32_t *counts, float temperature, uint64_t seed, uint64_t ply,
                                                       int32_t *actions, int64_t n)
{
    constexpr int L = G::LANES, A = G::ACTIONS;
    const int lane = threadIdx.x;
    const int64_t game = static_cast<int64_t>(blockIdx.x) * (WAVE / L) + lane / L;
    const bool live = game < n;
    const int64_t g = live ? game : 0;
    PickLane pl;
    const int action = pick_move<G, MATCH_STREAM>(counts + g * A, live, lane, temperature, nullptr, seed, ply, g, pl);
    if (live && lane % L == 0) actions[g] = action;
}

template <class G>
__global__ void __launch_bounds__(WAVE) k_match_team_sample(const int32_t *counts, int trees, int ensemble, float temperature,
                                                            uint64_t seed, uint64_t ply, int32_t *summed, int32_t *actions,
                                                            int out_trees, int out_ensemble, int32_t *tree_actions, int64_t n)
{
    constexpr int L = G::LANES, A = G::ACTIONS;
    const int lane = threadIdx.x, sub = lane % L;
    const int64_t game = static_cast<int64_t>(blockIdx.x) * (WAVE / L) + lane / L;
    const bool live = game < n;
    const int64_t g = live ? game : 0;
    int c0, c1;
    team_counts<G>(counts, g, trees, ensemble, live, sub, c0, c1);
    PickLane pl;
    const int action = pick_move_counts<G, MATCH_STREAM>(c0, c1, live, lane, temperature, nullptr, seed, ply, g, pl);
    if (!live) return;
    if (summed != nullptr) {
        if (pl.has0) summed[g * A + sub] = c0;
        if (pl.has1) summed[g * A + sub + L] = c1;
    }
    if (sub == 0) actions[g] = action;
    if (tree_actions != nullptr) store_team_actions<G>(tree_actions, g, out_trees, out_ensemble, sub, action);
}

template <class G>
__global__ void __launch_bounds__(256) k_match_team_roots(const uint64_t *bb0, const uint64_t *bb1, const int32_t *turns,
                                                          int trees, int ensemble, RootState rs, int64_t n_trees)
{
    const int64_t t = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (t >= n_trees) return;
    const int64_t g = t / trees;
    const int j = static_cast<int>(t - g * trees);
    uint64_t a = bb0[g], b = bb1[g];
    if (ensemble) { a = ensemble_board<G>(a, j); b = ensemble_board<G>(b, j); }     // the side to move stays (player.py:291-292)
    rs.bb0[t] = a; rs.bb1[t] = b; rs.turn[t] = turns[g];
    if (rs.aux != nullptr) rs.aux[t] = G::root_aux(a, b);
}

}  // namespace

#define AZ_MATCH_DISPATCH(game, ...)                                               \
    do {                                                                           \
        if ((game) == Connect4Dev::GAME_ID) { using G = Connect4Dev; __VA_ARGS__; } \
        else { using G = OthelloDev; __VA_ARGS__; }                                 \
    } while (0)

void launch_match_ply(int game, MatchPly a, hipStream_t s)
{
    if (a.n <= 0) return;
    AZ_MATCH_DISPATCH(game, {
        const unsigned grid = static_cast<unsigned>((a.n + WAVE / G::LANES - 1) / (WAVE / G::LANES));
        hipLaunchKernelGGL(k_match_ply<G>, dim3(grid), dim3(WAVE), 0, s, a);
    });
}

void launch_match_sample(int game, const int32_t *counts, float temperature, uint64_t seed, uint64_t ply, int32_t *actions,
                         int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    AZ_MATCH_DISPATCH(game, {
        const unsigned grid = static_cast<unsigned>((n + WAVE / G::LANES - 1) / (WAVE / G::LANES));
        hipLaunchKernelGGL(k_match_sample<G>, dim3(grid), dim3(WAVE), 0, s, counts, temperature, seed, ply, actions, n);
    });
}

void launch_match_team_sample(int game, const int32_t *counts, int trees, int ensemble, float temperature, uint64_t seed,
                              uint64_t ply, int32_t *summed, int32_t *actions, int out_trees, int out_ensemble,
                              int32_t *tree_actions, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    AZ_MATCH_DISPATCH(game, {
        const unsigned grid = static_cast<unsigned>((n + WAVE / G::LANES - 1) / (WAVE / G::LANES));
        hipLaunchKernelGGL(k_match_team_sample<G>, dim3(grid), dim3(WAVE), 0, s, counts, trees, ensemble, temperature, seed, ply,
                           summed, actions, out_trees, out_ensemble, tree_actions, n);
    });
}

void launch_match_team_roots(int game, const uint64_t *bb0, const uint64_t *bb1, const int32_t *turns, int trees, int ensemble,
                             RootState rs, int64_t n, hipStream_t s)
{
    const int64_t n_trees = n * trees;
    if (n_trees <= 0) return;
    AZ_MATCH_DISPATCH(game, hipLaunchKernelGGL(k_match_team_roots<G>, dim3(static_cast<unsigned>((n_trees + 255) / 256)), dim3(256), 0,
                                               s, bb0, bb1, turns, trees, ensemble, rs, n_trees));
}

}  // namespace az
