// team.h - a team of trees per game (root-parallel play, the symmetry ensemble; player.py:248-329), the pieces the ply
// tails of the match driver (match_kernels.hip) and of the self-play driver (selfplay_kernels.hip) share: tree j of game
// g is tree g * trees + j of its engine; in an ensemble, tree j works in the frame of the game's j-th symmetry
// (board_sym.h).  One lane group per game as in sp_pick.h: lane e owns action e, Othello's pass rides with lane 0.
#pragma once

#include "board_sym.h"
#include "games.h"

namespace az {

// What lane `sub` of game g's group holds of the team's summed count row: c0 = sum over the trees of action sub's
// count, c1 (Othello, lane 0) of the pass's; tree j's row is read at the action's index in that tree's frame.
template <class G>
__device__ __forceinline__ void team_counts(const int32_t *counts, int64_t g, int trees, int ensemble, bool live, int sub,
                                            int &c0, int &c1)
{
    constexpr int L = G::LANES, A = G::ACTIONS;
    const bool has0 = live && sub < A, has1 = A > L && live && sub + L < A;
    const int32_t *row = counts + g * trees * A;
    c0 = 0; c1 = 0;
    for (int j = 0; j < trees; ++j, row += A) {
        if (has0) c0 += row[ensemble ? ensemble_action<G>(sub, j) : sub];
        if (has1) c1 += row[ensemble ? ensemble_action<G>(sub + L, j) : sub + L];
    }
}

// the move (game frame, -1: none) in the frames of a team's trees: lanes of the group share the trees
template <class G>
__device__ __forceinline__ void store_team_actions(int32_t *actions, int64_t g, int trees, int ensemble, int sub, int action)
{
    for (int j = sub; j < trees; j += G::LANES)
        actions[g * trees + j] = (action >= 0 && ensemble) ? ensemble_action<G>(action, j) : action;
}

// Head field `f` (0..5: root_N, root_Q, root_M, root_D, root_P1W, root_P2W) of the team's merged root statistics
// (symmetry.py:156-158, a float32 mean): stats [n * trees][G::STATS] as az_mcts_dev_root_stats writes them; float32
// adds in tree order starting from tree 0's value, then one float32 division.  Root-level, so no permutation.
// k_team_root_stats and the team form of k_sp_pick (the recorded root_wdl) both call this: same bits.
template <class G>
__device__ __forceinline__ float team_head_mean(const float *stats, int64_t g, int trees, int f)
{
    const float *p = stats + g * trees * G::STATS + f;
    float acc = p[0];
    for (int j = 1; j < trees; ++j) acc = __fadd_rn(acc, p[static_cast<size_t>(j) * G::STATS]);
    return __fdiv_rn(acc, static_cast<float>(trees));
}

}  // namespace az
