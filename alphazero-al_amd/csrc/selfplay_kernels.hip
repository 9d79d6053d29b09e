// selfplay_kernels.hip - the ply tail of the native self-play driver (az_selfplay_* in az_mcts.h),
// instantiated per game like the tree kernels.
//
//   k_sp_pick     root visit counts -> the move of every game (player.py:348-371 with the temperature
//                 schedule of game.py:55-63) and, when recording, this ply's row of the game's
//                 trajectory (game.py:97-108).  One lane group per game as in kernels.hip (Connect4: 8
//                 lanes, 8 games per wavefront; Othello: a wavefront): lane e owns action e, Othello's
//                 65th action (pass) rides with lane 0.  The pick itself is sp_pick.h, shared with k_match_ply.
//                 Its team form (a team of trees per game, team.h) sums the team's count rows first, writes
//                 the move per game and per tree, `done` per tree, and records the merged root_wdl.
//   k_team_root_stats  a team's root statistics merged into the game's frame (symmetry.py:140-186).
//   k_sp_advance  after the re-rooting and the game step: ply counters, finished games' rows into the
//                 finished store, refill, next ply's noise epsilon (game.py:87-91; per tree of the
//                 game's team), running totals.
//                 One lane per game for the bookkeeping; a wavefront then copies the rows of ITS
//                 finished games together - bytes moved follow the games that ended, not slots x plies.
//   k_sp_export   the packed store of finished games -> the learner's replay-buffer rows, written in place
//                 into a ring in HBM: what game.py:110-157 (winner per row, steps to the end, the auxiliary
//                 target, the td-step column, the end-state row) followed by ReplayBuffer.py:92-123 (`store`,
//                 row by row, index _ptr % capacity) leaves there.  One workgroup per game; consecutive
//                 lanes write consecutive bytes of consecutive ring rows.
//
// Plain C++ and vector stores only.  Store rows are handed out per WAVEFRONT: a ballot counts the
// finished games, one lane adds the wave's figures to the two counters (games, rows), ranks come from
// the ballot and a wave-wide prefix sum - two atomics per wavefront that has a finished game, none else.
#include "kernels.h"

#include "dev_rng.h"
#include "games.h"
#include "sp_pick.h"
#include "team.h"

namespace az {
namespace {

constexpr int WAVE = 64;

// TEAM (player.py:248-329 with is_selfplay = 1): the game's `trees` count rows are one row in registers before the pick -
// lane e adds up its action's count over the rows, in an ensemble through each tree's symmetry (team.h; plain loads, no
// cross-lane traffic) - the draws are keyed by the GAME, the move goes once to the game (the game's frame) and to every
// tree in the tree's own frame, every lane of the group steps a copy of the position in registers as k_match_ply does
// and the group's lanes write `done` per tree (k_game_step still owns the stored position), and the recorded root_wdl is
// the team's merged one (team_head_mean, what k_team_root_stats gives).
template <class G, bool RECORD, bool TEAM>
__global__ void __launch_bounds__(WAVE) k_sp_pick(SpPick a)
{
    constexpr int L = G::LANES, A = G::ACTIONS;
    const int lane = threadIdx.x, sub = lane % L;
    const int64_t game = static_cast<int64_t>(blockIdx.x) * (WAVE / L) + lane / L;
    const bool live = game < a.n;
    const int64_t g = live ? game : 0;
    const int ply = a.ply[g];
    const bool dead = a.dead != nullptr && a.dead[g] != 0;

    // game.py:55-63
    const float temp = (a.temp_decay_moves <= 0 || ply < a.temp_decay_moves) ? a.temperature : a.temp_endgame;
    PickLane pl;
    int action;
    if (TEAM) {
        int c0, c1;
        team_counts<G>(a.counts, g, a.trees, a.ensemble, live, sub, c0, c1);
        action = pick_move_counts<G, SP_STREAM>(c0, c1, live, lane, temp, a.tape, a.seed, a.call, g, pl);
        if (action < 0 || action >= A) action = -1;        // a tape's -1: the game does not move
    } else {
        action = pick_move<G, SP_STREAM>(a.counts + g * A, live, lane, temp, a.tape, a.seed, a.call, g, pl);
    }
    const int n0 = pl.n0, n1 = pl.n1;
    const bool has0 = pl.has0, has1 = pl.has1;
    const long long total = pl.total;
    if (dead) action = -1;
    GameState s;
    if (TEAM) {
        const bool stepped = a.tree_done != nullptr;
        if (RECORD || stepped) { s.bb0 = a.bb0[g]; s.bb1 = a.bb1[g]; s.turn = a.turn[g]; s.aux = a.aux[g]; }
        if (live) {
            if (sub == 0) a.game_actions[g] = action;
            if (a.actions != nullptr) store_team_actions<G>(a.actions, g, a.trees, a.ensemble, sub, action);
            if (a.summed != nullptr) {
                if (has0) a.summed[g * A + sub] = n0;
                if (has1) a.summed[g * A + sub + L] = n1;
            }
            if (stepped) {
                // k_game_step's rule on a copy: it steps the stored position after the re-rooting
                int res = -1;
                if (action >= 0) {
                    GameState t = s;
                    G::step(t, action);
                    res = G::result(t);
                }
                for (int j = sub; j < a.trees; j += L) a.tree_done[g * a.trees + j] = res >= 0 ? 1 : 0;
            }
        }
    } else {
        if (live && sub == 0) a.actions[g] = action;
    }

    if (RECORD) {
        if (!live || dead || ply < 0 || ply >= a.rows_per_game) return;
        const size_t r = static_cast<size_t>(g) * a.rows_per_game + ply;
        if (!TEAM) { s.bb0 = a.bb0[g]; s.bb1 = a.bb1[g]; s.turn = a.turn[g]; s.aux = a.aux[g]; }
        if (sub == 0) {
            a.rec.bb0[r] = s.bb0; a.rec.bb1[r] = s.bb1; a.rec.turn[r] = static_cast<int8_t>(s.turn);
            if (TEAM) {
#pragma unroll
                for (int f = 0; f < 3; ++f) a.rec.wdl[r * 3 + f] = team_head_mean<G>(a.stats, g, a.trees, 3 + f);
            } else {
                const float *st = a.stats + g * G::STATS;
                a.rec.wdl[r * 3 + 0] = st[3]; a.rec.wdl[r * 3 + 1] = st[4]; a.rec.wdl[r * 3 + 2] = st[5];
            }
        }
        // player.py:356: int / int in double, rounded once to f32
        const double den = static_cast<double>(total);
        if (has0) {
            a.rec.prob[r * A + sub] = total > 0 ? static_cast<float>(static_cast<double>(n0) / den) : 0.0f;
            a.rec.mask[r * A + sub] = G::valid_in_frame(s, 0, sub) ? 1 : 0;
        }
        if (has1) {
            a.rec.prob[r * A + sub + L] = total > 0 ? static_cast<float>(static_cast<double>(n1) / den) : 0.0f;
            a.rec.mask[r * A + sub + L] = G::valid_in_frame(s, 0, sub + L) ? 1 : 0;
        }
    }
}

template <class G>
__global__ void __launch_bounds__(WAVE) k_sp_advance(SpAdvance a)
{
    constexpr int A = G::ACTIONS;
    const int lane = threadIdx.x;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * WAVE + lane;
    const bool live = i < a.n;
    const int64_t g = live ? i : 0;
    const bool was_dead = a.dead[g] != 0;
    const bool fin = live && a.done[g] != 0;          // a dead slot played action -1: done == 0
    const int win = a.winner[g];
    int ply = a.ply[g];
    if (!was_dead) ply += 1;
    GameState s;
    s.bb0 = a.bb0[g]; s.bb1 = a.bb1[g]; s.turn = a.turn[g]; s.aux = a.aux[g];

    const unsigned long long fin_mask = __ballot(fin);
    if (fin_mask != 0 && a.record) {
        const int n_fin = __popcll(fin_mask);
        const int rank = __popcll(fin_mask & ((1ull << lane) - 1ull));
        unsigned long long base_g = 0;
        if (lane == 0) base_g = atomicAdd(a.n_alloc, static_cast<unsigned long long>(n_fin));
        base_g = __shfl(base_g, 0, WAVE);
        // a full store drops the game (the host counts n_alloc - capacity as dropped)
        const bool keep = fin && base_g + rank < static_cast<unsigned long long>(a.capacity);
        const int T = ply < a.rows_per_game ? ply : a.rows_per_game;      // rows the game recorded
        const int my_rows = keep ? T + 1 : 0;                             // + the end state
        int incl = my_rows;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int w = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += w;
        }
        const int wave_rows = __shfl(incl, WAVE - 1, WAVE);
        unsigned long long base_r = 0;
        if (lane == 0 && wave_rows) base_r = atomicAdd(a.n_rows, static_cast<unsigned long long>(wave_rows));
        base_r = __shfl(base_r, 0, WAVE);
        const size_t row0 = static_cast<size_t>(base_r) + incl - my_rows;
        if (keep) {
            const size_t gi = static_cast<size_t>(base_g) + rank;
            a.fin_slot[gi] = static_cast<int32_t>(g); a.fin_len[gi] = T; a.fin_winner[gi] = win;
            a.fin_ply[gi] = a.driver_ply; a.fin_row0[gi] = static_cast<int64_t>(row0);
            a.fin.bb0[row0 + T] = s.bb0; a.fin.bb1[row0 + T] = s.bb1; a.fin.turn[row0 + T] = static_cast<int8_t>(s.turn);
        }
        // the wavefront moves the rows of its finished games, one game after the other
        for (unsigned long long m = __ballot(keep); m; m &= m - 1) {
            const int src = __ffsll(static_cast<long long>(m)) - 1;
            const size_t from = static_cast<size_t>(__shfl(static_cast<int>(g), src, WAVE)) * a.rows_per_game;
            const int Ts = __shfl(T, src, WAVE);
            const size_t to = static_cast<size_t>(__shfl(static_cast<long long>(row0), src, WAVE));
            for (int e = lane; e < Ts; e += WAVE) {
                a.fin.bb0[to + e] = a.rec.bb0[from + e]; a.fin.bb1[to + e] = a.rec.bb1[from + e];
                a.fin.turn[to + e] = a.rec.turn[from + e];
            }
            for (int e = lane; e < (Ts + 1) * 3; e += WAVE) a.fin.wdl[to * 3 + e] = e < Ts * 3 ? a.rec.wdl[from * 3 + e] : 0.0f;
            for (int e = lane; e < (Ts + 1) * A; e += WAVE) {
                const bool in = e < Ts * A;
                a.fin.prob[to * A + e] = in ? a.rec.prob[from * A + e] : 0.0f;
                a.fin.mask[to * A + e] = in ? a.rec.mask[from * A + e] : 0;
            }
        }
    }

    if (fin) {
        if (a.refill) {
            G::start(s);
            a.bb0[g] = s.bb0; a.bb1[g] = s.bb1; a.turn[g] = s.turn; a.aux[g] = 0;
            ply = 0;
        } else {
            a.dead[g] = 1;
        }
    }
    if (live) {
        a.ply[g] = ply;
        if (a.eps != nullptr) {
            // game.py:87-91 in double, then one rounding
            const double decay = fmax(0.0, 1.0 - static_cast<double>(ply) / static_cast<double>(a.noise_steps));
            const float eps = static_cast<float>(a.noise_eps_min + (a.noise_eps_init - a.noise_eps_min) * decay);
            // the engine reads one value per TREE: the game's, for each tree of its team
            const int trees = a.trees > 1 ? a.trees : 1;
            for (int j = 0; j < trees; ++j) a.eps[g * trees + j] = eps;
        }
    }
    if (lane == 0) {
        if (blockIdx.x == 0) atomicAdd(&a.totals[0], static_cast<unsigned long long>(a.n));
        if (fin_mask) {
            atomicAdd(&a.totals[1], static_cast<unsigned long long>(__popcll(fin_mask)));
        }
    }
    const unsigned long long w1 = __ballot(fin && win == 1), w2 = __ballot(fin && win == -1), w0 = __ballot(fin && win == 0);
    if (lane == 0) {
        if (w1) atomicAdd(&a.totals[2], static_cast<unsigned long long>(__popcll(w1)));
        if (w2) atomicAdd(&a.totals[3], static_cast<unsigned long long>(__popcll(w2)));
        if (w0) atomicAdd(&a.totals[4], static_cast<unsigned long long>(__popcll(w0)));
    }
}

// ---- k_team_root_stats --------------------------------------------------------------------------------
// symmetry.py:140-186 (`inverse_sym_stats`) for trees j = 0 .. trees - 1 of every game: rows of launch_root_stats
// (head root_N, root_Q, root_M, root_D, root_P1W, root_P2W; then per action N, Q, prior, noise, M, D, P1W, P2W) ->
// one row per game in the game's frame.  Lane e of the game's group owns action e and reads tree j's eight values at the
// action's index in that tree's frame (the perms are involutions, the pass stays; identity without an ensemble); lane 0
// writes the head.  All float32, every product and sum rounded on its own (no fused multiply-add), every sum taken in
// tree order starting from tree 0's term: numpy sums a column of fewer than 8 values in that order and pairwise from 8
// on, so from 8 trees on the merged means may differ from numpy's in the last bit.
//   head             sum / trees
//   N                sum
//   prior, noise     sum / trees
//   Q, M, D, P1W, P2W  sum_j(x_j * N_j) / sum_j(N_j) where that denominator is > 0, else 0
template <class G>
__global__ void __launch_bounds__(WAVE) k_team_root_stats(const float *stats, int trees, int ensemble, float *merged, int64_t n)
{
    constexpr int L = G::LANES, A = G::ACTIONS, ST = G::STATS;
    const int lane = threadIdx.x, sub = lane % L;
    const int64_t g = static_cast<int64_t>(blockIdx.x) * (WAVE / L) + lane / L;
    if (g >= n) return;                                    // no cross-lane traffic below
    const float *in = stats + g * trees * ST;
    float *out = merged + g * ST;
    if (sub == 0) {
#pragma unroll
        for (int f = 0; f < 6; ++f) out[f] = team_head_mean<G>(stats, g, trees, f);
    }
    const float k = static_cast<float>(trees);
    for (int act = sub; act < A; act += L) {
        float sum_n = 0.0f, prior = 0.0f, noise = 0.0f, q = 0.0f, m = 0.0f, d = 0.0f, p1 = 0.0f, p2 = 0.0f;
        for (int j = 0; j < trees; ++j) {
            const float *r = in + static_cast<size_t>(j) * ST + 6 + 8 * (ensemble ? ensemble_action<G>(act, j) : act);
            const float w = r[0];
            const float tq = __fmul_rn(r[1], w), tm = __fmul_rn(r[4], w), td = __fmul_rn(r[5], w);
            const float t1 = __fmul_rn(r[6], w), t2 = __fmul_rn(r[7], w);
            if (j == 0) {
                sum_n = w; prior = r[2]; noise = r[3]; q = tq; m = tm; d = td; p1 = t1; p2 = t2;
            } else {
                sum_n = __fadd_rn(sum_n, w); prior = __fadd_rn(prior, r[2]); noise = __fadd_rn(noise, r[3]);
                q = __fadd_rn(q, tq); m = __fadd_rn(m, tm); d = __fadd_rn(d, td); p1 = __fadd_rn(p1, t1); p2 = __fadd_rn(p2, t2);
            }
        }
        const bool any = sum_n > 0.0f;
        float *o = out + 6 + 8 * act;
        o[0] = sum_n;
        o[1] = any ? __fdiv_rn(q, sum_n) : 0.0f;
        o[2] = __fdiv_rn(prior, k);
        o[3] = __fdiv_rn(noise, k);
        o[4] = any ? __fdiv_rn(m, sum_n) : 0.0f;
        o[5] = any ? __fdiv_rn(d, sum_n) : 0.0f;
        o[6] = any ? __fdiv_rn(p1, sum_n) : 0.0f;
        o[7] = any ? __fdiv_rn(p2, sum_n) : 0.0f;
    }
}

// ---- k_sp_export --------------------------------------------------------------------------------------
// The bit of a cell of the [ROWS][COLS] planes (env_common.h:93-119): Connect4 keeps bit 7 * col + height and
// draws row 0 at the top; Othello keeps bit 8 * row + col.
template <class G>
__device__ __forceinline__ int cell_bit(int cell)
{
    if (G::GAME_ID == Connect4Dev::GAME_ID) return 7 * (cell % G::COLS) + (G::ROWS - 1 - cell / G::COLS);
    return cell;
}

// byte k of a state row: plane 0 the stones of the side to move, plane 1 the opponent's, plane 2 the turn sign
template <class G>
__device__ __forceinline__ uint32_t state_byte(uint64_t own, uint64_t opp, int turn, int k)
{
    const int plane = k / G::CELLS, cell = k % G::CELLS;
    if (plane == 2) return static_cast<uint8_t>(static_cast<int8_t>(turn));
    return static_cast<uint32_t>(((plane == 0 ? own : opp) >> cell_bit<G>(cell)) & 1ull);
}

// A state row in units of one store: Connect4's 126-byte rows keep consecutive rows 2-byte aligned (63 stores of
// 2 bytes), Othello's 192-byte rows 16-byte aligned (12 stores of 16 bytes).
template <class G> struct StateUnit { using type = uint16_t; };
template <> struct StateUnit<OthelloDev> { using type = uint4; };

template <class G>
__device__ __forceinline__ void state_unit(uint64_t own, uint64_t opp, int turn, int u, uint16_t &out)
{
    out = static_cast<uint16_t>(state_byte<G>(own, opp, turn, 2 * u) | (state_byte<G>(own, opp, turn, 2 * u + 1) << 8));
}

template <class G>
__device__ __forceinline__ void state_unit(uint64_t own, uint64_t opp, int turn, int u, uint4 &out)
{
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        w[i] = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) w[i] |= state_byte<G>(own, opp, turn, 16 * u + 4 * i + j) << (8 * j);
    }
    out = make_uint4(w[0], w[1], w[2], w[3]);
}

constexpr int EXPORT_THREADS = 256;

template <class G>
__global__ void __launch_bounds__(EXPORT_THREADS) k_sp_export(SpExport a)
{
    using Unit = typename StateUnit<G>::type;
    constexpr int A = G::ACTIONS;
    constexpr int UNITS = 3 * G::CELLS / static_cast<int>(sizeof(Unit));
    static_assert(UNITS * sizeof(Unit) == 3 * G::CELLS, "a state row is a whole number of stores");
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    const int T = a.len[g], win = a.winner[g];
    const int64_t src = a.src_row0[g], dst = a.dst_row0[g], cap = a.capacity;
    // ring rule: of a call with more rows than the ring has slots only the last `capacity` rows are written -
    // what row-by-row stores would leave, and no two rows of one call share a slot
    const int64_t total = a.dst_row0[a.n_games - 1] + a.len[a.n_games - 1] + 1;
    const int64_t skip = total > cap ? total - cap : 0;
    const int t0 = dst >= skip ? 0 : static_cast<int>(skip - dst < T + 1 ? skip - dst : T + 1);
    const int n = T + 1 - t0;                                  // rows of this game that are written: <= capacity
    if (n <= 0) return;
    const int64_t base = (a.ptr + dst + t0) % cap;             // the modulo once per game, the wrap per row
    auto slot = [&](int j) { const int64_t i = base + j; return static_cast<size_t>(i >= cap ? i - cap : i); };

    const uint64_t end0 = a.fin.bb0[src + T], end1 = a.fin.bb1[src + T];
    const int diff = __popcll(end0) - __popcll(end1);          // game.py:17-30: discs of player +1 minus player -1

    Unit *state = reinterpret_cast<Unit *>(a.state);
    for (int e = tid; e < n * UNITS; e += EXPORT_THREADS) {
        const int j = e / UNITS, u = e % UNITS;
        const size_t r = static_cast<size_t>(src) + t0 + j;
        const int turn = a.fin.turn[r];
        const uint64_t p1 = a.fin.bb0[r], p2 = a.fin.bb1[r];
        Unit v;
        state_unit<G>(turn > 0 ? p1 : p2, turn > 0 ? p2 : p1, turn, u, v);
        state[slot(j) * UNITS + u] = v;
    }
    for (int e = tid; e < n * A; e += EXPORT_THREADS) {
        const int j = e / A, c = e % A, t = t0 + j;
        const size_t from = (static_cast<size_t>(src) + t) * A + c, to = slot(j) * A + c;
        a.prob[to] = t < T ? a.fin.prob[from] : 0.0f;
        a.valid_mask[to] = t < T ? (a.fin.mask[from] != 0 ? 1 : 0) : 1;
    }
    for (int e = tid; e < n * 3; e += EXPORT_THREADS) {
        const int j = e / 3, c = e % 3, t = t0 + j;
        const size_t from = (static_cast<size_t>(src) + t) * 3 + c, to = slot(j) * 3 + c;
        a.root_wdl[to] = t < T ? a.fin.wdl[from] : 0.0f;
        a.future_root_wdl[to] = (a.td_steps > 0 && a.td_steps < T - t) ? a.fin.wdl[from + static_cast<size_t>(a.td_steps) * 3] : 0.0f;
    }
    for (int j = tid; j < n; j += EXPORT_THREADS) {
        const int t = t0 + j;
        const size_t to = slot(j);
        a.out_winner[to] = static_cast<int8_t>(win);
        a.steps_to_end[to] = static_cast<int16_t>(T - t);
        if (G::GAME_ID == OthelloDev::GAME_ID) a.aux_target[to] = static_cast<int16_t>(diff * a.fin.turn[static_cast<size_t>(src) + t]);
        else a.aux_target[to] = static_cast<int16_t>(T - t);
    }
}

}  // namespace

#define AZ_SP_DISPATCH(game, ...)                                                  \
    do {                                                                           \
        if ((game) == Connect4Dev::GAME_ID) { using G = Connect4Dev; __VA_ARGS__; } \
        else { using G = OthelloDev; __VA_ARGS__; }                                 \
    } while (0)

void launch_sp_pick(int game, SpPick a, bool record, hipStream_t s)
{
    if (a.n <= 0) return;
    AZ_SP_DISPATCH(game, {
        const unsigned grid = static_cast<unsigned>((a.n + WAVE / G::LANES - 1) / (WAVE / G::LANES));
        if (a.game_actions != nullptr) {
            if (record) hipLaunchKernelGGL((k_sp_pick<G, true, true>), dim3(grid), dim3(WAVE), 0, s, a);
            else hipLaunchKernelGGL((k_sp_pick<G, false, true>), dim3(grid), dim3(WAVE), 0, s, a);
        } else {
            if (record) hipLaunchKernelGGL((k_sp_pick<G, true, false>), dim3(grid), dim3(WAVE), 0, s, a);
            else hipLaunchKernelGGL((k_sp_pick<G, false, false>), dim3(grid), dim3(WAVE), 0, s, a);
        }
    });
}

void launch_team_root_stats(int game, const float *stats, int trees, int ensemble, float *merged, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    AZ_SP_DISPATCH(game, {
        const unsigned grid = static_cast<unsigned>((n + WAVE / G::LANES - 1) / (WAVE / G::LANES));
        hipLaunchKernelGGL(k_team_root_stats<G>, dim3(grid), dim3(WAVE), 0, s, stats, trees, ensemble, merged, n);
    });
}

void launch_sp_advance(int game, SpAdvance a, hipStream_t s)
{
    if (a.n <= 0) return;
    AZ_SP_DISPATCH(game, hipLaunchKernelGGL(k_sp_advance<G>, dim3(static_cast<unsigned>((a.n + WAVE - 1) / WAVE)), dim3(WAVE), 0, s, a));
}

void launch_sp_export(int game, SpExport a, hipStream_t s)
{
    if (a.n_games <= 0) return;
    AZ_SP_DISPATCH(game, hipLaunchKernelGGL(k_sp_export<G>, dim3(static_cast<unsigned>(a.n_games)), dim3(EXPORT_THREADS), 0, s, a));
}

}  // namespace az
