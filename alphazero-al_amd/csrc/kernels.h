// kernels.h - launch interface between the host engine (engine.hip) and the gfx950 kernels
// (kernels.hip, select_kernels.hip, backup_kernels.hip, rollout_search.hip and the *_kernels.hip of the drivers).  Everything here is plain data: device pointers and sizes.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "tree_layout.h"

namespace az {

// Search parameters of one launch: a by-value snapshot of the live az_search_config
// (MCTSNode.h:47-61) plus what the device needs besides.
struct SearchParams {
    float c_init, c_base, noise_eps, fpu_reduction, mlh_slope, mlh_cap, value_decay, alpha;
    float score_utility_factor;
    int   vl_count;
    int   use_symmetry;
    // c_puct(parent_n) = c_init + logf((parent_n + c_base + 1)/c_base) for parent_n < tab_n,
    // tabulated by the HOST libm so that the device takes the same branch the reference's
    // logf takes (MCTS.h:213-214).  cpuct_tab[tab_n + parent_n] = sqrtf(parent_n) (exact on both sides; a load
    // instead of the refinement sequence).
    const float *cpuct_tab;
    int   tab_n;
    // Othello terminal_aux = atanf(diff*turn / score_scale) * (2/pi) (Othello.h:260-266) for
    // diff*turn in [-64, 64], tabulated by the host libm for the same reason
    const float *term_aux_tab;
    // device generator key (used by the dev_* entry points only).  `call_ptr` points at a
    // counter in HBM that a one-thread kernel bumps after every use, so that a captured
    // hipGraph draws fresh numbers on every replay.
    uint64_t seed;
    const uint64_t *call_ptr;
    // per-tree root-noise epsilon (n trees, device memory) replacing `noise_eps` when set: the
    // self-play driver's noise decay over the plies of a game (game.py:87-91), where games have ages
    const float *noise_eps_tree;
};

struct TreeArena {
    HotRec  *hot;    // [B][2][S]: two halves per tree (tree_layout.h)
    ColdRec *cold;
    uint8_t *half;   // [B] the half a tree lives in now
    int32_t *root;   // [B] slot of each tree's root, relative to its half
    int32_t *used;   // [B] slots in use in that half
    int64_t  S;      // slots per half
    int      B;      // trees
};

// Root positions of the current call: two bitboards + side to move + the game's small integer
// (Connect4: index of the last mover, -1 on an empty board, Connect4.h:124-128; Othello:
// consecutive passes, 0 after an import, Othello.h:108-110)
struct RootState {
    uint64_t *bb0, *bb1;
    int32_t  *turn;
    int32_t  *aux;
};

// What a descent leaves behind for expansion/backup; flat index = tree*K + k
struct LeafBuf {
    int32_t  *slot;      // leaf node
    uint64_t *bb0, *bb1; // leaf position (unsymmetrised)
    int32_t  *turn;      // side to move at the leaf
    int32_t  *aux;       // the game's small integer at the leaf (see RootState)
    uint8_t  *nvalid;    // legal moves at the leaf (what an expansion will append)
    uint8_t  *flags;     // LEAF_*
    int32_t  *path_len;  // nodes on the path, root first (0 = no descent recorded)
    int32_t  *path;      // [flat*MAX_PATH + depth]
    int32_t  *sym;       // symmetry id shown to the evaluator
};

// Evaluator outputs for one backprop launch
struct EvalIn {
    const float   *policy;    // [n*K, A] in the frame the evaluator saw
    // host form (reference signature): absolute WDL and flags supplied by the caller
    const float   *d, *p1w, *p2w;
    const uint8_t *is_term;
    const int32_t *sym;       // VL host form: per leaf; nullptr -> LeafBuf::sym
    // fused form: relative [draw, win, loss] per leaf, terminal flag from LeafBuf
    const float   *wdl_rel;
    const float   *moves_left;
    // Dirichlet noise for root expansions, [B, A], already normalised (host RNG mode);
    // nullptr -> device generator
    const float   *root_noise;
};

// Device transposition table (tt_kernels.hip): entries of tt_entry_bytes(game) bytes - key (two u64 XORed
// with a checksum of the value), policy[A], relative wdl[3], auxiliary value, a stamp (0 = never written),
// padded to 64-byte lines: Connect4 64 B, Othello 320 B - in buckets of four
struct TtTable {
    void *e;
    uint64_t mask;                                  // entries - 1 (entries = power of two >= 4)
    unsigned long long *stats;                      // lookups, hits, inserts, replaced
};
size_t tt_entry_bytes(int game);

// bits of the engine's sticky device error word
constexpr int ERR_ARENA_OVERFLOW = 1;   // an expansion found no room in its tree's arena (it was dropped)
constexpr int ERR_LIST_OVERFLOW  = 2;   // a compact leaf list was asked to hold more entries than leaves exist

enum : int { CNT_SIMS = 0, CNT_LEVELS, CNT_EXPANSIONS, CNT_TERMINAL, CNT_DUP, CNT_BACKUP,
             CNT_SELECT_LAUNCHES, CNT_BACKPROP_LAUNCHES, CNT_N };
constexpr int CNT_STRIPES = 64;      // striped copies of the counters (CNT_N * 8 B = one 64-byte line each)
static_assert(CNT_N == 8, "one counter stripe is one 64-byte line");

// Every launcher takes the game id (AZ_GAME_*) and dispatches to the kernel instantiation.
void launch_import(int game, const int8_t *boards, const int32_t *turns, RootState rs, int B, hipStream_t s);
void launch_set_roots(int game, const uint64_t *bb0, const uint64_t *bb1, const int32_t *turns, RootState rs,
                      int B, hipStream_t s);
void launch_bump_call(uint64_t *call_ctr, hipStream_t s, uint64_t amount = 1);
// bump_call: the device generator's call counter, incremented once by the launch (nullptr: not)
// returns the name of the kernel it launched (a string literal)
const char *launch_select(int game, TreeArena ar, RootState rs, LeafBuf lf, SearchParams p, int K, bool vl,
                          unsigned long long *counters, hipStream_t s, uint64_t *bump_call = nullptr,
                          int64_t *zero = nullptr);   // zero: an int64 the launch clears (the live-leaf count)
void launch_backprop(int game, TreeArena ar, LeafBuf lf, SearchParams p, int K, bool vl, bool fused,
                     EvalIn in, unsigned long long *counters, int *err, hipStream_t s);
void launch_remove_vl(int game, TreeArena ar, LeafBuf lf, SearchParams p, int K, int strideK, hipStream_t s);
// Leaves -> evaluator input.  gen_sym: draw symmetry ids from the device generator (else read
// LeafBuf::sym).  Any output pointer may be nullptr.
void launch_export(int game, LeafBuf lf, SearchParams p, int n_leaves, bool gen_sym, int8_t *boards,
                   uint8_t *valid_mask, float *features, hipStream_t s);
// dev_noise: fresh root noise is written by the launch itself - from the device generator, or from
// `replay_noise` ([B, A] by edge index) when that is given
// A tree that occupies more than `compact_above` records has its kept subtree moved into its other half
// (compaction), the others re-root in place; max_live: device int that receives, by atomic max, the number
// of records a tree occupies afterwards; err: the engine's error word.
void launch_prune(int game, TreeArena ar, SearchParams p, const int32_t *actions, int32_t *noise_req,
                  bool dev_noise, hipStream_t s, const float *replay_noise, int *max_live, int *err, int compact_above);
void launch_apply_noise(int game, TreeArena ar, const int32_t *noise_req, const float *noise, hipStream_t s);
void launch_reset_masked(TreeArena ar, const uint8_t *mask, hipStream_t s);
void launch_counts(int game, TreeArena ar, int32_t *counts, hipStream_t s);
void launch_root_stats(int game, TreeArena ar, float *stats, hipStream_t s);
void launch_init_trees(TreeArena ar, hipStream_t s);
void launch_rollout(int game, LeafBuf lf, SearchParams p, int B, float *policy, float *d, float *p1w, float *p2w,
                    float *ml, uint8_t *is_term, hipStream_t s);
// n_sims whole pure-MCTS simulations of every tree in one launch (k_rollout_search, rollout_search.hip): descent, random
// playout, expansion + backup; simulation i draws from call number *p.call_ptr + call_off + i, the counter itself is not
// written; lf: only `path` is used (depths past the lane group)
void launch_rollout_search(int game, TreeArena ar, RootState rs, LeafBuf lf, SearchParams p, int n_sims, uint64_t call_off,
                           unsigned long long *counters, int *err, hipStream_t s);
void launch_game_step(int game, uint64_t *bb0, uint64_t *bb1, int32_t *turns, int32_t *aux, const int32_t *actions,
                      uint8_t *done, int32_t *winner, int64_t n, bool reset_finished, hipStream_t s);
// The device driver's ply tail (az_mcts_dev_ply_pick / az_mcts_dev_ply_advance, include/az_mcts.h): counts -> move at
// temperature 1 from the caller's exponential draws q [n, A]; and step + result + refill or death + tree reset + ply
// counters + totals behind the re-rooting, for the ar.B games of the engine's trees.
void launch_ply_pick(int game, const int32_t *counts, const float *q, const int32_t *ply, const uint8_t *dead,
                     int32_t *actions, int n, int decay_moves, bool hot_early, bool hot_late, hipStream_t s);
void launch_ply_advance(int game, TreeArena ar, uint64_t *bb0, uint64_t *bb1, int32_t *turns, int32_t *aux,
                        const int32_t *actions, uint8_t *done, int32_t *winner, int32_t *ply, uint8_t *dead,
                        int64_t *totals, bool refill, hipStream_t s);
void launch_game_valid_mask(int game, const uint64_t *bb0, const uint64_t *bb1, const int32_t *turns, const int32_t *aux,
                            uint8_t *mask, int64_t n, hipStream_t s);

// err: the engine's sticky error word (ERR_* bits)
// symmetry ids + action masks + (idx != nullptr) the compact list of non-terminal leaves, for evaluators that read
// leaf positions; `count` must have been cleared (the selection launch does)
void launch_leaf_prep(int game, LeafBuf lf, SearchParams p, int n_leaves, bool gen_sym, uint8_t *valid_mask, int32_t *idx,
                      int64_t *count, int *err, hipStream_t s);
void launch_live_leaves(LeafBuf lf, int n_leaves, int32_t *idx, int64_t *count, int *err, hipStream_t s, bool clear_count = true);
void launch_tt_lookup(int game, LeafBuf lf, int n_leaves, TtTable t, const uint64_t *clock, float *probs, float *wdl, float *ml,
                      int32_t *miss_idx, int64_t *miss_count, uint64_t *keys, int *err, hipStream_t s);
void launch_tt_insert(int game, int n_leaves, TtTable t, const uint64_t *clock, const int32_t *miss_idx, const int64_t *miss_count,
                      const uint64_t *keys, const float *probs, const float *wdl, const float *ml, hipStream_t s);

// table refresh (MCTS_cpp.py:361-377): entries [e0, e0+n) -> positions + masks + compact list; fresh values -> same keys
void launch_tt_refresh_gather(int game, TtTable t, uint64_t e0, int n, uint64_t *bb_p1, uint64_t *bb_p2, int32_t *turn, int32_t *sym,
                              uint8_t *mask, int32_t *rows, int64_t *count, uint64_t *keys, hipStream_t s);
void launch_tt_refresh_store(int game, TtTable t, uint64_t e0, int n, const int32_t *rows, const int64_t *count, const uint64_t *keys,
                             const float *probs, const float *wdl, const float *ml, hipStream_t s);

// ---- native self-play driver (selfplay_kernels.hip) ------------------------------------------------
// Trajectory rows, structure of arrays: row r of a store (the games in progress: slot * rows_per_game + ply;
// the finished store: packed, a game's rows 0..len are adjacent)
struct SpRows {
    uint64_t *bb0, *bb1;
    int8_t   *turn;
    float    *prob;      // [rows][A]
    float    *wdl;       // [rows][3]
    uint8_t  *mask;      // [rows][A]
};

struct SpPick {
    const int32_t *counts;   // [n][A] root visit counts
    const float   *stats;    // [n][STATS] root statistics (recording only)
    const int32_t *ply;      // [n]
    const uint8_t *dead;     // [n] or nullptr: slots whose game is over (action -1)
    const int32_t *tape;     // [n] or nullptr: this ply's actions, read instead of drawn
    int32_t       *actions;  // [n]
    const uint64_t *bb0, *bb1;   // positions (recording only)
    const int32_t *turn, *aux;
    SpRows  rec;
    int     rows_per_game;
    float   temperature, temp_endgame;
    int     temp_decay_moves;
    uint64_t seed, call;     // generator key: the engine's seed and the driver's ply counter
    int64_t n;
    // The team form (k_sp_pick's TEAM instantiation; MatchPly's conventions): game_actions != nullptr selects it.  n is
    // then the number of GAMES, counts [n * trees][A] and stats [n * trees][STATS] hold a game's trees side by side, the
    // rows are summed per game (through the symmetries of an ensemble) before the pick, whose draws are keyed by the game.
    int      trees, ensemble;
    int32_t *game_actions;   // [n] out: the move in the game's frame (what the game step reads); `actions` is then
                             // [n * trees] or nullptr: the move in each tree's own frame (what the re-rooting reads)
    uint8_t *tree_done;      // [n * trees] or nullptr, out: 1 iff the tree's game ends with this move (the trees' reset
                             // reads it; needs bb0 / bb1 / turn / aux: the kernel steps the position in registers)
    int32_t *summed;         // [n][A] or nullptr, out: the summed row
};

struct SpAdvance {
    uint64_t *bb0, *bb1;
    int32_t  *turn, *aux, *ply;
    uint8_t  *dead;
    const uint8_t *done;
    const int32_t *winner;
    int64_t  n;
    int      refill, record;
    SpRows   rec, fin;
    int      rows_per_game;
    int32_t *fin_slot, *fin_len, *fin_winner;
    int64_t *fin_ply, *fin_row0;
    unsigned long long *n_alloc, *n_rows;    // games asked for (may pass `capacity`: those were dropped), rows handed out
    int64_t  capacity;                       // games the finished store holds
    int64_t  driver_ply;
    int      trees;                          // trees per game (0 counts as 1)
    float   *eps;                            // [n * trees] noise epsilon of the next ply, the game's value for each of its trees, or nullptr
    int      noise_steps;
    double   noise_eps_init, noise_eps_min;
    unsigned long long *totals;              // positions, games, p1 wins, p2 wins, draws
};

void launch_sp_pick(int game, SpPick a, bool record, hipStream_t s);
void launch_sp_advance(int game, SpAdvance a, hipStream_t s);
// Merged root statistics of a team (k_team_root_stats; symmetry.py:140-186 `inverse_sym_stats`): stats [n * trees][6 + 8A]
// as launch_root_stats writes them -> merged [n][6 + 8A] in the game's frame
void launch_team_root_stats(int game, const float *stats, int trees, int ensemble, float *merged, int64_t n, hipStream_t s);

// Packed games -> replay-buffer rows in a ring (k_sp_export; az_replay_tensors in az_mcts.h).  Game g: rows
// src_row0[g] .. src_row0[g] + len[g] of `fin`, written to the ring slots (ptr + dst_row0[g] + t) % capacity.
// dst_row0 ascends and is packed: the call carries dst_row0[n-1] + len[n-1] + 1 rows.
struct SpExport {
    SpRows fin;                              // read only
    const int32_t *len, *winner;             // [n_games]
    const int64_t *src_row0, *dst_row0;      // [n_games]
    int64_t  n_games;
    int8_t  *state;                          // [capacity][3][ROWS][COLS]
    float   *prob;                           // [capacity][A]
    int8_t  *out_winner;                     // [capacity]
    int16_t *steps_to_end, *aux_target;      // [capacity]
    float   *root_wdl, *future_root_wdl;     // [capacity][3]
    uint8_t *valid_mask;                     // [capacity][A]
    int64_t  capacity, ptr;
    int      td_steps;
};

void launch_sp_export(int game, SpExport a, hipStream_t s);

// ---- evaluation matches between two engines (match_kernels.hip) -------------------------------------
// One ply's tail of a match (k_match_ply; az_match_* in az_mcts.h): the mover engine's root counts -> the move, the
// stepped position, what both engines' re-rooting and resets read, results, the move record, totals.
// A player's trees of one game are its team: tree j of game g is tree g * trees + j of that player's engine; in an
// ensemble team, tree j works in the frame of the game's j-th symmetry (board_sym.h).
struct MatchTeam {
    int32_t *actions;        // [n * trees] out: what this engine's prune reads, the move in each tree's own frame
    uint8_t *done;           // [n * trees] out: 1 iff the tree's game ended on this ply (this engine's reset reads it)
    int      trees, ensemble;
};
struct MatchPly {
    const int32_t *counts;   // [n * trees][A] root visit counts of the engine that searched (trees: the mover's)
    int      trees, ensemble;    // the mover's team: its rows are summed per game, through the symmetries of an ensemble
    const int32_t *tape;     // [n] or nullptr: this ply's actions, read instead of picked
    uint64_t *bb0, *bb1;     // [n] positions, stepped in place
    int32_t  *turn, *aux;
    int32_t  *length;        // [n] plies played
    uint8_t  *dead;          // [n] the game is over: action -1 from then on
    MatchTeam team[2];       // the trees of player +1 / -1
    int32_t  *winner;        // [n] +1 / -1 / 0, written when the game ends
    int32_t  *moves;         // [max_plies][n] or nullptr: row `ply` is written (the game's frame)
    unsigned long long *totals;   // won by +1, won by -1, drawn, finished
    float    temperature;
    uint64_t seed, ply;      // generator key: engine_p1's seed and the match's ply counter
    int64_t  n;              // games
};
void launch_match_ply(int game, MatchPly a, hipStream_t s);
// the pick alone on caller-supplied counts (az_match_sample): counts [n][A] -> actions [n], same generator stream
void launch_match_sample(int game, const int32_t *counts, float temperature, uint64_t seed, uint64_t ply, int32_t *actions,
                         int64_t n, hipStream_t s);
// the team form of it (az_match_team_sample): counts [n * trees][A] -> summed [n][A] (or nullptr), actions [n], and the
// move in the frames of a team of out_trees trees, tree_actions [n * out_trees] (or nullptr)
void launch_match_team_sample(int game, const int32_t *counts, int trees, int ensemble, float temperature, uint64_t seed,
                              uint64_t ply, int32_t *summed, int32_t *actions, int out_trees, int out_ensemble,
                              int32_t *tree_actions, int64_t n, hipStream_t s);
// positions [n] -> a team's roots [n * trees], symmetrised for an ensemble (k_match_team_roots); rs.aux may be nullptr
void launch_match_team_roots(int game, const uint64_t *bb0, const uint64_t *bb1, const int32_t *turns, int trees, int ensemble,
                             RootState rs, int64_t n, hipStream_t s);

// ---- training batches from the replay ring (replay_kernels.hip) -------------------------------------
// Ring rows -> one augmented batch (k_replay_batch; az_replay_batch in az_mcts.h).  Sample b of the batch is the
// ring row idx[order ? order[first + b] : first + b]; it becomes the output rows s * B + b, s = 0 .. S - 1, one
// per board symmetry of the game.  A row number outside [0, capacity) gives zero rows and reads nothing.
struct ReplayBatch {
    // the ring, read only
    const int8_t  *state;                    // [capacity][3][ROWS][COLS]
    const float   *prob;                     // [capacity][A]
    const int8_t  *winner;                   // [capacity]
    const int16_t *steps_to_end, *aux_target;
    const float   *root_wdl, *future_root_wdl;   // [capacity][3]
    const uint8_t *valid_mask;               // [capacity][A]
    int64_t capacity;
    const int64_t *idx, *order;              // order may be nullptr
    int64_t first, B;
    // the batch, [S * B] rows each
    float   *o_state;                        // [S*B][3][ROWS][COLS]
    float   *o_prob;                         // [S*B][A]
    int8_t  *o_winner;
    int16_t *o_steps_to_end, *o_aux_target;
    float   *o_root_wdl, *o_future_root_wdl;
    uint8_t *o_valid_mask;                   // [S*B][A]
};

int  replay_num_augment(int game);           // S: 2 (Connect4), 4 (Othello)
void launch_replay_batch(int game, ReplayBatch a, hipStream_t s);
// n indices uniform in [0, n_valid), element e from the generator stream (seed, call, e, REPLAY_STREAM)
void launch_replay_indices(uint64_t seed, uint64_t call, int64_t n_valid, int64_t *idx, int64_t n, hipStream_t s);

}  // namespace az
