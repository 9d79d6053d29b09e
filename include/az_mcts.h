/*
 * az_mcts.h - C ABI of the MI355X batched self-play search engine (libaz_mcts.so).
 *
 * This is the drop-in boundary for the reference's native search layer: every entry point
 * below replaces one method the reference binds in src/cpp/mcts_bindings.cpp (cited per
 * function, paths relative to the reference checkout).  Plain pointers and sizes only; no
 * torch / pybind types.  All trees live in HBM; the library fails (non-zero return,
 * message in az_last_error()) when no HIP device is usable - there is no CPU fallback.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error (AZ_ERR_*); the reference
 *     throws std::runtime_error at the same points (mcts_bindings.cpp:76-79,97-100,
 *     155-165,206-212,278-288,323-327) and the pybind layer re-raises RuntimeError.
 *   - "host" entry points take host pointers, are synchronous, and mirror the reference
 *     signature 1:1 (caller-allocated outputs instead of fresh numpy arrays).
 *   - "dev" entry points take DEVICE pointers and a hipStream_t (as void*), never
 *     synchronise, and are what the fused self-play loop uses (no host round trip).
 *   - flat leaf index of simulation k of tree i in a K-wide call is i*K + k
 *     (BatchedMCTS.h:221,251).
 */
#ifndef AZ_MCTS_H
#define AZ_MCTS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AZ_OK            0
#define AZ_ERR_ARG       1   /* size / shape / range mismatch (reference: runtime_error) */
#define AZ_ERR_DEVICE    2   /* HIP error or no device                                   */
#define AZ_ERR_CAPACITY  3   /* a tree arena overflowed (cannot happen unless growth is disabled) */
#define AZ_ERR_STATE     4   /* call sequence not supported                              */

#define AZ_GAME_CONNECT4 0
#define AZ_GAME_OTHELLO  1

/* Same fields, order and defaults as the reference SearchConfig (MCTSNode.h:47-61),
 * exposed as a LIVE struct exactly like `BatchedMCTS.config` (mcts_bindings.cpp:55-58):
 * the engine re-reads it at every call. */
typedef struct az_search_config {
    float   c_init;               /* 1.25    */
    float   c_base;               /* 19652   */
    float   dirichlet_alpha;      /* 0.3     */
    float   noise_epsilon;        /* 0.25    */
    float   fpu_reduction;        /* 0.4     */
    float   mlh_slope;            /* 0       */
    float   mlh_cap;              /* 0.2     */
    float   score_utility_factor; /* 0       */
    float   score_scale;          /* 8       */
    float   value_decay;          /* 1       */
    uint8_t use_symmetry;         /* true    */
    int32_t vl_count;             /* 1       */
} az_search_config;

typedef struct az_mcts az_mcts;

/* thread-local message of the last failing call */
const char *az_last_error(void);

/* static game geometry: BatchedMCTS_<G>.action_size / board_size (mcts_bindings.cpp:359-369) */
int az_game_action_size(int game);
int az_game_board_size(int game);
int az_game_board_rows(int game);
int az_game_board_cols(int game);

/* ---- lifetime ------------------------------------------------------------------------ */

/* BatchedMCTS(int n_envs), mcts_bindings.cpp:52 / BatchedMCTS.h:52-58.  device < 0 uses
 * the current HIP device. */
int  az_mcts_create(int game, int n_envs, int device, az_mcts **out);
void az_mcts_destroy(az_mcts *m);
/* `.config` property, mcts_bindings.cpp:55-58 */
az_search_config *az_mcts_config(az_mcts *m);
/* get_num_envs, mcts_bindings.cpp:68 */
int  az_mcts_num_envs(const az_mcts *m);
/* set_seed, mcts_bindings.cpp:61 / BatchedMCTS.h:68-84.  Seeds the host mt19937 that feeds
 * symmetry ids and Dirichlet noise in "reference RNG" mode (== the reference run with
 * OMP_NUM_THREADS=1) and the counter-based device generator used by the dev entry points. */
int  az_mcts_set_seed(az_mcts *m, int seed);
/* reset_env, mcts_bindings.cpp:65 / BatchedMCTS.h:93-99 (out-of-range index is ignored) */
int  az_mcts_reset_env(az_mcts *m, int env);
/* prune_roots, mcts_bindings.cpp:72-81 / MCTS.h:90-132; n must equal n_envs */
int  az_mcts_prune_roots(az_mcts *m, const int32_t *actions, int64_t n);

/* ---- host entry points (reference signatures) ----------------------------------------- */

/* search_batch, mcts_bindings.cpp:89-134 / BatchedMCTS.h:119-171 */
int az_mcts_search_batch(az_mcts *m, const int8_t *boards, const int32_t *turns, int64_t n,
                         int8_t *out_boards, float *out_term_d, float *out_term_p1w,
                         float *out_term_p2w, uint8_t *out_is_term, int32_t *out_turns,
                         uint8_t *out_valid_mask);
/* backprop_batch, mcts_bindings.cpp:139-179 / BatchedMCTS.h:176-199 */
int az_mcts_backprop_batch(az_mcts *m, const float *policy, const float *d, const float *p1w,
                           const float *p2w, const float *moves_left, const uint8_t *is_term,
                           int64_t n);
/* remove_all_vl, mcts_bindings.cpp:184-191 / BatchedMCTS.h:209-216 */
int az_mcts_remove_all_vl(az_mcts *m, int K);
/* search_batch_vl, mcts_bindings.cpp:197-252 / BatchedMCTS.h:227-286 */
int az_mcts_search_batch_vl(az_mcts *m, int K, const int8_t *boards, const int32_t *turns,
                            int64_t n, int8_t *out_boards, float *out_term_d,
                            float *out_term_p1w, float *out_term_p2w, uint8_t *out_is_term,
                            int32_t *out_turns, int32_t *out_sym_ids, uint8_t *out_valid_mask);
/* backprop_batch_vl, mcts_bindings.cpp:257-306 / BatchedMCTS.h:296-332; total must be n_envs*K */
int az_mcts_backprop_batch_vl(az_mcts *m, int K, const float *policy, const float *d,
                              const float *p1w, const float *p2w, const float *moves_left,
                              const uint8_t *is_term, const int32_t *sym_ids, int64_t total);
/* search(RolloutEvaluator, ...), mcts_bindings.cpp:313-337 / BatchedMCTS.h:339-407 with
 * RolloutEvaluator.h:23-48, in the reference's random stream like every host entry point: playout
 * moves (one uniform_int per move, leaves in env order) and root-noise rows come from the host
 * mt19937 as the reference with OMP_NUM_THREADS=1 consumes them - bit-exact against it (fixture G9);
 * selection, expansion and backup run on the device, one host round trip per playout. */
int az_mcts_search_rollout(az_mcts *m, const int8_t *boards, const int32_t *turns, int64_t n,
                           int n_playout);
/* The same search with the random playouts on the device as well (moves and noise from the device
 * generator: same distribution, another stream; no host round trip inside the loop). */
int az_mcts_search_rollout_dev(az_mcts *m, const int8_t *boards, const int32_t *turns, int64_t n,
                               int n_playout);
/* get_all_counts, mcts_bindings.cpp:342 / BatchedMCTS.h:413-427: out[n_envs*A] */
int az_mcts_get_all_counts(az_mcts *m, int32_t *out);
/* get_all_root_stats, mcts_bindings.cpp:348-356 / MCTS.h:637-673: out[n_envs*(6+8A)] */
int az_mcts_get_all_root_stats(az_mcts *m, float *out);

/* ---- device entry points (fused loop; no reference equivalent - they are what removes the
 *      four host crossings per iteration of MCTS_cpp.py:250-357) --------------------------- */

/* Must be called OUTSIDE any stream capture before the other dev_* calls and again whenever
 * the live config changed: sizes the leaf buffers for K descents per tree, refreshes the
 * c_puct table, and guarantees arena room for `sims_per_tree` more simulations per tree
 * (grows the arenas if needed; synchronises).  Reserve PER SEARCH: the host-side occupancy bound restarts
 * from the figure each az_mcts_dev_prune_roots reports, so room reserved before a re-rooting for
 * searches enqueued after it is forgotten - call this once for every search, after the re-rooting that
 * precedes it (as selfplay.py / fused.py do).  The room is sims_per_tree x the game's largest block of children
 * (Connect4 7; Othello 33, the most legal moves of a position REACHABLE in play): imported Othello positions with
 * more moves are searched correctly but can outrun the reservation - an expansion that does not fit is dropped and
 * raises the sticky error word (az_mcts_dev_check: arena full), never a store out of range. */
int az_mcts_dev_prepare(az_mcts *m, int K, int64_t sims_per_tree);
/* The same for a caller whose work on these trees is all on ONE stream: when the call has to look
 * at the trees (their fill), move a buffer or refresh a table, it waits for that stream only
 * instead of the whole device - what a driver with several engines on several streams wants. */
int az_mcts_dev_prepare_stream(az_mcts *m, int K, int64_t sims_per_tree, void *stream);
/* Sticky device error word, polled without stalling: enqueues a copy of the word to pinned host
 * memory on `stream` and reports what the PREVIOUS poll brought back - AZ_ERR_CAPACITY (message
 * in az_last_error) once an expansion found its arena full or a compact leaf list overflowed.
 * A self-play driver calls it once per ply; az_mcts_counters reports the same word synchronously. */
int az_mcts_dev_check(az_mcts *m, void *stream);
/* Test hook - recorded draws instead of the device generator.  The reference draws symmetry ids
 * and Dirichlet noise from one mt19937 in env order (BatchedMCTS.h:148-154,261-267; MCTS.h:113-132,
 * 352-358); the device loop has a counter-based generator of its own.  To compare the device loop
 * with the reference bit for bit, a test records what the reference (the oracle) drew and plays it
 * back: sym_ids int32 [n_select_calls][sym_stride] in DEVICE memory - the c-th az_mcts_dev_select
 * (or selection inside az_mcts_dev_search) after this call shows leaf `flat` under symmetry
 * sym_ids[c*sym_stride + flat] (0 for terminal leaves; running past the tape is AZ_ERR_STATE);
 * root_noise float [n_envs][A] in DEVICE memory, row = tree, column = EDGE index (legal moves in
 * ascending order), already normalised - what root expansions and az_mcts_dev_prune_roots store
 * from now on; the arrays are read when the kernels run, so update them in stream order.  Either
 * pointer may be NULL (that part stays with the generator); both NULL ends the replay. */
int az_mcts_dev_replay(az_mcts *m, const int32_t *sym_ids, int64_t sym_stride, int64_t n_select_calls,
                       const float *root_noise);
/* Root positions as bitboards already in HBM: bb_p1/bb_p2 uint64[n_envs], turn int32[n_envs]
 * (the reference passes int8 grids on every call, BatchedMCTS.h:136-137,244-245). */
int az_mcts_dev_set_roots(az_mcts *m, const uint64_t *bb_p1, const uint64_t *bb_p2,
                          const int32_t *turns, void *stream);
/* Same from int8 grids in HBM (device pointer), boards[n_envs*board_size]. */
int az_mcts_dev_import_roots(az_mcts *m, const int8_t *boards, const int32_t *turns, void *stream);
/* K descents per tree (K=1, vl=0: simulate; vl=1: simulate_vl), then gather of the leaves into
 * the evaluator's input: features float32[n_envs*K,3,rows,cols] in the reference's relative
 * planes (MCTS_cpp.py:15-20), action mask uint8[n_envs*K,A] (0 for terminal leaves).
 * Symmetry ids come from the device generator. */
int az_mcts_dev_select(az_mcts *m, int K, int vl, float *features, uint8_t *valid_mask,
                       void *stream);
/* Expansion + backup straight from the evaluator's outputs: probs float32[n*K,A] (leaf frame,
 * possibly mirrored), wdl_rel float32[n*K,3] = [draw, win, loss] for the side to move
 * (converted as MCTS_cpp.py:23-30), moves_left float32[n*K].  Terminal leaves ignore the
 * evaluator and use their cached result (MCTS_cpp.py:275-282). */
int az_mcts_dev_backprop(az_mcts *m, int K, int vl, const float *probs, const float *wdl_rel,
                         const float *moves_left, void *stream);
/* Leaf positions of the last dev_select (unsymmetrised): bb_p1/bb_p2 uint64[n*K],
 * turn int32[n*K], flags uint8[n*K] (bit 0 = terminal, bits 1-2 = result 0 draw / 1 P1 /
 * 2 P2).  Any pointer may be NULL. */
int az_mcts_dev_leaves(az_mcts *m, int K, uint64_t *bb_p1, uint64_t *bb_p2, int32_t *turns,
                       uint8_t *flags, void *stream);
/* Symmetry ids the leaves of the last dev_select (or of the last selection inside az_mcts_dev_search) were shown
 * under: int32[n*K] into HBM (0 for terminal leaves) - what BatchedMCTS.h:148-154,261-267 draws per leaf; lets a
 * test look at the device generator's draws themselves (tests/test_devrng_gpu.py). */
int az_mcts_dev_leaf_syms(az_mcts *m, int K, int32_t *sym_ids, void *stream);
/* Root visit counts int32[n_envs*A] / root stats float32[n_envs*(6+8A)] into HBM. */
int az_mcts_dev_counts(az_mcts *m, int32_t *counts, void *stream);
int az_mcts_dev_root_stats(az_mcts *m, float *stats, void *stream);
/* prune_roots with actions in HBM and Dirichlet noise from the device generator (or from az_mcts_dev_replay);
 * trees that run out of room are compacted into their other arena half on the way (see az_mcts_reserve). */
int az_mcts_dev_prune_roots(az_mcts *m, const int32_t *actions, void *stream);
/* Reset the trees whose mask byte is non-zero (mask uint8[n_envs] in HBM). */
int az_mcts_dev_reset_masked(az_mcts *m, const uint8_t *mask, void *stream);

/* Batched Connect4 positions in HBM - the device-side counterpart of Env.step / done /
 * winPlayer (env_common.h:141-147, env_connect4.h:38-40, Connect4.h:159-203) for a self-play
 * driver that keeps its games next to the trees: plays actions[i] in game i (bitboards and
 * side to move updated in place), writes done[i] (1 = won or board full) and winner[i]
 * (+1 / -1 / 0).  With reset_finished != 0 a finished game is replaced by the empty board
 * with player +1 to move.  Games with actions[i] < 0 are left untouched (done = 0). */
int az_c4_dev_step(uint64_t *bb_p1, uint64_t *bb_p2, int32_t *turns, const int32_t *actions,
                   uint8_t *done, int32_t *winner, int64_t n, int reset_finished, void *stream);
/* The same for either game (AZ_GAME_*).  `aux` [n] is the game's small integer carried from ply to
 * ply - Othello: consecutive passes so far (Othello.h:206-235, the Env keeps them although a tree
 * forgets them at every import, Othello.h:108-110); NULL: derived from the position as an import
 * derives it (enough for Connect4).  A finished game with reset_finished != 0 restarts from the
 * game's initial position (Connect4.h reset / Othello.h:62-75). */
int az_game_dev_step(int game, uint64_t *bb_p1, uint64_t *bb_p2, int32_t *turns, int32_t *aux,
                     const int32_t *actions, uint8_t *done, int32_t *winner, int64_t n, int reset_finished,
                     void *stream);
/* mask[i, a] = 1 iff action a is legal in position i (what `Env.valid_mask()` returns,
 * env_common.h; Othello: the pass action only when no placement exists, none after the end). */
int az_game_dev_valid_mask(int game, const uint64_t *bb_p1, const uint64_t *bb_p2, const int32_t *turns,
                           const int32_t *aux, uint8_t *mask, int64_t n, void *stream);

/* The tail of a self-play ply for a driver that keeps its games in HBM next to the trees, as two launches.
 *
 * az_game_dev_pick: root visit counts int32[n*A] -> actions int32[n] at temperature 1 (player.py:348-371 with the
 * schedule of game.py:55-63).  Weights are the positive counts as floats, a row without one counts as all ones; the
 * sampled move is the arg-max over the row of weight / q[i, a] (float32[n*A], the caller's Exp(1) draws: one draw
 * per row of a multinomial, the form torch.multinomial uses, so a caller that fills q from its torch generator
 * plays what torch.multinomial would have played); the greedy move is the arg-max of the counts; the lowest index
 * wins ties.  A game takes the sampled move when the temperature in force is above the greedy threshold:
 * hot_early while ply[i] < temp_decay_moves (always, when temp_decay_moves <= 0), hot_late from then on.
 * dead uint8[n] (NULL: none): slots that get action -1.
 *
 * az_mcts_dev_ply_advance, behind az_mcts_dev_prune_roots, for the n_envs games of the engine's trees:
 * az_game_dev_step's step, done[] and winner[] (a slot with an action out of range is left alone, done = 0); a
 * finished game restarts from the initial position with ply 0 (refill != 0) or its slot turns dead (dead[i] = 1);
 * its tree is reset (az_mcts_dev_reset_masked with done[] as the mask); ply[i] += 1 in slots that were not dead;
 * totals int64[5] += {n_envs, finished games, wins of +1, wins of -1, draws}.  All arrays in HBM, updated in place. */
int az_game_dev_pick(int game, const int32_t *counts, const float *q, const int32_t *ply, const uint8_t *dead,
                     int32_t *actions, int64_t n, int temp_decay_moves, int hot_early, int hot_late, void *stream);
int az_mcts_dev_ply_advance(az_mcts *m, uint64_t *bb_p1, uint64_t *bb_p2, int32_t *turns, int32_t *aux,
                            const int32_t *actions, uint8_t *done, int32_t *winner, int32_t *ply, uint8_t *dead,
                            int64_t *totals, int refill, void *stream);

/* Root-noise epsilon PER TREE: `per_tree` (n_envs floats in DEVICE memory, owned and kept alive by the
 * caller; NULL switches back to the config's scalar) replaces az_search_config.noise_epsilon in every
 * selection from the next launch on.  The reference decays one global epsilon over the plies of a batch
 * of games that start together (game.py:87-91, AlphaZeroPlayer.noise_steps); a driver that refills
 * finished slots has games of all ages in one batch and needs the value per game.  The array is read by
 * the kernels when they run: update it in stream order. */
int az_mcts_dev_set_noise_epsilons(az_mcts *m, const float *per_tree);

/* The leaves of the last az_mcts_dev_select that an evaluator has to see - all but the terminal
 * ones, as the reference's wrapper evaluates them (MCTS_cpp.py:275-297): their flat indices go to
 * leaf_idx[0 .. *leaf_count) (int32 [n*K] and int64 [1] in DEVICE memory; order unspecified). */
int az_mcts_dev_live_leaves(az_mcts *m, int K, int32_t *leaf_idx, int64_t *leaf_count, void *stream);

/* A whole search as ONE call: the iteration schedule of the reference's wrapper
 * (MCTS_cpp.py:110-113, 217-264: one plain simulation that expands every root, then virtual-loss
 * batches of K until n_playout simulations per tree are done) with the evaluator inside the loop -
 * az_mcts_dev_select, az_mcts_dev_live_leaves (or the table's lookup / insert when use_table != 0),
 * az_nn_model_forward (include/az_nn.h) on the leaves that need it, az_mcts_dev_backprop - every
 * launch issued from native code on `stream`, the leaf batch in buffers the engine owns.  Roots
 * are the ones set by az_mcts_dev_set_roots / import_roots; results are read with
 * az_mcts_dev_counts / root_stats.  Identical to issuing the same calls one by one (tests).  Engines
 * on different streams (and host threads) overlap on the device: one engine's selection and
 * backup kernels, which leave most of the chip idle, run under another engine's evaluator. */
struct az_nn_model;
int az_mcts_dev_search(az_mcts *m, const struct az_nn_model *model, int n_playout, int K, int use_table,
                       void *stream);
/* CONTINUES a search on the same roots: n_sims more simulations per tree as whole iterations (virtual-loss batches of
 * min(K, remaining); plain simulations for K <= 1) WITHOUT the warm-up simulation az_mcts_dev_search starts with.  A
 * search under a time budget (MCTS_cpp.py:70-87,200-209,252-261: wall-clock check and top-2 early exit between
 * iterations) is az_mcts_dev_search(.., 1, ..) followed by chunks of this call, with az_mcts_dev_counts read once per
 * chunk - alphazero-al_amd/src/fused.py `search_timed`.  Every call leaves the trees without in-flight visits. */
int az_mcts_dev_search_more(az_mcts *m, const struct az_nn_model *model, int n_sims, int K, int use_table,
                            void *stream);

/* BatchedMCTS::search with RolloutEvaluator (BatchedMCTS.h:339-407) on the roots set by az_mcts_dev_set_roots /
 * import_roots: n_playout plain simulations per tree, playouts and root noise from the device generator, as ONE
 * search kernel per chunk of sims_per_launch simulations (<= 0: the library's default) plus the call counter's
 * bump - same trees, counts and root statistics, bit for bit, as az_mcts_search_rollout_dev from the same seed
 * and call counter.  Reserves its own arena room (n_playout x the game's largest block of children); only
 * enqueues on `stream` unless a buffer must grow.  No selection or backup launch is issued: az_mcts_counters [6]
 * and [7] do not move, [0..5] count the same work as the launch-per-simulation route.  The leaves stay in
 * registers: what az_mcts_dev_leaves / az_mcts_dev_leaf_syms report after this call is unspecified.
 * AZ_ERR_ARG: n_playout < 0; AZ_ERR_CAPACITY arrives through az_mcts_dev_check. */
int az_mcts_dev_rollout_search(az_mcts *m, int n_playout, int sims_per_launch, void *stream);

/* ---- self-play from C: whole plies, recording included (alphazero-al_amd/csrc/selfplay_kernels.hip) -------
 * The reference's driver is Python per game and per ply (src/game.py:65-164 with src/player.py:333-375);
 * here a driver object owns the positions, ply counters, trajectories and the store of finished games in
 * HBM, and a ply outside the search is: root counts / statistics, k_sp_pick (the move, this ply's
 * trajectory row), the re-rooting, the game step, the tree resets, k_sp_advance (finished games' rows into
 * the store, refill, next epsilon, totals).  The driver borrows the engine: destroy it BEFORE the engine,
 * use one driver per engine, and make every call of a driver on ONE stream and from one thread at a time
 * (drivers on different engines, streams and host threads run side by side).  With noise_steps > 0 the
 * driver installs its per-game epsilons with az_mcts_dev_set_noise_epsilons.
 *
 * Fields: temperature while a game's ply < temp_decay_moves, temp_endgame after, constant `temperature`
 * when temp_decay_moves <= 0 (game.py:55-63); T <= 1e-6 plays the first most visited move, else the move
 * is drawn with probability N^(1/T) (player.py:362-371) from the device generator (stream of its own,
 * keyed by the engine's seed, the driver's ply counter and the game).  refill: a finished game restarts
 * at once in its slot; otherwise the slot is dead (action -1) from then on.  record: keep what
 * game.py:97-108 keeps per ply and move finished games to a store of max_finished_games games
 * (<= 0: max(4 n_envs, 1024)); games that end while it is full are dropped and counted.  noise_steps > 0:
 * epsilon of a game at ply p = eps_min + (eps_init - eps_min) * max(0, 1 - p / noise_steps), in double and
 * rounded once (game.py:87-91) - the two are doubles because the reference's are Python floats. */
typedef struct az_selfplay_config {
    float   temperature;
    float   temp_endgame;
    int32_t temp_decay_moves;
    int32_t refill;
    int32_t record;
    int32_t noise_steps;
    int64_t max_finished_games;
    double  noise_eps_init;
    double  noise_eps_min;
} az_selfplay_config;
#define AZ_SELFPLAY_CONFIG_BYTES 48
#ifdef __cplusplus
static_assert(sizeof(az_selfplay_config) == AZ_SELFPLAY_CONFIG_BYTES, "az_selfplay_config layout");
#else
_Static_assert(sizeof(az_selfplay_config) == AZ_SELFPLAY_CONFIG_BYTES, "az_selfplay_config layout");
#endif

typedef struct az_selfplay az_selfplay;

/* Every game at its initial position, ply 0, every tree of the engine reset (synchronises). */
int  az_selfplay_create(az_mcts *m, const az_selfplay_config *c, az_selfplay **out);
void az_selfplay_destroy(az_selfplay *sp);
/* n_plies whole plies on `stream`: per ply az_mcts_dev_set_roots, az_mcts_dev_search(model, n_playout, K,
 * use_table), then the tail above and az_mcts_dev_check.  Nothing but enqueues unless the engine's buffers
 * must grow; the host runs at most one ply ahead of the device (it waits for the event behind the ply
 * before the previous one, never for the device).  AZ_ERR_CAPACITY as az_mcts_dev_check reports it. */
int az_selfplay_step(az_selfplay *sp, const struct az_nn_model *model, int n_playout, int K, int use_table,
                     int n_plies, void *stream);
/* The two halves of a ply on their own, for an evaluator that is not an az_nn_model: begin_ply puts the
 * positions into the engine as roots; the caller searches (az_mcts_dev_prepare_stream and the select /
 * backprop calls, or alphazero-al_amd/src/fused.py); finish_ply is everything after the search. */
int az_selfplay_begin_ply(az_selfplay *sp, void *stream);
int az_selfplay_finish_ply(az_selfplay *sp, void *stream);
/* Test hook - recorded moves instead of the sampler: actions int32 [n_plies][n_envs] in DEVICE memory, kept
 * alive by the caller; the p-th ply after this call plays actions[p] (-1: the slot does not move; no draw is
 * made).  Running past the tape is AZ_ERR_STATE, as with az_mcts_dev_replay.  NULL ends it. */
int az_selfplay_set_action_tape(az_selfplay *sp, const int32_t *actions, int64_t n_plies);
/* Running totals: [0] positions played [1] games finished [2] won by player +1 [3] by player -1 [4] drawn
 * (synchronises). */
int az_selfplay_totals(az_selfplay *sp, int64_t out[5]);
/* The games in progress, to HOST arrays of n_envs entries, any of them NULL (synchronises). */
int az_selfplay_positions(az_selfplay *sp, uint64_t *bb_p1, uint64_t *bb_p2, int32_t *turns, int32_t *ply);
/* What the finished store holds: games, trajectory rows (a game of L moves has L + 1: one per position
 * before a move, then the end state), and the games dropped since creation (synchronises). */
int az_selfplay_finished(az_selfplay *sp, int64_t *n_games, int64_t *n_rows, int64_t *n_dropped);
/* HOST arrays sized from az_selfplay_finished.  Game g: the slot it was played in, its moves, the winner
 * (+1 / -1 / 0), the driver ply it ended on, and its first row; rows row_start[g] .. row_start[g] + length[g]:
 * both bitboards and the side to move (end state included), and for the rows before the end the visit
 * distribution N / sum N (double division, rounded once: player.py:356), the root's [draw, p1, p2] and the
 * legal-move mask (zeros in the end-state row). */
typedef struct az_selfplay_games {
    int32_t  *slot, *length, *winner;      /* [n_games] */
    int64_t  *finish_ply, *row_start;      /* [n_games] */
    uint64_t *bb_p1, *bb_p2;               /* [n_rows] */
    int8_t   *turn;                        /* [n_rows] */
    float    *prob;                        /* [n_rows][A] */
    float    *wdl;                         /* [n_rows][3] */
    uint8_t  *mask;                        /* [n_rows][A] */
} az_selfplay_games;
/* Copies the store out in the order (finishing ply, slot) and empties it (synchronises); n_games and
 * n_rows must be what az_selfplay_finished just reported. */
int az_selfplay_drain(az_selfplay *sp, const az_selfplay_games *out, int64_t n_games, int64_t n_rows);

/* ---- finished games as replay-buffer rows, on the device (k_sp_export) -----------------------------------
 * The reference's learner keeps every position in dense tensors (src/ReplayBuffer.py:11-23) and fills them
 * row by row: `store` (ReplayBuffer.py:92-123) writes row number _ptr to index _ptr % capacity, and a game
 * arrives as the tuples of src/game.py:110-157.  az_replay_tensors names such tensors in DEVICE memory, all
 * contiguous and 16-byte aligned, `capacity` rows each; A = 7 and R x C = 6 x 7 (Connect4), A = 65 and 8 x 8
 * (Othello).  A game of T moves is T + 1 rows; row t (0 <= t <= T, t = T the end state) holds
 *   state            the position as three planes: stones of the side to move, stones of the opponent, the
 *                    turn sign (+1 / -1) in every cell; Connect4: cell (r, c) is bit 7 c + (5 - r) of a
 *                    bitboard (row 0 is the top), Othello: bit 8 r + c
 *   prob             t < T: the visit distribution of the row; end state: zeros
 *   winner           the game's winner (+1 / -1 / 0) in every row
 *   steps_to_end     T - t
 *   aux_target       Connect4: T - t.  Othello: (discs of player +1 - discs of player -1 in the END state)
 *                    x the side to move of row t
 *   root_wdl         t < T: the root's [draw, p1, p2] of the row; end state: zeros
 *   valid_mask       t < T: the legal-move mask of the row (bytes 0 / 1); end state: all ones
 *   future_root_wdl  root_wdl of row t + td_steps of the same game if td_steps > 0 and t + td_steps < T,
 *                    zeros otherwise
 * Floats are copied bit for bit.  Row number r of a call (its games in order, rows in order) goes to index
 * (ptr + r) % capacity; of a call that carries more rows than `capacity` only the last `capacity` rows are
 * written, which is what storing them one by one would leave. */
typedef struct az_replay_tensors {
    int8_t  *state;             /* [capacity][3][R][C] */
    float   *prob;              /* [capacity][A] */
    int8_t  *winner;            /* [capacity] */
    int16_t *steps_to_end;      /* [capacity] */
    int16_t *aux_target;        /* [capacity] */
    float   *root_wdl;          /* [capacity][3] */
    uint8_t *valid_mask;        /* [capacity][A], one byte per entry */
    float   *future_root_wdl;   /* [capacity][3] */
    int64_t  capacity;
} az_replay_tensors;
#define AZ_REPLAY_TENSORS_BYTES 72
#ifdef __cplusplus
static_assert(sizeof(az_replay_tensors) == AZ_REPLAY_TENSORS_BYTES, "az_replay_tensors layout");
#else
_Static_assert(sizeof(az_replay_tensors) == AZ_REPLAY_TENSORS_BYTES, "az_replay_tensors layout");
#endif
/* HOST arrays of n_games entries each, filled in export order, any of them NULL: what a caller's statistics
 * need of the exported games (server.py:304 keeps the episode lengths). */
typedef struct az_selfplay_export_info {
    int32_t *slot, *length, *winner;
    int64_t *finish_ply;
} az_selfplay_export_info;
/* Moves the whole finished store into `dst` as rows ptr .. ptr + n_rows - 1, the games in az_selfplay_drain's
 * order (finishing ply, then slot), and empties the store as az_selfplay_drain does; *new_ptr = ptr + n_rows
 * (new_ptr may be NULL).  n_games and n_rows must be what az_selfplay_finished just reported, ptr >= 0,
 * 0 <= td_steps.  Only the per-game figures (slot, length, winner, finishing ply, first row) cross to the host,
 * which sorts them and hands the kernel the games' source and destination rows; the rows themselves never leave
 * the device.  The call waits for the device before it reads those figures, then ONLY enqueues on `stream`: the
 * kernel, and behind it the reset of the store's counters - so an az_selfplay_step issued after it on the same
 * stream is correct without a wait in between, and `dst` is complete once `stream` reaches that point.
 * `info` is optional.  AZ_ERR_ARG: the driver does not record, sizes differ from what az_selfplay_finished
 * reported, capacity <= 0, a null or misaligned tensor. */
int az_selfplay_export(az_selfplay *sp, const az_replay_tensors *dst, int64_t ptr, int td_steps, int64_t n_games,
                       int64_t n_rows, const az_selfplay_export_info *info, int64_t *new_ptr, void *stream);
/* The same kernel on packed games a caller keeps itself, every array in DEVICE memory: of `games_dev` the
 * fields length, winner, bb_p1, bb_p2, turn, prob, wdl and mask are read (laid out as az_selfplay_drain fills
 * them); game g occupies the source rows src_row0[g] .. src_row0[g] + length[g] and becomes the call's rows
 * dst_row0[g] .. dst_row0[g] + length[g].  dst_row0 starts at 0 and is packed in game order (dst_row0[g + 1] =
 * dst_row0[g] + length[g] + 1): the kernel takes the call's row count from its last entry.  Only enqueues. */
int az_replay_dev_store(int game, const az_selfplay_games *games_dev, const int64_t *src_row0, const int64_t *dst_row0,
                        int64_t n_games, const az_replay_tensors *dst, int64_t ptr, int td_steps, void *stream);
/* k_sp_pick on caller-supplied counts, for tests: counts int32 [n][A] and ply int32 [n] in DEVICE memory
 * -> actions int32 [n]; draws are keyed by (seed, call, row).  Only the temperature fields of `c` are read. */
int az_selfplay_sample(int game, const int32_t *counts, const int32_t *ply, const az_selfplay_config *c,
                       uint64_t seed, uint64_t call, int32_t *actions, int64_t n, void *stream);

/* ---- teams in the self-play driver ----------------------------------------------------------------------------
 * The reference's self-play player may search SEVERAL trees of one root (AlphaZeroPlayer.get_action /
 * _get_action_sym_ensemble with is_selfplay = 1, src/player.py:248-329): root-parallel play (n_trees = K) and the
 * symmetry ensemble (one tree per board symmetry of the game).  Every tree of the team searches the same root, the
 * move and the recorded policy target come from the summed visit counts, and every tree is re-rooted with the move
 * mapped into its own frame, so each keeps its subtree.  az_selfplay_create_teams gives every game `trees` trees:
 * tree j of game g is the engine's tree g * trees + j (the match driver's rule, see az_match_create_teams below), so
 * n_games = n_envs / trees.  In an ensemble (trees = az_game_num_augment(game)) tree j works in the frame of the
 * game's j-th symmetry - Connect4: identity, column mirror; Othello: the reference's ids 0, 2, 6, 7 - and the
 * engine's own random symmetry should be off (player.py:177-180: use_symmetry = 0 in its az_search_config).  A ply:
 *   roots    every tree of a game gets the game's position, ensemble tree j under symmetry j;
 *   move     summed[a] = sum over j of counts[tree j][perm_j(a)] (perm_j the identity without an ensemble; the
 *            pass stays; every perm is an involution); k_sp_pick's rule runs on that row, its draws keyed by (the
 *            engine's seed, the driver's ply counter, the GAME) - with one tree they are az_selfplay_create's;
 *   record   the position (the game's frame), prob = summed / its total, the legal mask of the game's position, and
 *            the team's merged root [draw, p1, p2]: elements 3..5 of az_mcts_dev_team_root_stats, bit for bit;
 *   re-root  every tree with the move in its own frame; a dead slot or a tape entry of -1 gives -1 to every tree;
 *   reset    every tree of a game that ended; with noise_steps > 0 every tree of a game gets the game's epsilon.
 * The tail has as many launches as a single-tree ply's, none of which grows with `trees`.  Trees of one game
 * diverge only through what the engine's generator gives each TREE (root noise, symmetry ids) or, in an ensemble,
 * through the frames.  Every per-game quantity of the calls above has n_games entries: az_selfplay_positions, the
 * rows of the action tape, `slot` of finished games; totals[0] counts n_games positions per ply; the default store
 * holds max(4 n_games, 1024) games.  The begin / finish route covers all trees: the caller of az_selfplay_begin_ply
 * searches the whole engine.  az_selfplay_create is az_selfplay_create_teams with {1, 0}. */
typedef struct az_selfplay_teams {
    int32_t trees;       /* trees per game, >= 1 */
    int32_t ensemble;    /* != 0: a game's trees are its symmetry ensemble */
} az_selfplay_teams;
#define AZ_SELFPLAY_TEAMS_BYTES 8
#ifdef __cplusplus
static_assert(sizeof(az_selfplay_teams) == AZ_SELFPLAY_TEAMS_BYTES, "az_selfplay_teams layout");
#else
_Static_assert(sizeof(az_selfplay_teams) == AZ_SELFPLAY_TEAMS_BYTES, "az_selfplay_teams layout");
#endif
/* AZ_ERR_ARG: a null argument, trees < 1, an n_envs that is no multiple of trees, an ensemble whose tree count is
 * not az_game_num_augment(game). */
int az_selfplay_create_teams(az_mcts *m, const az_selfplay_config *c, const az_selfplay_teams *t, az_selfplay **out);
/* The team pick on caller-supplied counts, for tests - az_selfplay_sample's contract with the team in front: counts
 * int32 [n * trees][A] and ply int32 [n] in DEVICE memory -> summed int32 [n][A] (may be NULL), actions int32 [n] in
 * the game's frame, tree_actions int32 [n * trees] in each tree's frame (may be NULL); draws are keyed by (seed, call,
 * game).  With trees = 1 and ensemble = 0 the actions are az_selfplay_sample's.  Only enqueues.  AZ_ERR_ARG: an
 * unknown game, a null pointer that may not be, trees < 1, an ensemble whose tree count is not az_game_num_augment. */
int az_selfplay_team_sample(int game, const int32_t *counts, const int32_t *ply, const az_selfplay_config *c, int trees,
                            int ensemble, uint64_t seed, uint64_t call, int32_t *summed, int32_t *actions,
                            int32_t *tree_actions, int64_t n, void *stream);
/* A team's root statistics merged into the game's frame (k_team_root_stats): what the reference's inverse_sym_stats
 * (src/symmetry.py:140-186) returns for trees j = 0 .. trees - 1, with the game's ensemble symmetries for an ensemble
 * and the identity for a root-parallel team.  stats float32 [n * trees][6 + 8A] as az_mcts_dev_root_stats writes them
 * (head root_N, root_Q, root_M, root_D, root_P1W, root_P2W, then per action N, Q, prior, noise, M, D, P1W, P2W) ->
 * merged float32 [n][6 + 8A], both in DEVICE memory.  All arithmetic is float32, every product and sum rounded on its
 * own, every sum in tree order from tree 0: head and prior / noise are sum / trees, N is the sum, Q, M, D, P1W and P2W
 * are sum_j(x_j N_j) / sum_j(N_j) where the denominator is > 0, else 0.  numpy sums fewer than 8 float32 values in
 * that order and pairwise from 8 on: from 8 trees on the merged means may differ from numpy's in the last bit.
 * Only enqueues.  AZ_ERR_ARG as az_selfplay_team_sample. */
int az_mcts_dev_team_root_stats(int game, const float *stats, int trees, int ensemble, float *merged, int64_t n,
                                void *stream);

/* ---- evaluation matches between two networks (alphazero-al_amd/csrc/match_kernels.hip) ---------------------
 * The reference's gate plays n games between two players in lock step (src/pipeline.py:264-335,
 * `_batched_eval_games`): two BatchedMCTS objects over the same games (pipeline.py:280-293), the side to move
 * searches in its own (pipeline.py:306-318), the move comes from its visit counts (pipeline.py:337-351) and BOTH
 * objects are re-rooted with it (pipeline.py:323-324), so each player keeps its subtree across the opponent's
 * reply.  Here a match object borrows TWO engines - engine_p1 holds the trees of the player who is +1, engine_p2
 * those of -1; same game, same n_envs, same device - and owns the positions, per-game ply counters, dead flags,
 * results and an optional move record in HBM.  A ply outside the search is: the mover engine's root counts,
 * k_match_ply (the move, the game step, done / winner / length / dead flag, the move record, the totals - ONE
 * launch), the re-rooting of both engines with the same actions, the reset of both engines' trees of the games that
 * ended.  Search parameters (c_init, c_base, alpha, noise epsilon, symmetry, ...) stay in each engine's own
 * az_search_config: the two players may differ.  Destroy the match BEFORE the engines; make every call of a match on
 * ONE stream and from one thread at a time.
 *
 * Every game has the same side to move and turns alternate strictly (Othello's pass is action 64), so one engine
 * searches per ply.  A finished game is dead from then on: action -1 to both engines (their trees of that game stay
 * reset), no further row in the move record - like a self-play slot with refill = 0.  The reference goes on searching
 * finished games and discards the move (pipeline.py:306-318 search every env).
 *
 * temperature: T <= 1e-6 plays the first most visited move, else the move is drawn with probability N^(1/T)
 * (pipeline.py:337-351, the rule of player.py:362-371) - the pick of k_sp_pick, shared.  Draws come from the device
 * generator on a stream of its own (MATCH_STREAM in dev_rng.h, not the self-play driver's), keyed by (the seed of
 * engine_p1, the match's ply counter, the game): az_selfplay_sample does NOT reproduce them, az_match_sample does.
 * The reference's two objects draw noise and symmetry ids from ONE thread-local mt19937 (MCTS.h:13-17); here each
 * engine has its own device generator stream.
 *
 * Teams.  The reference's strongest players search SEVERAL trees of one root and choose the move from the summed
 * visit counts: root-parallel play (AlphaZeroPlayer / MCTSPlayer with n_trees = K, src/player.py:73-103, 248-283) and
 * the symmetry ensemble (sym_ensemble, player.py:285-329 with src/symmetry.py: one tree per board symmetry of the
 * game).  az_match_create_teams gives each player `trees` trees per game: tree j of game g is tree g * trees + j of
 * that player's engine, so n_games = n_envs(engine) / trees and the two engines may differ in n_envs.  In an ensemble
 * team (trees = az_game_num_augment(game)) tree j works in the frame of the game's j-th symmetry - Connect4:
 * identity, column mirror; Othello: the reference's ids 0, 2, 6, 7; the order of az_replay_dev_batch - and the
 * engine's own random symmetry should be off (player.py:177-180: use_symmetry = 0 in its az_search_config).  A ply:
 *   roots    every tree of the mover's team gets the game's position, ensemble tree j under symmetry j (both
 *            bitboards transformed, the side to move as it is);
 *   move     the team's count rows become one row per game, summed[a] = sum over j of counts[tree j][perm_j(a)]
 *            (perm_j the identity without an ensemble; the pass stays; every perm is an involution), and the pick
 *            above runs on that row, its draws keyed by (seed of engine_p1, ply, GAME).  The move record, winner,
 *            length and totals are per game and in the game's frame;
 *   re-root  BOTH engines, every tree with the move mapped into its own frame (player.py:321-324); every tree of a
 *            finished or dead game gets action -1 and is reset, as a single tree is.
 * Trees of one game diverge through what the engine's generator gives each TREE (root noise, symmetry ids, random
 * playouts) or, in an ensemble, through the frames.  All per-game arrays of the calls below (set_positions, results,
 * moves, remaining, the action tape) have n_games entries; fresh_trees and the begin / finish route cover all trees
 * of the side (the caller of begin_ply searches the mover's engine over all its trees). */
typedef struct az_match_config {
    float   temperature;
    int32_t record_moves;
} az_match_config;
#define AZ_MATCH_CONFIG_BYTES 8
#ifdef __cplusplus
static_assert(sizeof(az_match_config) == AZ_MATCH_CONFIG_BYTES, "az_match_config layout");
#else
_Static_assert(sizeof(az_match_config) == AZ_MATCH_CONFIG_BYTES, "az_match_config layout");
#endif

typedef struct az_match_teams {
    int32_t trees_p1, trees_p2;          /* trees per game of player +1 / -1, >= 1 */
    int32_t ensemble_p1, ensemble_p2;    /* != 0: that player's trees are the game's symmetry ensemble */
} az_match_teams;
#define AZ_MATCH_TEAMS_BYTES 16
#ifdef __cplusplus
static_assert(sizeof(az_match_teams) == AZ_MATCH_TEAMS_BYTES, "az_match_teams layout");
#else
_Static_assert(sizeof(az_match_teams) == AZ_MATCH_TEAMS_BYTES, "az_match_teams layout");
#endif

typedef struct az_match az_match;

/* Every game at its initial position with player +1 to move, ply 0, every tree of both engines reset
 * (synchronises).  AZ_ERR_ARG: the engines differ in game, n_envs or device, or are one and the same.
 * az_match_create_teams with {1, 1, 0, 0}. */
int  az_match_create(az_mcts *engine_p1, az_mcts *engine_p2, const az_match_config *c, az_match **out);
/* The same with a team of trees per player and game (see above): n_games = n_envs(engine_p1) / trees_p1 =
 * n_envs(engine_p2) / trees_p2.  AZ_ERR_ARG besides az_match_create's: a null argument, a tree count below 1, an
 * n_envs that is no multiple of its tree count, unequal game counts, an ensemble whose tree count is not
 * az_game_num_augment(game). */
int  az_match_create_teams(az_mcts *engine_p1, az_mcts *engine_p2, const az_match_config *c, const az_match_teams *t,
                           az_match **out);
void az_match_destroy(az_match *mt);
/* Start positions from HOST arrays of n_games entries (an opening suite; deterministic tests); before the first ply
 * only (AZ_ERR_ARG after it).  Every game must have the same side to move (AZ_ERR_ARG otherwise).  Both engines'
 * trees of every game are reset; a position that is already over counts as finished at ply 0 with its winner and
 * length 0.  Connect4's last mover and Othello's pass count are derived as an import derives them.  Synchronises. */
int az_match_set_positions(az_match *mt, const uint64_t *bb_p1, const uint64_t *bb_p2, const int32_t *turns);
/* n_plies whole plies on `stream`: per ply az_mcts_dev_set_roots into the mover's engine, az_mcts_dev_search on it
 * with the mover's model (model_p1 when +1 moves), its root counts, k_match_ply, az_mcts_dev_prune_roots of BOTH
 * engines, az_mcts_dev_reset_masked of BOTH, az_mcts_dev_check of both.  Nothing but enqueues unless an engine's
 * buffers must grow; the host runs at most one ply ahead of the device.  Once every game is over (as
 * az_match_remaining last saw it, or as the newest completed ply reported) or the game's ply bound is reached, the
 * remaining plies are not played: the call changes nothing.  AZ_ERR_ARG: a null model. */
int az_match_step(az_match *mt, const struct az_nn_model *model_p1, const struct az_nn_model *model_p2, int n_playout,
                  int K, int use_table, int n_plies, void *stream);
/* az_match_step with players of either kind: a NULL model makes that side the rollout player (searched with
 * az_mcts_dev_rollout_search, n_playout_pX simulations; K and use_table apply to network sides only).
 * fresh_trees: bit 0 player +1, bit 1 player -1 - that player's engine starts every one of its searches from
 * empty trees (game.py:41, player.py:102,279-281) instead of the subtree kept by the re-rooting; the reset is
 * enqueued in front of the search (az_mcts_dev_reset_masked with a mask of ones that the match owns).
 * AZ_ERR_ARG: a null match, a negative count. */
int az_match_step_players(az_match *mt, const struct az_nn_model *model_p1, const struct az_nn_model *model_p2,
                          int n_playout_p1, int n_playout_p2, int K, int use_table, int fresh_trees,
                          int n_plies, void *stream);
/* The two halves of a ply, for an evaluator that is not an az_nn_model: begin_ply puts the positions into the
 * mover's engine as roots and reports the mover (+1: search engine_p1, -1: engine_p2; 0: the match is over, nothing
 * was done and finish_ply will do nothing); the caller searches that engine (az_mcts_dev_prepare_stream and the
 * select / backprop calls, or alphazero-al_amd/src/fused.py); finish_ply is everything after the search. */
int az_match_begin_ply(az_match *mt, void *stream, int *mover);
int az_match_finish_ply(az_match *mt, void *stream);
/* Test hook - recorded moves instead of the pick, the contract of az_selfplay_set_action_tape: actions int32
 * [n_plies][n_envs] in DEVICE memory, kept alive by the caller; the p-th ply after this call plays actions[p]
 * (-1: the game does not move).  Running past the tape is AZ_ERR_STATE.  NULL ends it. */
int az_match_set_action_tape(az_match *mt, const int32_t *actions, int64_t n_plies);
/* Games still running (synchronises). */
int az_match_remaining(az_match *mt, int64_t *n);
/* HOST arrays, any of them NULL (synchronises): winner[n_envs] +1 / -1 / 0 (0 while the game is running),
 * length[n_envs] plies played so far, totals = won by +1, won by -1, drawn, still running. */
int az_match_results(az_match *mt, int32_t *winner, int32_t *length, int64_t totals[4]);
/* With record_moves: the [max_plies][n_envs] actions played, -1 where the game had ended (or the ply has not been
 * played); max_plies = az_match_max_plies: 42 for Connect4, 126 for Othello.  HOST array (synchronises). */
int az_match_moves(az_match *mt, int32_t *actions);
int az_match_max_plies(const az_match *mt);
/* k_match_ply's pick on caller-supplied counts, for tests: counts int32 [n][A] in DEVICE memory -> actions int32 [n];
 * draws are keyed by (seed, ply, row) on the match's generator stream - with seed = what az_mcts_set_seed(s >= 0)
 * leaves in engine_p1, (uint32) s * 0x9E3779B97F4A7C15 + 1, and ply = the match's ply counter it reproduces a
 * match's draws. */
int az_match_sample(int game, const int32_t *counts, float temperature, uint64_t seed, uint64_t ply, int32_t *actions,
                    int64_t n, void *stream);
/* The team forms, for tests; both only enqueue, every pointer is DEVICE memory.
 * az_match_team_roots: positions [n] -> a team's roots [n * trees], tree j of game g at g * trees + j, symmetrised
 * for an ensemble - what a team match puts into the mover's engine.
 * az_match_team_sample: counts [n * trees][A] -> summed [n][A] (may be NULL), actions [n] in the game's frame (the
 * pick of az_match_sample on the summed row, draws keyed by (seed, ply, game)) and tree_actions [n * out_trees], the
 * move in the frames of a team of out_trees trees (out_ensemble as above; may be NULL).  With trees = 1 and
 * ensemble = 0 the actions are az_match_sample's.  AZ_ERR_ARG: an unknown game, a null pointer that may not be, a tree
 * count below 1, an ensemble whose tree count is not az_game_num_augment(game). */
int az_match_team_roots(int game, const uint64_t *bb_p1, const uint64_t *bb_p2, const int32_t *turns, int trees,
                        int ensemble, uint64_t *out_bb_p1, uint64_t *out_bb_p2, int32_t *out_turns, int64_t n,
                        void *stream);
int az_match_team_sample(int game, const int32_t *counts, int trees, int ensemble, float temperature, uint64_t seed,
                         uint64_t ply, int32_t *summed, int32_t *actions, int out_trees, int out_ensemble,
                         int32_t *tree_actions, int64_t n, void *stream);

/* ---- augmented training batches out of the replay tensors, on the device (k_replay_batch) ----------------
 * The reference's learner draws a sample on the host (src/ReplayBuffer.py:130-145: np.random.randint, `get`, a
 * TensorDataset behind a shuffling DataLoader that collates sample by sample) and passes every batch through the
 * game's `augment` (src/environments/Connect4/utils.py:50-67, src/environments/Othello/utils.py:65-91).  Here a
 * batch is one launch: B ring rows named by index become S * B rows, S = az_game_num_augment(game), laid out
 * symmetry-major - output row s * B + b is sample b under symmetry s, which is what `augment(get(idx))` returns.
 *   Connect4, S = 2   identity; the column mirror c -> 6 - c (action a -> 6 - a)
 *   Othello,  S = 4   identity; (r, c) -> (7 - r, 7 - c); (r, c) -> (c, r); (r, c) -> (7 - c, 7 - r) - the
 *                     reference's ids 0, 2, 6, 7; the pass (action 64) stays in place
 * state: the int8 planes as float32, planes 0 and 1 permuted, plane 2 (the turn sign) as it is.  prob and
 * valid_mask: the board actions permuted the same way, floats bit for bit, mask bytes 0 / 1.  winner,
 * steps_to_end, aux_target, root_wdl, future_root_wdl: repeated S times bit for bit.  az_replay_batch names the
 * batch's tensors in DEVICE memory, all contiguous and 16-byte aligned, S * B rows each. */
typedef struct az_replay_batch {
    float   *state;             /* [S*B][3][R][C] */
    float   *prob;              /* [S*B][A] */
    int8_t  *winner;            /* [S*B] */
    int16_t *steps_to_end;      /* [S*B] */
    int16_t *aux_target;        /* [S*B] */
    float   *root_wdl;          /* [S*B][3] */
    uint8_t *valid_mask;        /* [S*B][A], one byte per entry */
    float   *future_root_wdl;   /* [S*B][3] */
} az_replay_batch;
#define AZ_REPLAY_BATCH_BYTES 64
#ifdef __cplusplus
static_assert(sizeof(az_replay_batch) == AZ_REPLAY_BATCH_BYTES, "az_replay_batch layout");
#else
_Static_assert(sizeof(az_replay_batch) == AZ_REPLAY_BATCH_BYTES, "az_replay_batch layout");
#endif
/* Board symmetries a batch is augmented with: 2 (Connect4), 4 (Othello); -1 for an unknown game. */
int az_game_num_augment(int game);
/* Sample b (0 <= b < B) of the batch is the ring row idx[order ? order[first + b] : first + b]: `idx` is a sample
 * (int64, DEVICE memory) and `order`, optional, a permutation of its positions (int64, DEVICE memory) - an epoch's
 * shuffle needs no gather pass of its own, a batch is a window [first, first + B) of it.  The caller keeps first + B
 * within the arrays and the entries of `order` within `idx`.  A ring row outside [0, capacity) is never read: it
 * gives all-zero output rows in every tensor (the kernel cannot report to the host without a wait).  Replaces
 * ReplayBuffer.py:144-145 (dataset, loader, per-sample collation) and the `augment` call of the training step.
 * Only enqueues on `stream`.  AZ_ERR_ARG: unknown game, B <= 0 (or beyond 2^30), first < 0, capacity <= 0, a null
 * or misaligned tensor (both structs: 16 bytes), a null `src`, `idx` or `out`. */
int az_replay_dev_batch(int game, const az_replay_tensors *src, const int64_t *idx, const int64_t *order, int64_t first,
                        int64_t B, const az_replay_batch *out, void *stream);
/* n ring indices uniform in [0, n_valid) into idx (int64 [n], DEVICE memory), element e from the device
 * generator's stream (seed, call, e): the same (seed, call) gives the same indices whatever n is, another `call`
 * gives others.  Each is the high half of a 64-bit draw times n_valid, so the bias is below n_valid / 2^64.
 * Replaces np.random.randint(0, len(buffer), sample_size) of ReplayBuffer.py:142.  Only enqueues on `stream`.
 * AZ_ERR_ARG: n_valid <= 0, n < 0, a null idx with n > 0. */
int az_replay_dev_sample_indices(uint64_t seed, uint64_t call, int64_t n_valid, int64_t *idx, int64_t n, void *stream);

/* ---- device transposition table of evaluator outputs (both games) ------------------------
 * Replaces, for the device loop, the LRU table of the reference's wrapper (src/Cache.py:5-58 used
 * by src/MCTS_cpp.py:146-189 and 298-339): key = the symmetrised leaf position + side to move,
 * value = policy[A], relative wdl[3], auxiliary value.  2^log2_entries entries of 64 bytes (Connect4)
 * or 320 bytes (Othello), buckets of four, approximate-LRU replacement inside a bucket.  Between az_mcts_dev_select and
 * az_mcts_dev_backprop of one iteration:
 *   az_mcts_dev_tt_lookup   hits: the cached values are written to probs / wdl_rel / moves_left
 *                           at the leaf's flat index; misses: their flat indices are appended to
 *                           miss_idx[0 .. *miss_count) (int32 [n*K] and int64 [1], DEVICE memory;
 *                           the count is reset first).  Terminal leaves are neither.
 *   (evaluate the rows listed in miss_idx, writing the same three arrays - az_nn.h `batch_dev`)
 *   az_mcts_dev_tt_insert   stores the freshly evaluated rows.
 * A lookup never returns a value that was not inserted for exactly its key (torn entries fail a
 * checksum and read as misses).  When the evaluator's weights change the cached outputs are stale:
 * az_mcts_dev_tt_refresh re-evaluates them in place as the reference's `refresh_cache` does
 * (MCTS_cpp.py:361-377; both games), az_mcts_dev_tt_clear empties the table.
 * Statistics (synchronises): lookups, hits, inserts, entries replaced. */
int az_mcts_dev_tt_create(az_mcts *m, int log2_entries);
int az_mcts_dev_tt_clear(az_mcts *m, void *stream);
int az_mcts_dev_tt_lookup(az_mcts *m, int K, float *probs, float *wdl_rel, float *moves_left, int32_t *miss_idx,
                          int64_t *miss_count, void *stream);
int az_mcts_dev_tt_insert(az_mcts *m, int K, const int32_t *miss_idx, const int64_t *miss_count, const float *probs,
                          const float *wdl_rel, const float *moves_left, void *stream);
/* refresh_cache (MCTS_cpp.py:361-377): after a weight update every resident key is evaluated
 * again with `model` (include/az_nn.h) and keeps its place and age; entries that do not decode to
 * a position are emptied.  Enqueued on `stream` in chunks of 16384 entries. */
int az_mcts_dev_tt_refresh(az_mcts *m, const struct az_nn_model *model, void *stream);
int az_mcts_dev_tt_stats(az_mcts *m, int64_t out[4]);

/* ---- capacity / instrumentation ------------------------------------------------------- */

/* Tree arenas.  Every tree owns two halves of `capacity` node records and lives in one of them; a re-rooting
 * (prune_roots) copies the subtree it keeps into the other half when the tree could not take two more
 * searches' worth of growth where it is (the reference never reclaims a node before the next reset,
 * MCTS.h:90-108; node numbering is not observable).  az_mcts_reserve makes every half hold at least
 * `slots_per_tree` records (grows, never shrinks; synchronises); the engine grows by itself when a tree needs
 * more.  az_mcts_capacity: records per half. */
int az_mcts_reserve(az_mcts *m, int64_t slots_per_tree);
int64_t az_mcts_capacity(const az_mcts *m);
/* Changes whenever any device buffer the dev_* kernels address was reallocated (arena growth,
 * wider K, new c_puct table): a captured hipGraph of dev_* calls is valid for one epoch. */
int64_t az_mcts_epoch(const az_mcts *m);
/* Largest number of node records any tree uses right now (synchronises). */
int az_mcts_max_used(az_mcts *m, int64_t *out);

/* Workload counters since creation / last reset (synchronises):
 * [0] simulations [1] select levels [2] expansions [3] terminal leaves [4] duplicate VL
 * leaves [5] nodes updated by backup [6] select launches [7] backprop launches */
#define AZ_NUM_COUNTERS 8
int az_mcts_counters(az_mcts *m, int64_t out[AZ_NUM_COUNTERS]);
int az_mcts_counters_reset(az_mcts *m);

/* Kernel timing with HIP events recorded on the launch stream around every selection and every
 * expansion/backup kernel issued by the dev_* entry points (bench.py's roofline figures).
 * enable != 0 starts recording (at most AZ_PROFILE_MAX launches per kind are kept between
 * reads); enable = n > 1 times every n-th launch of a kind only (an event pair costs the stream
 * ~5 us, which a bench does not want around every launch); az_mcts_profile_read synchronises and returns, for [0] selection and [1]
 * expansion/backup, the summed kernel time in ms and the number of launches summed. */
#define AZ_PROFILE_MAX 8192
int az_mcts_profile(az_mcts *m, int enable);
int az_mcts_profile_read(az_mcts *m, double out_ms[2], int64_t out_launches[2]);
/* Name of the kernel behind the newest TIMED selection launch ("" before the first one): what the
 * engine launched, not what an environment knob asked for (static string, never NULL). */
const char *az_mcts_timed_select_kernel(az_mcts *m);

/* Test hook for the host generator: `count` Dirichlet-gamma draws from one fresh
 * gamma(alpha,1) object on an mt19937 seeded with `seed` (checked against libstdc++). */
int az_rng_gamma_selftest(uint32_t seed, float alpha, int count, float *out);

#ifdef __cplusplus
}
#endif
#endif
