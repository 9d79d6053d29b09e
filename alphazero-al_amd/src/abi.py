"""The C ABI of lib/libaz_mcts.so as ctypes sees it: the one place that loads the library, mirrors the structs of
include/az_mcts.h, include/az_nn.h and include/az_train.h and states every function's prototype.  A declaration file, not
a layer: callers take the library object from `lib()` and call `L.az_*` themselves.  `PROTOTYPES` lists the functions in
header order, one line each, as (name, restype, argtypes): handles, device and host buffer pointers and streams are
c_void_p, a struct parameter is POINTER(<its mirror>); `MIRRORS` names the mirror of every typedef.
tests/test_abi_cpu.py holds both tables and the mirrors' layouts to the headers."""
import ctypes as C
import os

import torch


class SearchConfig(C.Structure):
    """az_search_config (include/az_mcts.h)."""
    _fields_ = [(n, C.c_float) for n in ("c_init", "c_base", "dirichlet_alpha", "noise_epsilon", "fpu_reduction", "mlh_slope",
                                         "mlh_cap", "score_utility_factor", "score_scale", "value_decay")] + \
               [("use_symmetry", C.c_uint8), ("vl_count", C.c_int32)]


class SelfPlayConfig(C.Structure):
    """az_selfplay_config (include/az_mcts.h)."""
    _fields_ = [("temperature", C.c_float), ("temp_endgame", C.c_float), ("temp_decay_moves", C.c_int32),
                ("refill", C.c_int32), ("record", C.c_int32), ("noise_steps", C.c_int32),
                ("max_finished_games", C.c_int64), ("noise_eps_init", C.c_double), ("noise_eps_min", C.c_double)]


class SelfPlayGames(C.Structure):
    """az_selfplay_games (include/az_mcts.h): host arrays az_selfplay_drain fills."""
    _fields_ = [(n, C.c_void_p) for n in ("slot", "length", "winner", "finish_ply", "row_start", "bb_p1", "bb_p2",
                                          "turn", "prob", "wdl", "mask")]


class ReplayTensorsC(C.Structure):
    """az_replay_tensors (include/az_mcts.h): device pointers of a replay buffer's tensors and its capacity."""
    _fields_ = [(n, C.c_void_p) for n in ("state", "prob", "winner", "steps_to_end", "aux_target", "root_wdl",
                                          "valid_mask", "future_root_wdl")] + [("capacity", C.c_int64)]


class SelfPlayExportInfo(C.Structure):
    """az_selfplay_export_info (include/az_mcts.h): host arrays az_selfplay_export fills."""
    _fields_ = [(n, C.c_void_p) for n in ("slot", "length", "winner", "finish_ply")]


class MatchConfig(C.Structure):
    """az_match_config (include/az_mcts.h)."""
    _fields_ = [("temperature", C.c_float), ("record_moves", C.c_int32)]


class MatchTeams(C.Structure):
    """az_match_teams (include/az_mcts.h): trees per game and the ensemble flag of player +1 / -1.  Passed by address to a
    c_void_p parameter (C.byref), so it is no entry of `MIRRORS`; tests/test_team_cpu.py holds its layout to the header."""
    _fields_ = [(n, C.c_int32) for n in ("trees_p1", "trees_p2", "ensemble_p1", "ensemble_p2")]


class SelfPlayTeams(C.Structure):
    """az_selfplay_teams (include/az_mcts.h): trees per game and the ensemble flag of a self-play driver.  Passed by address
    to a c_void_p parameter (C.byref) like MatchTeams, so it is no entry of `MIRRORS`; tests/test_team_selfplay_cpu.py holds
    its layout to the header."""
    _fields_ = [("trees", C.c_int32), ("ensemble", C.c_int32)]


class ReplayBatchC(C.Structure):
    """az_replay_batch (include/az_mcts.h): device pointers of one augmented batch's tensors."""
    _fields_ = [(n, C.c_void_p) for n in ("state", "prob", "winner", "steps_to_end", "aux_target", "root_wdl",
                                          "valid_mask", "future_root_wdl")]


class Positions(C.Structure):
    """az_nn_positions of include/az_nn.h"""
    _fields_ = [(n, C.c_void_p) for n in ("bb_p1", "bb_p2", "turn", "sym")]


class HeadsWeights(C.Structure):
    """az_nn_heads_weights of include/az_nn.h"""
    _PTRS = ("p_norm", "p_gate_w", "p_fc_w", "p_fc_b", "p_out_w", "d_pool_norm", "d_pool_w", "d_pool_b", "d_norm",
             "d_fc_w", "d_fc_b", "d_out_norm", "d_val_w", "d_val_b", "d_aux_w")
    _fields_ = [(n, C.c_void_p) for n in _PTRS] + [(n, C.c_float) for n in ("p_gate_b", "p_out_b", "d_aux_b", "aux_scale")]


MAX_BLOCKS = 8          # AZ_NN_MAX_BLOCKS


class ModelWeights(C.Structure):
    """az_nn_model_weights of include/az_nn.h"""
    _fields_ = ([(n, C.c_void_p) for n in ("emb_own", "emb_opp", "pos", "stem_w", "stem_b")] + [("n_blocks", C.c_int32)] +
                [(n, C.c_void_p * MAX_BLOCKS) for n in ("block_w", "block_b", "block_gamma", "block_beta")] +
                [(n, C.c_void_p) for n in ("pre_w", "qkvg_w", "qn_w", "kn_w", "o_w")] +
                [("heads", HeadsWeights), ("eps", C.c_float), ("stem_frag", C.c_void_p), ("stem_pmap", C.c_void_p)])


class _HeadsW(C.Structure):          # az_nn_othello_heads_weights (include/az_nn.h)
    _PTRS = ("board_w", "pass_norm_w", "pass_fc_w", "v_conv_w", "v_bn_s", "v_bn_b", "v_fc_w", "v_fc_b", "a_fc_wt", "a_fc_b",
             "a_norm_w", "a_out_w")
    _fields_ = ([(n, C.c_void_p) for n in _PTRS] + [(n, C.c_float) for n in ("board_b", "pass_fc_b", "a_out_b", "aux_to_score", "eps")] +
                [("a_fc_w16", C.c_void_p)])


class _ConvLayer(C.Structure):       # az_nn_othello_conv_layer
    _fields_ = [(n, C.c_void_p) for n in ("w_packed", "pre_scale", "pre_shift", "post_scale", "post_shift")] + \
               [(n, C.c_int32) for n in ("residual", "c_in", "h_in", "pad")]


class _OthelloW(C.Structure):        # az_nn_othello_weights
    _fields_ = [("embed_table", C.c_void_p), ("n_body", C.c_int32), ("n_convs", C.c_int32), ("conv", _ConvLayer * 16),
                ("dual_w16", C.c_void_p), ("dual_scale16", C.c_void_p), ("dual_shift16", C.c_void_p), ("heads", _HeadsW)]


class TrainLossConfigC(C.Structure):
    """az_train_loss_config (include/az_train.h)."""
    _fields_ = [("value_decay", C.c_double), ("distill_alpha", C.c_double), ("distill_temp", C.c_double),
                ("psw_beta", C.c_double), ("entropy_lambda", C.c_double), ("td_alpha", C.c_double),
                ("td_steps", C.c_int32), ("reserved", C.c_int32), ("aux_target_offset", C.c_double)]


class TrainHeadsC(C.Structure):
    """az_train_heads (include/az_train.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("log_p", "value", "steps")]


class TrainLossOutC(C.Structure):
    """az_train_loss_out (include/az_train.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("losses", "counts", "workspace")]


class TrainGradsC(C.Structure):
    """az_train_grads (include/az_train.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("d_log_p", "d_value", "d_steps")]


class TrainBlockParamsC(C.Structure):
    """az_train_block_params (include/az_train.h).  Passed by address to a c_void_p parameter (C.byref) like MatchTeams, as
    are the two below, so none is an entry of `MIRRORS`; tests/test_train_block_cpu.py holds their layouts to the header."""
    _fields_ = [(n, C.c_void_p) for n in ("norm_weight", "norm_bias", "conv_weight", "conv_bias")]


class TrainBlockSavedC(C.Structure):
    """az_train_block_saved (include/az_train.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("z", "stats")]


class TrainBlockGradsC(C.Structure):
    """az_train_block_grads (include/az_train.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("dx", "d_norm_weight", "d_norm_bias", "d_conv_weight", "d_conv_bias", "workspace")] + \
               [("workspace_bytes", C.c_int64)]


class TrainAttnParamsC(C.Structure):
    """az_train_attn_params (include/az_train.h).  Bound like TrainBlockParamsC, as is the one below: passed by address to a
    c_void_p parameter (tests/test_abi_cpu.py fixes the number of `MIRRORS` entries); tests/test_train_attn_cpu.py holds their
    layouts to the header."""
    _fields_ = [(n, C.c_void_p) for n in ("prenorm_weight", "qkv_weight", "gate_weight", "o_weight", "q_norm_weight", "k_norm_weight")]


class TrainAttnGradsC(C.Structure):
    """az_train_attn_grads (include/az_train.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("dx", "d_prenorm_weight", "d_qkv_weight", "d_gate_weight", "d_o_weight", "d_q_norm_weight",
                                          "d_k_norm_weight", "workspace")] + [("workspace_bytes", C.c_int64)]


class TrainStemParamsC(C.Structure):
    """az_train_stem_params (include/az_train.h).  Bound like TrainBlockParamsC, as is the one below: passed by address to a
    c_void_p parameter; tests/test_train_stem_cpu.py holds their layouts to the header."""
    _fields_ = [(n, C.c_void_p) for n in ("piece_emb", "pos_emb", "conv_weight", "conv_bias")]


class TrainStemGradsC(C.Structure):
    """az_train_stem_grads (include/az_train.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("d_piece_emb", "d_pos_emb", "d_conv_weight", "d_conv_bias", "workspace")] + \
               [("workspace_bytes", C.c_int64)]


class TrainHeadsParamsC(C.Structure):
    """az_train_heads_params (include/az_train.h).  Bound like TrainBlockParamsC, as is the one below: passed by address to a
    c_void_p parameter; tests/test_train_heads_cpu.py holds their layouts to the header."""
    _NAMES = ("policy_norm_weight", "row_gate_weight", "row_gate_bias", "policy_fc_weight", "policy_fc_bias", "policy_out_weight",
              "policy_out_bias", "pool_norm_weight", "pool_fc_weight", "pool_fc_bias", "norm_weight", "fc_weight", "fc_bias",
              "out_norm_weight", "value_out_weight", "value_out_bias", "aux_out_weight", "aux_out_bias")
    _fields_ = [(n, C.c_void_p) for n in _NAMES]


class TrainHeadsGradsC(C.Structure):
    """az_train_heads_grads (include/az_train.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("d_tokens",) + tuple("d_" + n for n in TrainHeadsParamsC._NAMES) + ("workspace",)] + \
               [("workspace_bytes", C.c_int64)]


MIRRORS = {"az_search_config": SearchConfig, "az_selfplay_config": SelfPlayConfig, "az_selfplay_games": SelfPlayGames,
           "az_replay_tensors": ReplayTensorsC, "az_selfplay_export_info": SelfPlayExportInfo, "az_match_config": MatchConfig,
           "az_replay_batch": ReplayBatchC, "az_nn_positions": Positions, "az_nn_heads_weights": HeadsWeights,
           "az_nn_model_weights": ModelWeights, "az_nn_othello_heads_weights": _HeadsW, "az_nn_othello_conv_layer": _ConvLayer,
           "az_nn_othello_weights": _OthelloW, "az_train_loss_config": TrainLossConfigC, "az_train_heads": TrainHeadsC,
           "az_train_loss_out": TrainLossOutC, "az_train_grads": TrainGradsC}

P, vp, cstr, i32, i64, u32, u64, f32 = C.POINTER, C.c_void_p, C.c_char_p, C.c_int, C.c_int64, C.c_uint32, C.c_uint64, C.c_float

# The three az_train_block_*, the two az_train_attn_*, the two az_train_stem_* and the two az_train_heads_* struct parameters below are bound as plain c_void_p (their mirrors are no entries of `MIRRORS`,
# see TrainBlockParamsC), so tests/test_abi_cpu.py does NOT check their pointer types: tests/test_train_block_cpu.py,
# tests/test_train_attn_cpu.py, tests/test_train_stem_cpu.py and tests/test_train_heads_cpu.py hold the layouts instead.  A new struct belongs in `MIRRORS` with a POINTER(<mirror>) parameter, not here.
PROTOTYPES = (
    # include/az_mcts.h
    ("az_last_error", cstr, []),
    ("az_game_action_size", i32, [i32]),
    ("az_game_board_size", i32, [i32]),
    ("az_game_board_rows", i32, [i32]),
    ("az_game_board_cols", i32, [i32]),
    ("az_mcts_create", i32, [i32, i32, i32, P(vp)]),
    ("az_mcts_destroy", None, [vp]),
    ("az_mcts_config", P(SearchConfig), [vp]),
    ("az_mcts_num_envs", i32, [vp]),
    ("az_mcts_set_seed", i32, [vp, i32]),
    ("az_mcts_reset_env", i32, [vp, i32]),
    ("az_mcts_prune_roots", i32, [vp, vp, i64]),
    ("az_mcts_search_batch", i32, [vp, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp]),
    ("az_mcts_backprop_batch", i32, [vp, vp, vp, vp, vp, vp, vp, i64]),
    ("az_mcts_remove_all_vl", i32, [vp, i32]),
    ("az_mcts_search_batch_vl", i32, [vp, i32, vp, vp, i64, vp, vp, vp, vp, vp, vp, vp, vp]),
    ("az_mcts_backprop_batch_vl", i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, i64]),
    ("az_mcts_search_rollout", i32, [vp, vp, vp, i64, i32]),
    ("az_mcts_search_rollout_dev", i32, [vp, vp, vp, i64, i32]),
    ("az_mcts_get_all_counts", i32, [vp, vp]),
    ("az_mcts_get_all_root_stats", i32, [vp, vp]),
    ("az_mcts_dev_prepare", i32, [vp, i32, i64]),
    ("az_mcts_dev_prepare_stream", i32, [vp, i32, i64, vp]),
    ("az_mcts_dev_check", i32, [vp, vp]),
    ("az_mcts_dev_replay", i32, [vp, vp, i64, i64, vp]),
    ("az_mcts_dev_set_roots", i32, [vp, vp, vp, vp, vp]),
    ("az_mcts_dev_import_roots", i32, [vp, vp, vp, vp]),
    ("az_mcts_dev_select", i32, [vp, i32, i32, vp, vp, vp]),
    ("az_mcts_dev_backprop", i32, [vp, i32, i32, vp, vp, vp, vp]),
    ("az_mcts_dev_leaves", i32, [vp, i32, vp, vp, vp, vp, vp]),
    ("az_mcts_dev_leaf_syms", i32, [vp, i32, vp, vp]),
    ("az_mcts_dev_counts", i32, [vp, vp, vp]),
    ("az_mcts_dev_root_stats", i32, [vp, vp, vp]),
    ("az_mcts_dev_prune_roots", i32, [vp, vp, vp]),
    ("az_mcts_dev_reset_masked", i32, [vp, vp, vp]),
    ("az_c4_dev_step", i32, [vp, vp, vp, vp, vp, vp, i64, i32, vp]),
    ("az_game_dev_step", i32, [i32, vp, vp, vp, vp, vp, vp, vp, i64, i32, vp]),
    ("az_game_dev_valid_mask", i32, [i32, vp, vp, vp, vp, vp, i64, vp]),
    ("az_game_dev_pick", i32, [i32, vp, vp, vp, vp, vp, i64, i32, i32, i32, vp]),
    ("az_mcts_dev_ply_advance", i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]),
    ("az_mcts_dev_set_noise_epsilons", i32, [vp, vp]),
    ("az_mcts_dev_live_leaves", i32, [vp, i32, vp, vp, vp]),
    ("az_mcts_dev_search", i32, [vp, vp, i32, i32, i32, vp]),
    ("az_mcts_dev_search_more", i32, [vp, vp, i32, i32, i32, vp]),
    ("az_mcts_dev_rollout_search", i32, [vp, i32, i32, vp]),
    ("az_selfplay_create", i32, [vp, P(SelfPlayConfig), P(vp)]),
    ("az_selfplay_destroy", None, [vp]),
    ("az_selfplay_step", i32, [vp, vp, i32, i32, i32, i32, vp]),
    ("az_selfplay_begin_ply", i32, [vp, vp]),
    ("az_selfplay_finish_ply", i32, [vp, vp]),
    ("az_selfplay_set_action_tape", i32, [vp, vp, i64]),
    ("az_selfplay_totals", i32, [vp, P(i64 * 5)]),
    ("az_selfplay_positions", i32, [vp, vp, vp, vp, vp]),
    ("az_selfplay_finished", i32, [vp, P(i64), P(i64), P(i64)]),
    ("az_selfplay_drain", i32, [vp, P(SelfPlayGames), i64, i64]),
    ("az_selfplay_export", i32, [vp, P(ReplayTensorsC), i64, i32, i64, i64, P(SelfPlayExportInfo), P(i64), vp]),
    ("az_replay_dev_store", i32, [i32, P(SelfPlayGames), vp, vp, i64, P(ReplayTensorsC), i64, i32, vp]),
    ("az_selfplay_sample", i32, [i32, vp, vp, P(SelfPlayConfig), u64, u64, vp, i64, vp]),
    ("az_selfplay_create_teams", i32, [vp, P(SelfPlayConfig), vp, P(vp)]),
    ("az_selfplay_team_sample", i32, [i32, vp, vp, P(SelfPlayConfig), i32, i32, u64, u64, vp, vp, vp, i64, vp]),
    ("az_mcts_dev_team_root_stats", i32, [i32, vp, i32, i32, vp, i64, vp]),
    ("az_match_create", i32, [vp, vp, P(MatchConfig), P(vp)]),
    ("az_match_create_teams", i32, [vp, vp, P(MatchConfig), vp, P(vp)]),
    ("az_match_destroy", None, [vp]),
    ("az_match_set_positions", i32, [vp, vp, vp, vp]),
    ("az_match_step", i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
    ("az_match_step_players", i32, [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
    ("az_match_begin_ply", i32, [vp, vp, P(i32)]),
    ("az_match_finish_ply", i32, [vp, vp]),
    ("az_match_set_action_tape", i32, [vp, vp, i64]),
    ("az_match_remaining", i32, [vp, P(i64)]),
    ("az_match_results", i32, [vp, vp, vp, P(i64 * 4)]),
    ("az_match_moves", i32, [vp, vp]),
    ("az_match_max_plies", i32, [vp]),
    ("az_match_sample", i32, [i32, vp, f32, u64, u64, vp, i64, vp]),
    ("az_match_team_roots", i32, [i32, vp, vp, vp, i32, i32, vp, vp, vp, i64, vp]),
    ("az_match_team_sample", i32, [i32, vp, i32, i32, f32, u64, u64, vp, vp, i32, i32, vp, i64, vp]),
    ("az_game_num_augment", i32, [i32]),
    ("az_replay_dev_batch", i32, [i32, P(ReplayTensorsC), vp, vp, i64, i64, P(ReplayBatchC), vp]),
    ("az_replay_dev_sample_indices", i32, [u64, u64, i64, vp, i64, vp]),
    ("az_mcts_dev_tt_create", i32, [vp, i32]),
    ("az_mcts_dev_tt_clear", i32, [vp, vp]),
    ("az_mcts_dev_tt_lookup", i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
    ("az_mcts_dev_tt_insert", i32, [vp, i32, vp, vp, vp, vp, vp, vp]),
    ("az_mcts_dev_tt_refresh", i32, [vp, vp, vp]),
    ("az_mcts_dev_tt_stats", i32, [vp, P(i64 * 4)]),
    ("az_mcts_reserve", i32, [vp, i64]),
    ("az_mcts_capacity", i64, [vp]),
    ("az_mcts_epoch", i64, [vp]),
    ("az_mcts_max_used", i32, [vp, P(i64)]),
    ("az_mcts_counters", i32, [vp, P(i64 * 8)]),
    ("az_mcts_counters_reset", i32, [vp]),
    ("az_mcts_profile", i32, [vp, i32]),
    ("az_mcts_profile_read", i32, [vp, P(C.c_double * 2), P(i64 * 2)]),
    ("az_mcts_timed_select_kernel", cstr, [vp]),
    ("az_rng_gamma_selftest", i32, [u32, f32, i32, vp]),
    # include/az_nn.h
    ("az_nn_stem_embed", i32, [vp, vp, vp, vp, vp, vp, vp, i64, vp, vp, vp]),
    ("az_nn_stem_embed_positions", i32, [P(Positions), vp, vp, vp, vp, vp, vp, i64, vp, vp, vp]),
    ("az_nn_stem_folded", i32, [vp, vp, vp, vp, i64, vp, vp, vp]),
    ("az_nn_stem_folded_positions", i32, [P(Positions), vp, vp, vp, i64, vp, vp, vp]),
    ("az_nn_conv_block", i32, [vp, i32, vp, vp, vp, vp, i32, vp, i64, f32, vp, vp]),
    ("az_nn_stem_conv_block_positions", i32, [P(Positions), vp, vp, vp, vp, vp, vp, vp, i64, f32, vp, vp, vp]),
    ("az_nn_stem_conv_chain_positions", i32, [P(Positions), vp, vp, i32, vp, vp, vp, vp, vp, vp, i64, f32, vp, vp, vp]),
    ("az_nn_attn_block", i32, [vp, vp, vp, vp, vp, vp, vp, i64, f32, vp, vp]),
    ("az_nn_heads", i32, [vp, P(HeadsWeights), vp, vp, vp, vp, i64, f32, vp, vp, vp]),
    ("az_nn_attn_heads", i32, [vp, vp, vp, vp, vp, vp, P(HeadsWeights), vp, vp, vp, vp, i64, f32, vp, vp, vp]),
    ("az_nn_model_create", i32, [P(ModelWeights), P(vp)]),
    ("az_nn_model_create_hash", i32, [i32, P(vp)]),
    ("az_nn_model_create_hash_salted", i32, [i32, u64, P(vp)]),
    ("az_nn_model_kind", i32, [vp]),
    ("az_nn_model_destroy", None, [vp]),
    ("az_nn_model_scratch_bytes", u64, [vp, i64]),
    ("az_nn_model_forward", i32, [vp, vp, vp, vp, vp, vp, i64, vp, vp, vp, u64, vp]),
    ("az_nn_model_forward_positions", i32, [vp, P(Positions), vp, vp, vp, vp, i64, vp, vp, vp, u64, vp]),
    ("az_nn_model_profile", i32, [i32]),
    ("az_nn_model_profile_read", i32, [P(C.c_double), P(i64)]),
    ("az_nn_model_profile_read_kernels", i32, [P(C.c_double * 4), P(i64 * 4)]),
    # az_nn_publish_src travels as plain c_void_p; its mirror lives in src/publish.py under its own table and
    # tests/test_publish_cpu.py holds its layout to the header
    ("az_nn_publish_dev", i32, [vp, P(ModelWeights), vp, vp]),
    ("az_nn_model_set_head_biases", i32, [vp, f32, f32, f32]),
    ("az_nn_model_head_biases", i32, [vp, P(f32 * 3)]),
    ("az_nn_model_publish", i32, [vp, vp, vp, vp]),
    ("az_nn_debug", i32, [i32]),
    ("az_nn_debug_flags", i32, []),
    ("az_nn_conv_profile", i32, [vp, i32]),
    ("az_nn_debug_col_reduce2", i32, [vp, vp, vp, vp]),
    ("az_nn_embed", i32, [vp, vp, vp, vp, vp, i64, i32, vp, vp, vp]),
    ("az_nn_heads_prep", i32, [vp, vp, vp, f32, vp, vp, i64, f32, vp]),
    ("az_nn_othello_conv", i32, [vp, vp, vp, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, vp, vp]),
    ("az_nn_othello_conv_narrow", i32, [vp, vp, vp, vp, vp, i64, vp, vp]),
    ("az_nn_othello_embed", i32, [P(Positions), vp, vp, vp, i64, vp, vp, vp]),
    ("az_nn_othello_heads", i32, [vp, vp, P(_HeadsW), vp, vp, vp, i64, vp, vp, vp]),
    ("az_nn_model_create_othello", i32, [P(_OthelloW), P(vp)]),
    # az_nn_othello_publish_src travels as plain c_void_p, as az_nn_publish_src does: its mirror lives in src/publish.py
    # and tests/test_publish_othello_cpu.py holds its layout to the header
    ("az_nn_othello_publish_dev", i32, [vp, P(_OthelloW), vp, vp]),
    ("az_nn_model_set_othello_head_biases", i32, [vp, f32, f32, f32]),
    ("az_nn_model_othello_head_biases", i32, [vp, P(f32 * 3)]),
    ("az_nn_model_publish_othello", i32, [vp, vp, vp, vp]),
    # include/az_train.h
    ("az_train_loss_workspace_bytes", i64, [i32, i64]),
    ("az_train_dev_loss", i32, [i32, P(ReplayBatchC), P(TrainHeadsC), i64, P(TrainLossConfigC), P(TrainLossOutC), vp]),
    ("az_train_dev_loss_grad", i32, [i32, P(ReplayBatchC), P(TrainHeadsC), i64, P(TrainLossConfigC), P(TrainLossOutC), vp,
                                     P(TrainGradsC), vp]),
    ("az_opt_create", i32, [i64, vp, vp, i32, P(vp)]),
    ("az_opt_destroy", None, [vp]),
    ("az_opt_bind", i32, [vp, vp, vp, vp]),
    ("az_opt_dev_step", i32, [vp, vp, vp, vp, f32, vp, vp]),
    # az_learn_config and az_learn_out travel as plain c_void_p too; their mirrors live in src/learner.py under its own
    # table and tests/test_learner_cpu.py holds their layouts to the header
    ("az_learn_create", i32, [vp, P(vp)]),
    ("az_learn_destroy", None, [vp]),
    ("az_learn_bind", i32, [vp, i64, vp, vp, i32, vp, vp, vp, vp]),
    ("az_learn_dev_step", i32, [vp, P(ReplayBatchC), i64, P(TrainLossConfigC), vp, vp, u64, vp]),
    ("az_learn_dev_epoch", i32, [vp, P(ReplayTensorsC), vp, vp, i64, i64, i32, P(TrainLossConfigC), vp, vp, u64, P(i64), vp]),
    ("az_learn_dev_eval", i32, [vp, P(ReplayBatchC), i64, P(TrainLossConfigC), vp]),
    ("az_learn_dev_keep", i32, [vp, i64, u64, vp]),
    ("az_learn_outputs", i32, [vp, vp]),
    ("az_learn_reset_sums", i32, [vp, vp]),
    ("az_learn_publish", i32, [vp, vp, vp, vp]),
    ("az_train_block_workspace_bytes", i64, [i64, i32]),
    ("az_train_dev_block_fwd", i32, [vp, vp, vp, i64, f32, vp, vp, vp]),
    ("az_train_dev_block_bwd", i32, [vp, vp, vp, vp, vp, i64, i32, vp, vp]),
    ("az_train_attn_workspace_bytes", i64, [i64, i32]),
    ("az_train_dev_attn_fwd", i32, [vp, vp, i32, vp, f32, i64, f32, vp, vp]),
    ("az_train_dev_attn_bwd", i32, [vp, vp, i32, vp, f32, vp, i64, f32, i32, vp, vp]),
    ("az_train_stem_workspace_bytes", i64, [i64, i32]),
    ("az_train_dev_stem_fwd", i32, [vp, vp, i64, vp, vp, i64, vp]),
    ("az_train_dev_stem_bwd", i32, [vp, vp, vp, vp, i64, i32, vp, vp]),
    ("az_train_heads_workspace_bytes", i64, [i64, i32]),
    ("az_train_dev_heads_fwd", i32, [vp, vp, vp, vp, vp, i64, f32, vp, vp, vp, vp]),
    ("az_train_dev_heads_bwd", i32, [vp, vp, vp, vp, vp, vp, vp, vp, i64, f32, i32, vp, vp]),
)

_LIB = None


def lib():
    """lib/libaz_mcts.so, loaded once, with every prototype of `PROTOTYPES` set.  OSError when it cannot be loaded."""
    global _LIB
    if _LIB is None:
        L = C.CDLL(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib", "libaz_mcts.so"))
        for name, restype, argtypes in PROTOTYPES:
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _LIB = L
    return _LIB


def glue():
    """`lib()`, or None when the library cannot be loaded."""
    try:
        return lib()
    except OSError:
        return None


def check(rc):
    if rc != 0:
        raise RuntimeError(lib().az_last_error().decode())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def counters(handle):
    arr = (C.c_int64 * 8)()
    check(lib().az_mcts_counters(handle, C.byref(arr)))
    names = ("sims", "levels", "expansions", "terminal", "dup_leaves", "backup_nodes",
             "select_launches", "backprop_launches")
    return dict(zip(names, list(arr)))
