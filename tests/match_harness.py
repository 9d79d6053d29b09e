"""The reference's evaluation-match loop, restated for tests that cannot import it.

`TrainPipeline._batched_eval_games` with `_sample_actions` (src/pipeline.py:264-351) drives two `BatchedMCTS`
wrappers and the `Env` objects; fixture G17 holds what it returned on the compiled reference.  On the GPU box the
reference does not exist, so this module restates the loop - which engine searches, how moves are drawn from
numpy's global generator (active games only, in index order), that BOTH wrappers are re-rooted with every move, that
finished games stay in the batch and play their arg-max - on top of any two objects with the wrapper's interface.
tests/test_match_cpu.py checks the restatement against G17 (oracle as the native backend); the GPU suite compares
the native match driver (az_match_*) with it.

Two additions for tests: `openings` (one move sequence per game) or `positions` ((boards, turns), one side to move)
are put on the Envs before the first search, with both wrappers' trees reset; and every move is recorded.
"""
import numpy as np

import scenarios as S


def sample_actions(visits, temp, active_idx):
    """pipeline.py:337-351: arg-max everywhere, then one np.random.choice per ACTIVE game in index order."""
    actions = np.argmax(visits, axis=1).astype(np.int32)
    for i in active_idx:
        v = visits[i]
        valid_mask = v > 0
        valid_actions = np.where(valid_mask)[0]
        log_v = np.log(v[valid_mask].astype(np.float64))
        log_v -= log_v.max()
        probs = np.exp(log_v / temp)
        probs /= probs.sum()
        actions[i] = np.random.choice(valid_actions, p=probs)
    return actions


def start_envs(Env, n_envs, openings=None, positions=None):
    """The games' Env objects: reset (pipeline.py:295-297), then the opening moves, or the given positions."""
    assert openings is None or positions is None
    if positions is not None:
        boards, turns = positions
        envs = []
        for b, t in zip(boards, turns):
            e = Env(np.asarray(b, np.float32))
            e.turn = int(t)
            envs.append(e)
        return envs
    envs = [Env() for _ in range(n_envs)]
    for e in envs:
        e.reset()
    for e, seq in zip(envs, openings or []):
        for a in seq:
            e.step(int(a))
    return envs


def env_bitboards(envs):
    """(bb_p1, bb_p2, turns) of the Envs, as az_match_set_positions takes them."""
    bb = [e.bitboards for e in envs]
    return (np.array([int(b[0]) for b in bb], np.uint64), np.array([int(b[1]) for b in bb], np.uint64),
            np.array([int(e.turn) for e in envs], np.int32))


def batched_eval_games(w_p1, w_p2, net_p1, net_p2, Env, n_envs, vl_batch=1, eval_temp=0.2, openings=None, positions=None):
    """pipeline.py:295-335 on the two search wrappers `w_p1` (player +1) and `w_p2` (player -1), each of n_envs
    trees and configured by the caller (pipeline.py:286-293).  Returns dict(winner int32 [n], length int32 [n],
    moves int32 [plies, n] with -1 where the game had ended)."""
    envs = start_envs(Env, n_envs, openings, positions)
    for i in range(n_envs):
        w_p1.reset_env(i)
        w_p2.reset_env(i)
    board_shape = tuple(np.asarray(envs[0].board).shape)
    boards = np.zeros((n_envs, *board_shape), dtype=np.int8)
    turns = np.ones(n_envs, dtype=np.int32)
    done = np.array([bool(e.done()) for e in envs])
    results = np.array([int(e.winPlayer()) if d else 0 for e, d in zip(envs, done)], dtype=np.int32)
    length = np.zeros(n_envs, dtype=np.int32)
    moves = []
    while not done.all():
        active_idx = np.where(~done)[0]
        current_turn = int(envs[active_idx[0]].turn)
        assert all(int(envs[i].turn) == current_turn for i in active_idx), "one side to move per ply"
        for i in range(n_envs):
            boards[i] = np.asarray(envs[i].board).astype(np.int8)
            turns[i] = int(envs[i].turn)
        if current_turn == 1:
            w_p1.batch_playout(net_p1, boards, turns, vl_batch=vl_batch)
            visits = w_p1.get_visits_count()
        else:
            w_p2.batch_playout(net_p2, boards, turns, vl_batch=vl_batch)
            visits = w_p2.get_visits_count()
        if eval_temp > 0:
            actions = sample_actions(visits, eval_temp, active_idx)
        else:
            actions = np.argmax(visits, axis=1).astype(np.int32)
        w_p1.prune_roots(actions)
        w_p2.prune_roots(actions)
        row = np.full(n_envs, -1, np.int32)
        for i in active_idx:
            envs[i].step(int(actions[i]))
            row[i] = actions[i]
            length[i] += 1
            if envs[i].done():
                done[i] = True
                results[i] = envs[i].winPlayer()
        moves.append(row)
    return dict(winner=results, length=length, moves=np.array(moves, np.int32).reshape(len(moves), n_envs))


class OthelloNumpyHashEvaluator:
    """tests/scenarios.py `OthelloHashPV` with a salt XOR-ed into the first bitboard word before the hash: the numpy
    twin of az_nn_model_create_hash_salted(AZ_GAME_OTHELLO, salt) and of hash_eval.OthelloHashEvaluator(salt=...)."""
    n_actions = S.OT_A

    def __init__(self, salt=0):
        self.native_hash_salt = int(salt) & ((1 << 64) - 1)

    def predict(self, state, action_mask=None):
        state = np.asarray(state)
        turns = state[:, 2, 0, 0].astype(np.int32)
        boards = ((state[:, 0] - state[:, 1]) * turns[:, None, None]).astype(np.int8)
        bb0, bb1 = S.ot_bitboards(boards)
        h = S.hash64(bb0 ^ np.uint64(self.native_hash_salt), bb1, turns)
        n = h.shape[0]
        probs = np.empty((n, S.OT_A), np.float32)
        with np.errstate(over="ignore"):
            for k in range(5):
                hk = h + np.uint64(0x9E3779B97F4A7C15) * np.uint64(k + 1)
                hk ^= hk >> np.uint64(29); hk *= np.uint64(0xBF58476D1CE4E5B9); hk ^= hk >> np.uint64(32)
                for j in range(16):
                    a = k * 16 + j
                    if a < S.OT_A:
                        probs[:, a] = (1 + ((hk >> np.uint64(4 * j)) & np.uint64(15))).astype(np.float32) / np.float32(16)
        w = np.stack([1 + ((h >> np.uint64(s)) & np.uint64(31)) for s in (28, 33, 38)], axis=1)
        wdl = (w.astype(np.float32) / w.sum(axis=1, keepdims=True).astype(np.float32)).astype(np.float32)
        aux = ((h >> np.uint64(43)) & np.uint64(63)).astype(np.float32) / np.float32(32) - np.float32(1)
        if action_mask is not None:
            probs = probs * np.asarray(action_mask, dtype=np.float32)
        return probs, wdl, aux.reshape(-1, 1)


def moves_table(moves, max_plies):
    """A harness move record padded to the native record's [max_plies, n] with -1."""
    out = np.full((max_plies, moves.shape[1]), -1, np.int32)
    out[:moves.shape[0]] = moves
    return out
