#!/usr/bin/env python3
"""Generate tests/golden/g22_team_stats.npz from the REAL reference, compiled into oracle/_ref.

Run in the build container only (needs the reference checkout):

    make -C oracle ref && OMP_NUM_THREADS=1 python tests/golden/make_golden_team_stats.py

In the manner of make_golden_team.py: the reference's compiled extensions are imported from oracle/_ref/native, its
unmodified Python (src/player.py, src/symmetry.py, src/MCTS_cpp.py) from the reference checkout; nothing of it is copied or
restated here - the restatements under test are tests/team_selfplay_harness.py, `team_root_stats` of src/match.py and the
kernel k_team_root_stats.  Root statistics travel as rows of 6 + 8A floats, the layout of the reference's own
`get_all_root_stats` (head root_N, root_Q, root_M, root_D, root_P1W, root_P2W, then per action N, Q, prior, noise, M, D, P1W,
P2W); `pack` below only lays a dict of `get_root_stats` / `inverse_sym_stats` out in that order.

(a) `inverse_sym_stats` (src/symmetry.py:140-186)
    real statistics: `AlphaZeroPlayer(sym_ensemble=True, alpha=None, is_selfplay=0)` over the numpy hash evaluators on the
      positions of fixture G21's openings, both games; `get_root_stats()` of the player's search object right after the
      search (from inside a wrapped `get_visits_count`, before the trees are reset), merged with the game's sym_ids;
    random arrays: ensembles of 2 (Connect4) and 4 (Othello) trees, root-parallel teams of 3 and 7 with sym_ids = [0] * K.
(b) self-play ply sequences: the reference's player with is_selfplay=1, alpha=None, use_symmetry=False - as an ensemble for
    both games and with n_trees=3 for Connect4 - plays `get_action(env, temp=0)` ply after ply from several of G21's openings,
    at least MIN_PLIES plies each (a sequence ends early when its game does), so that the subtrees every tree keeps matter.
    Per ply: the position, the per-tree raw visit counts and root statistics, the action, `action_probs`, and the statistics
    merged by `inverse_sym_stats`.

Asserted here, on the reference alone (else the symmetry handling would not be exercised): in at least half of the ensemble
positions the trees' raw count rows are not all equal, and in at least one position the merged Q differs from tree 0's Q
for some action.

The committed file holds data only: boards, count vectors, statistics, actions, probabilities, the openings and settings.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("AZ_REFERENCE", "/root/reference")
assert os.environ.get("OMP_NUM_THREADS") == "1", "run with OMP_NUM_THREADS=1"

sys.path[:0] = [os.path.join(ROOT, "oracle", "_ref", "native"), REF, os.path.join(ROOT, "tests")]
for absent in ("numba", "swanlab"):
    if absent not in sys.modules:
        sys.modules[absent] = types.ModuleType(absent)
sys.modules["numba"].njit = lambda *a, **k: (lambda f: f)

from src import symmetry as ref_sym                 # noqa: E402  (reference python, unmodified)
from src.player import AlphaZeroPlayer              # noqa: E402  (reference python, unmodified)
from src.env_cpp.connect4 import Env as C4Env       # noqa: E402  (compiled reference)
from src.env_cpp.othello import Env as OtEnv        # noqa: E402  (compiled reference)

import match_harness as MH                          # noqa: E402


def _project_module(name, path):
    """A module of THIS project by file path (its package is called `src` too, like the reference's)."""
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


HASH = _project_module("az_hash_eval", os.path.join(ROOT, "alphazero-al_amd", "src", "hash_eval.py"))
G21 = np.load(os.path.join(HERE, "g21_team_play.npz"))

SALT = int(G21["salt"][0])
HEAD = ("root_N", "root_Q", "root_M", "root_D", "root_P1W", "root_P2W")
FIELDS = ("N", "Q", "prior", "noise", "M", "D", "P1W", "P2W")
MIN_PLIES = 6
# (a) real statistics - name: (game, n_playout, c_init, salt): G21's ensemble cases
REAL = {"c4_real": ("Connect4", 48, 1.25, 0), "c4_real_salted": ("Connect4", 30, 1.6, SALT),
        "ot_real": ("Othello", 28, 1.25, 0), "ot_real_salted": ("Othello", 20, 1.6, SALT)}
# (a) random arrays - name: (game, trees, ensemble)
RANDOM = {"c4_rand_ens": ("Connect4", 2, True), "ot_rand_ens": ("Othello", 4, True), "c4_rand_3": ("Connect4", 3, False),
          "c4_rand_7": ("Connect4", 7, False), "ot_rand_3": ("Othello", 3, False), "ot_rand_7": ("Othello", 7, False)}
# (b) - name: (game, sym_ensemble, n_trees, n_playout, c_init, salt, which of G21's openings, plies played from each)
SELFPLAY = {"c4_sp_ens": ("Connect4", True, 1, 48, 1.25, 0, (0, 1, 3, 5), 8),
            "c4_sp_trees3": ("Connect4", False, 3, 40, 1.25, SALT, (0, 1, 4), 7),
            "ot_sp_ens": ("Othello", True, 1, 28, 1.25, 0, (0, 2, 4), 6)}


def openings_of(game):
    return [[int(a) for a in row if a >= 0] for row in G21[("c4" if game == "Connect4" else "ot") + "_openings"]]


def pack(stats, n):
    """A dict of `get_root_stats` / `inverse_sym_stats` as rows [n][6 + 8A] in `get_all_root_stats`'s order."""
    for k in HEAD + FIELDS:
        assert np.asarray(stats[k]).dtype == np.float32, (k, np.asarray(stats[k]).dtype)
    head = np.stack([np.asarray(stats[k]).reshape(n) for k in HEAD], axis=1)
    per = np.stack([np.asarray(stats[k]).reshape(n, -1) for k in FIELDS], axis=2)
    return np.concatenate([head, per.reshape(n, -1)], axis=1).astype(np.float32)


def unpack(rows, A):
    """Rows [K][6 + 8A] as the dict `get_root_stats` returns (per-action arrays of shape (K, A))."""
    rows = np.asarray(rows, np.float32)
    out = {k: np.ascontiguousarray(rows[:, i]) for i, k in enumerate(HEAD)}
    per = rows[:, 6:].reshape(len(rows), A, 8)
    out.update({k: np.ascontiguousarray(per[:, :, i]) for i, k in enumerate(FIELDS)})
    return out


def sym_ids_of(game, trees, ensemble):
    return list(ref_sym.get_sym_config(game)["sym_ids"]) if ensemble else [0] * trees


def make_player(game, ensemble, n_trees, n_playout, c_init, salt, is_selfplay):
    net = HASH.NumpyHashEvaluator(salt) if game == "Connect4" else MH.OthelloNumpyHashEvaluator(salt)
    player = AlphaZeroPlayer(net, n_envs=1, c_init=c_init, c_base=500, n_playout=n_playout, alpha=None, is_selfplay=is_selfplay,
                             use_symmetry=False, game_name=game, n_trees=n_trees, sym_ensemble=ensemble)
    seen = []
    real = player.mcts.get_visits_count

    def recording():
        v = np.array(real(), np.int32)
        stats = player.mcts.get_root_stats()
        seen.append((v.copy(), pack(stats, len(v)), {k: np.array(x, copy=True) for k, x in stats.items()}))
        return v
    player.mcts.get_visits_count = recording
    return player, seen


def opening_env(game, seq):
    env = (C4Env if game == "Connect4" else OtEnv)()
    env.reset()
    for a in seq:
        assert int(a) in [int(v) for v in env.valid_move()]
        env.step(int(a))
    assert not env.done()
    return env


def real_statistics(out, name, game, n_playout, c_init, salt):
    player, seen = make_player(game, True, 1, n_playout, c_init, salt, 0)
    ids = sym_ids_of(game, 0, True)
    raw, merged = [], []
    for seq in openings_of(game):
        env = opening_env(game, seq)
        player.get_action(env, 0)
        _, rows, stats = seen[-1]
        raw.append(rows)
        merged.append(pack(ref_sym.inverse_sym_stats(stats, ids, game), 1)[0])
    out[name + "_stats"], out[name + "_merged"] = np.array(raw, np.float32), np.array(merged, np.float32)
    out[name + "_team"] = np.array([len(ids), 1], np.int32)
    return len(raw)


def random_statistics(out, name, game, trees, ensemble, rng, n=4):
    A = 7 if game == "Connect4" else 65
    rows = np.zeros((n, trees, 6 + 8 * A), np.float32)
    merged = []
    for i in range(n):
        r = rows[i]
        r[:, 0] = rng.integers(1, 400, trees)
        r[:, 1:6] = rng.uniform(-1, 1, (trees, 5))
        per = r[:, 6:].reshape(trees, A, 8)
        per[:, :, 0] = rng.integers(0, 60, (trees, A)) * (rng.random((trees, A)) < 0.7)
        per[:, :, 1:] = rng.uniform(-1, 1, (trees, A, 7))
        if A > 7:                                      # Othello: a dozen squares and the pass have an edge, as at a real root
            keep = np.zeros(A, bool)
            keep[rng.choice(A - 1, 12, replace=False)] = True
            keep[[1, 2, A - 1]] = True
            per[:, ~keep, :] = 0
        per[:, 1, 0] = 0                               # an action nobody visited: the weighted means are 0
        per[1:, 2, 0] = 0                              # an action only tree 0 visited (where it sits in tree 0's frame)
        merged.append(pack(ref_sym.inverse_sym_stats(unpack(r, A), sym_ids_of(game, trees, ensemble), game), 1)[0])
    out[name + "_stats"], out[name + "_merged"] = rows, np.array(merged, np.float32)
    out[name + "_team"] = np.array([trees, int(ensemble)], np.int32)


def selfplay_sequences(out, name, game, ensemble, n_trees, n_playout, c_init, salt, which, plies):
    player, seen = make_player(game, ensemble, n_trees, n_playout, c_init, salt, 1)
    ids = sym_ids_of(game, n_trees, ensemble)
    openings = openings_of(game)
    boards, turns, visits, stats, merged, actions, probs, lengths = [], [], [], [], [], [], [], []
    for o in which:
        env = opening_env(game, openings[o])
        player.reset_player()
        lengths.append(0)
        for _ in range(plies):
            if env.done():
                break
            lengths[-1] += 1
            boards.append(np.asarray(env.board).astype(np.int8).copy())
            turns.append(int(env.turn))
            n_before = len(seen)
            action, p = player.get_action(env, 0)
            assert len(seen) == n_before + 1
            visits.append(seen[-1][0]); stats.append(seen[-1][1])
            merged.append(pack(ref_sym.inverse_sym_stats(seen[-1][2], ids, game), 1)[0])
            actions.append(int(action)); probs.append(np.asarray(p, np.float32).copy())
            env.step(int(action))
    assert min(lengths) >= MIN_PLIES, (name, lengths)
    # the plies of all sequences one after the other; sequence i has lengths[i] of them
    out[name + "_boards"] = np.array(boards, np.int8)
    out[name + "_turns"] = np.array(turns, np.int32)
    out[name + "_tree_visits"] = np.array(visits, np.int32)
    out[name + "_stats"] = np.array(stats, np.float32)
    out[name + "_merged"] = np.array(merged, np.float32)
    out[name + "_actions"] = np.array(actions, np.int32)
    out[name + "_probs"] = np.array(probs, np.float32)
    out[name + "_openings"] = np.array(which, np.int32)
    out[name + "_lengths"] = np.array(lengths, np.int32)
    out[name + "_settings"] = np.array([int(ensemble), n_trees, n_playout, plies], np.int32)
    out[name + "_floats"] = np.array([c_init, 500.0], np.float64)            # c_init, c_base
    out[name + "_salt"] = np.array([salt], np.uint64)
    return np.array(visits, np.int32), np.array(stats, np.float32), np.array(merged, np.float32)


def exercised(visits, stats, merged, A):
    """(positions whose trees' raw count rows are not all equal, positions whose merged Q differs from tree 0's somewhere)"""
    differ = sum(len({tuple(r) for r in v}) > 1 for v in visits)
    q_tree0 = stats[:, 0, 6:].reshape(len(stats), A, 8)[:, :, 1]
    q_merged = merged[:, 6:].reshape(len(merged), A, 8)[:, :, 1]
    return differ, int((q_tree0.view(np.uint32) != q_merged.view(np.uint32)).any(axis=1).sum())


def main():
    out = dict(salt=np.array([SALT], np.uint64), min_plies=np.array([MIN_PLIES], np.int32))
    rng = np.random.default_rng(22)
    for name, case in REAL.items():
        print(name, "positions:", real_statistics(out, name, *case))
    for name, case in RANDOM.items():
        random_statistics(out, name, *case, rng)
    positions = differ = q_moved = 0
    for name, case in SELFPLAY.items():
        visits, stats, merged = selfplay_sequences(out, name, *case)
        d, q = exercised(visits, stats, merged, 7 if case[0] == "Connect4" else 65)
        print(name, "plies:", len(visits), "trees differ (raw counts):", d, "merged Q != tree 0's Q:", q,
              "actions", out[name + "_actions"].tolist())
        if case[1]:
            positions, differ, q_moved = positions + len(visits), differ + d, q_moved + q
    assert 2 * differ >= positions, "the ensemble's trees agree too often: the symmetry handling is not exercised"
    assert q_moved >= 1, "the merged Q never differs from tree 0's"
    path = os.path.join(HERE, "g22_team_stats.npz")
    np.savez_compressed(path, **out)
    print("g22_team_stats.npz  %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
