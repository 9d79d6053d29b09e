#!/usr/bin/env python3
"""Generate tests/golden/g21_team_play.npz from the REAL reference, compiled into oracle/_ref.

Run in the build container only (needs the reference checkout):

    make -C oracle ref && OMP_NUM_THREADS=1 python tests/golden/make_golden_team.py

What was done, in the manner of make_golden_match.py: the reference's compiled extensions are imported from
oracle/_ref/native, its unmodified Python (src/player.py, src/symmetry.py, src/MCTS_cpp.py) from the reference checkout;
nothing of it is copied or restated here - the restatement under test is tests/team_harness.py.

(a) symmetry functions: for both games and every symmetry id of the game's ensemble, `apply_sym_board` on random boards,
    `apply_sym_action` for every action, `inverse_sym_visits` on random count vectors.
(b) ensemble decisions: the reference's own `AlphaZeroPlayer(sym_ensemble=True, alpha=None, is_selfplay=0)` over the numpy
    hash evaluator (this project's src/hash_eval.py for Connect4, tests/match_harness.py's twin for Othello) on positions
    reached by fixed openings; `get_visits_count` of the player's search object is wrapped to keep the per-tree raw
    counts, `get_action(env, temp=0)` gives the action and `action_probs`.  For Connect4 the same with `n_trees=3` and no
    ensemble.  No noise (alpha=None) and the engine's random symmetry off, so nothing is drawn from the reference's
    generator; the trees are reset after every call (is_selfplay=0), so each position is searched from empty trees.

The committed file holds data only: boards, count vectors, actions, probabilities, the openings and the settings.
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

SALT = 0x5A17C0DE1234ABCD
MAX_OPENING = 8
# fixed openings.  Connect4: the columns played; Othello: per ply, which of the legal moves in ascending order is played
# (index modulo their number) - the moves themselves go into the fixture
OPENINGS = {
    "Connect4": [[], [3], [3, 3, 2], [0, 6, 2, 4], [3, 2, 3, 2, 4], [1, 1, 5, 5, 0, 6], [6, 5, 6, 5, 6, 4, 0, 0]],
    "Othello": [[], [0], [1, 2], [3, 0, 2], [2, 2, 1, 4], [0, 1, 0, 3, 5], [3, 3, 3, 3, 3, 3, 3, 3]],
}
PLAYED = {"Connect4": OPENINGS["Connect4"], "Othello": []}      # Othello: filled by the first case that plays them
# name: (game, sym_ensemble, n_trees, n_playout, c_init, salt)
CASES = {
    "c4_ens": ("Connect4", True, 1, 48, 1.25, 0),
    "c4_ens_salted": ("Connect4", True, 1, 30, 1.6, SALT),
    "c4_trees3": ("Connect4", False, 3, 40, 1.25, 0),
    "ot_ens": ("Othello", True, 1, 28, 1.25, 0),
    "ot_ens_salted": ("Othello", True, 1, 20, 1.6, SALT),
}


def symmetry_records(out):
    rng = np.random.default_rng(21)
    for game, tag, shape, A in (("Connect4", "c4", (6, 7), 7), ("Othello", "ot", (8, 8), 65)):
        ids = list(ref_sym.get_sym_config(game)["sym_ids"])
        boards = rng.integers(-1, 2, (4,) + shape).astype(np.int8)
        visits = rng.integers(0, 50, (4, A)).astype(np.int32)
        out[tag + "_sym_ids"] = np.array(ids, np.int32)
        out[tag + "_sym_boards_in"] = boards
        out[tag + "_sym_visits_in"] = visits
        out[tag + "_sym_boards"] = np.array([[ref_sym.apply_sym_board(b, s, game) for b in boards] for s in ids], np.int8)
        out[tag + "_sym_actions"] = np.array([[ref_sym.apply_sym_action(a, s, game) for a in range(A)] for s in ids], np.int32)
        out[tag + "_sym_visits"] = np.array([[ref_sym.inverse_sym_visits(v, s, game) for v in visits] for s in ids], np.int32)


def decisions(game, ensemble, n_trees, n_playout, c_init, salt):
    Env = C4Env if game == "Connect4" else OtEnv
    net = HASH.NumpyHashEvaluator(salt) if game == "Connect4" else MH.OthelloNumpyHashEvaluator(salt)
    player = AlphaZeroPlayer(net, n_envs=1, c_init=c_init, c_base=500, n_playout=n_playout, alpha=None, is_selfplay=0,
                             use_symmetry=False, game_name=game, n_trees=n_trees, sym_ensemble=ensemble)
    player.eval()
    if not ensemble and n_trees > 1:
        player.mcts.set_noise_epsilon(0.0)          # eval() keeps 0.05 for root-parallel play: nothing random in a fixture
    seen = []
    real = player.mcts.get_visits_count

    def recording():
        v = np.array(real(), np.int32)
        seen.append(v.copy())
        return v
    player.mcts.get_visits_count = recording
    boards, turns, tree_visits, actions, probs = [], [], [], [], []
    played = []
    for seq in OPENINGS[game]:
        env = Env()
        env.reset()
        played.append([])
        for a in seq:
            valid = sorted(int(v) for v in env.valid_move())
            a = a if game == "Connect4" else valid[a % len(valid)]
            assert a in valid, (game, seq, a)
            env.step(int(a))
            played[-1].append(int(a))
        assert not env.done()
        boards.append(np.asarray(env.board).astype(np.int8).copy())
        turns.append(int(env.turn))
        n_before = len(seen)
        action, p = player.get_action(env, 0)
        assert len(seen) == n_before + 1
        tree_visits.append(seen[-1])
        actions.append(int(action))
        probs.append(np.asarray(p, np.float32).copy())
    assert PLAYED[game] in ([], played)
    PLAYED[game] = played
    return (np.array(boards, np.int8), np.array(turns, np.int32), np.array(tree_visits, np.int32), np.array(actions, np.int32),
            np.array(probs, np.float32))


def main():
    out = dict(salt=np.array([SALT], np.uint64))
    symmetry_records(out)
    for name, (game, ensemble, n_trees, n_playout, c_init, salt) in CASES.items():
        boards, turns, visits, actions, probs = decisions(game, ensemble, n_trees, n_playout, c_init, salt)
        out[name + "_boards"], out[name + "_turns"] = boards, turns
        out[name + "_tree_visits"], out[name + "_actions"], out[name + "_probs"] = visits, actions, probs
        out[name + "_settings"] = np.array([int(ensemble), n_trees, n_playout], np.int32)
        out[name + "_floats"] = np.array([c_init, 500.0], np.float64)            # c_init, c_base
        out[name + "_salt"] = np.array([salt], np.uint64)
        differ = sum(len({tuple(r) for r in v}) > 1 for v in visits)
        print(name, "actions", actions.tolist(), "positions whose trees differ (raw counts):", differ, "of", len(visits))
    for game, tag in (("Connect4", "c4"), ("Othello", "ot")):
        op = np.full((len(PLAYED[game]), MAX_OPENING), -1, np.int32)
        for i, seq in enumerate(PLAYED[game]):
            op[i, :len(seq)] = seq
        out[tag + "_openings"] = op
    path = os.path.join(HERE, "g21_team_play.npz")
    np.savez_compressed(path, **out)
    print("g21_team_play.npz  %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
