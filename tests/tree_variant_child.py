"""One side-by-side comparison of the HIP engine with the plain-C oracle (as test_hip_parity._side_by_side: visit
counts, symmetry ids, leaf signature, root statistics as uint32 bit patterns), for test_tree_variants_gpu.

Importable (the in-process tests call `side_by_side`), and a program: the engine reads AZ_SELECT_VARIANT,
AZ_BACKPROP_V1, AZ_BACKPROP_SPREAD and AZ_TREES_PER_WAVE once per process, so every env-selected kernel route
gets a fresh interpreter that runs this file with the switches in its environment.  It builds nothing.

    python tests/tree_variant_child.py {connect4|othello} B n_playout K plies
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alphazero-al_amd"), ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import scenarios as S  # noqa: E402
from oracle import oracle as O  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def side_by_side(mcts_cpp, game, B, n, K, plies):
    """20-ply openings (duplicate leaves, terminal leaves), seeded actor configuration (root noise, symmetry ids)."""
    if game == "connect4":
        boards, turns = S.random_openings(np.random.default_rng(4), B, 20)
        makes, cfg, g = (mcts_cpp.BatchedMCTS_Connect4, O.BatchedMCTS_Connect4), dict(S.ACTOR_CFG, c_base=500.0), S.C4Game
    else:
        boards, turns = S.ot_openings(np.random.default_rng(31), B, 20)
        makes, cfg, g = (mcts_cpp.BatchedMCTS_Othello, O.BatchedMCTS_Othello), S.OT_ACTOR_CFG, S.OthelloGame
    res = []
    for make in makes:
        m = make(B)
        S.apply_cfg(m, cfg)
        m.set_seed(11 + K)
        res.append(S.play_plies(m, boards, turns, n, K, plies, record_leaves=True, game=g))
    hip, orc = res
    assert np.array_equal(hip["counts"], orc["counts"]), "visit counts differ from the oracle"
    assert np.array_equal(hip["sym"], orc["sym"]), "symmetry ids differ from the oracle"
    assert np.array_equal(hip["leaf_sig"], orc["leaf_sig"]), "leaf signature differs from the oracle"
    assert np.array_equal(_bits(hip["stats"]), _bits(orc["stats"])), "root statistics differ from the oracle"


if __name__ == "__main__":
    from src import mcts_cpp
    side_by_side(mcts_cpp, sys.argv[1], *(int(a) for a in sys.argv[2:6]))
    print("ok", " ".join(sys.argv[1:]))
