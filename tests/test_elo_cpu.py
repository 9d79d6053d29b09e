"""The rating step without a device: src/elo.py against the reference's own `Elo` (fixture G20), the yardsticks of the
GPU rating-match tests on the CPU oracle, and the new entry points' argument checks.

G20  tests/golden/g20_elo.npz (tests/golden/make_golden_elo.py: the reference's src/utils.py, three start pairs, 64
     updates each, one pair on the 1500 floor): every rating to a relative 1e-12 - not bit for bit, `10 ** x` comes
     from the host's libm;
Y1   the strength match of tests/test_rating_match_gpu.py on the oracle: rollout 128 against rollout 8, fresh trees,
     64 games per colour - the reference search itself must score at least 0.93 for the stronger side;
Y2   the forced move of the same file: three in a row on the bottom, 128 playouts, 8 seeds x 256 trees, no tree
     picks another column.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import scenarios as S
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
G = os.path.join(ROOT, "tests", "golden")
AZ_ERR_ARG = 1

# player.py:84-88 with pipeline.py:233's c_puct
PLAYER_C4 = dict(c_init=1.0, c_base=500.0, dirichlet_alpha=0.0, noise_epsilon=0.0, fpu_reduction=0.0, use_symmetry=False,
                 mlh_slope=0.0, mlh_cap=0.2, value_decay=1.0)


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    return True


# ------------------------------------------------------------------ G20

def test_g20_elo_reproduces_the_reference(built):
    from src.elo import Elo
    g = np.load(os.path.join(G, "g20_elo.npz"))
    assert g["ratings"].shape == (3, 64, 2)
    assert (g["ratings"][2, :, 0] == 1500).any()               # the floor is in the fixture
    for (a, b), results, want in zip(g["starts"], g["results"], g["ratings"]):
        elo = Elo(a, b)
        for r, w in zip(results, want):
            got = elo.update(float(r))
            assert np.allclose(got, w, rtol=1e-12, atol=0.0), (got, w)


def test_rate_is_update_elo_s_sequence(built):
    from src.elo import Elo, rate, score
    assert [score(w, 1) for w in (1, 0, -1)] == [1, 0.5, 0] and [score(w, -1) for w in (1, 0, -1)] == [0, 0.5, 1]
    for w1 in (1, 0, -1):
        for w2 in (1, 0, -1):
            a, b = Elo(1612.5, 1540.0), Elo(1612.5, 1540.0)
            a.update(1 if w1 == 1 else 0.5 if w1 == 0 else 0)          # pipeline.py:236
            want = a.update(1 if w2 == -1 else 0.5 if w2 == 0 else 0)  # pipeline.py:239
            assert rate(b, np.array([w1], np.int32), np.array([w2], np.int32)) == want
    # more games: first[0], second[0], first[1], second[1], ...
    first, second = [1, -1, 0], [-1, -1, 1]
    a, b = Elo(), Elo()
    for x, y in zip(first, second):
        a.update(score(x, 1))
        a.update(score(y, -1))
    assert rate(b, first, second) == (a.R_A, a.R_B)
    assert rate(Elo(1510, 1520), [], []) == (1510, 1520)


def test_elo_imports_no_engine(built):
    code = ("import sys; sys.path.insert(0, %r); import src.elo; "
            "print(sorted(m for m in ('torch', 'src.abi', 'src.MCTS_cpp', 'src.mcts_cpp', 'src.selfplay', 'src.match') if m in sys.modules))" % PKG)
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "[]"


# ------------------------------------------------------------------ Y1, Y2: the reference search as the yardstick

def oracle_rollout_match(n_games, playouts, seeds):
    """`Game.play`'s shape on the oracle, n_games in lock step: the side to move searches the position from empty
    trees with its own playout count, plays its most visited move (player.py:99-102).  playouts / seeds: (player
    +1, player -1).  Returns the winners."""
    engines = []
    for seed in seeds:
        o = O.BatchedMCTS_Connect4(n_games)
        S.apply_cfg(o, PLAYER_C4)
        o.set_seed(seed)
        engines.append(o)
    boards = np.zeros((n_games, 6, 7), np.int8)
    winner = np.zeros(n_games, np.int32)
    live = np.ones(n_games, bool)
    turn = 1
    for _ in range(42):
        if not live.any():
            break
        side = 0 if turn == 1 else 1
        o = engines[side]
        for i in range(n_games):
            o.reset_env(i)
        search_boards = np.where(live[:, None, None], boards, 0).astype(np.int8)      # a finished game: any legal position
        o.search_rollout(search_boards, np.full(n_games, turn, np.int32), playouts[side])
        moves = S.counts_of(o, n_games).argmax(1)
        for i in np.nonzero(live)[0]:
            S.np_drop(boards[i], int(moves[i]), turn)
            if S.np_done(boards[i]):
                live[i] = False
                winner[i] = S.np_winner(boards[i])
        turn = -turn
    assert not live.any()
    return winner


def strength_score(as_p1, as_p2):
    """Share of the points the player scored that was +1 in `as_p1` and -1 in `as_p2`; a draw counts half."""
    wins = np.sum(as_p1 == 1) + np.sum(as_p2 == -1)
    draws = np.sum(as_p1 == 0) + np.sum(as_p2 == 0)
    return float(wins + 0.5 * draws) / (len(as_p1) + len(as_p2))


def test_oracle_strength_match_is_the_yardstick():
    as_p1 = oracle_rollout_match(64, (128, 8), (1, 2))
    as_p2 = oracle_rollout_match(64, (8, 128), (3, 4))
    s = strength_score(as_p1, as_p2)
    print("oracle: rollout 128 against rollout 8 scores", s)
    assert s >= 0.93, s


def forced_position(n):
    boards = np.zeros((n, 6, 7), np.int8)
    boards[:, 5, 0:3] = 1
    boards[:, 4, 0:3] = -1
    return boards, np.ones(n, np.int32)


def test_oracle_plays_the_forced_move_at_128_playouts():
    boards, turns = forced_position(256)
    wrong = 0
    for seed in range(8):
        o = O.BatchedMCTS_Connect4(256)
        S.apply_cfg(o, PLAYER_C4)
        o.set_seed(seed)
        o.search_rollout(boards, turns, 128)
        wrong += int((S.counts_of(o, 256).argmax(1) != 3).sum())
    assert wrong == 0, wrong


# ------------------------------------------------------------------ argument checks that need no device

def test_step_players_refuses_a_null_match(built):
    lib = C.CDLL(os.path.join(PKG, "lib", "libaz_mcts.so"))
    assert hasattr(lib, "az_mcts_dev_rollout_search")
    vp, i32 = C.c_void_p, C.c_int
    lib.az_match_step_players.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]
    assert lib.az_match_step_players(None, None, None, 8, 8, 1, 0, 3, 1, None) == AZ_ERR_ARG
