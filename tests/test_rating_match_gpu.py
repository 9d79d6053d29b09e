"""Rating matches on the device: az_match_step_players (players of either kind, fresh trees) and its Python side
(match.RolloutPlayer, EvaluationMatch(fresh_trees=...), match.rating_games).

R1  composition: az_match_step_players equals the same plies issued by hand - az_match_begin_ply, a reset of the
    mover's trees, az_mcts_dev_rollout_search (or az_mcts_dev_search for a network side), az_match_finish_ply;
R2  fresh trees are fresh, and a fresh-tree player's arenas do not grow from ply to ply;
R3  a forced move is played; R4 more playouts win (yardsticks: tests/test_elo_cpu.py runs both on the CPU oracle);
R5  the Python side.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
SALT = 0x5A17C0DE1234ABCD


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src import abi, hash_eval, match
    return dict(torch=torch, F=abi, L=abi.lib(), M=match, H=hash_eval)


def rollout_engine(env, n, seed, game=0):
    """An engine as MCTSPlayer configures it (player.py:84-88) with pipeline.py:233's c_puct."""
    L, m = env["L"], C.c_void_p()
    env["F"].check(L.az_mcts_create(game, n, -1, C.byref(m)))
    cfg = L.az_mcts_config(m).contents
    cfg.c_init, cfg.c_base, cfg.dirichlet_alpha, cfg.noise_epsilon, cfg.fpu_reduction, cfg.use_symmetry = 1.0, 500.0, 0.0, 0.0, 0.0, 0
    cfg.mlh_slope, cfg.value_decay = 0.0, 1.0
    env["F"].check(L.az_mcts_set_seed(m, seed))
    return m


def network_engine(env, n, seed):
    L, m = env["L"], C.c_void_p()
    env["F"].check(L.az_mcts_create(0, n, -1, C.byref(m)))
    cfg = L.az_mcts_config(m).contents
    cfg.c_init, cfg.c_base, cfg.dirichlet_alpha, cfg.noise_epsilon, cfg.use_symmetry = 1.25, 500.0, 0.3, 0.25, 1
    env["F"].check(L.az_mcts_set_seed(m, seed))
    return m


class Match:
    """A match object over two engines, through ctypes only.  models: per side an az_nn_model* or None (rollout)."""

    def __init__(self, env, engines, models, playouts, n, K=4):
        self.env, self.e, self.models, self.playouts, self.n, self.K = env, engines, models, playouts, n, K
        self.mt = C.c_void_p()
        env["F"].check(env["L"].az_match_create(engines[0], engines[1], C.byref(env["F"].MatchConfig(0.0, 1)), C.byref(self.mt)))
        self.ones = env["torch"].ones(n, dtype=env["torch"].uint8, device="cuda")

    def close(self):
        L = self.env["L"]
        L.az_match_destroy(self.mt)
        for e in self.e:
            L.az_mcts_destroy(e)

    def set_positions(self, bb1, bb2, turn):
        a, b = np.full(self.n, bb1, np.uint64), np.full(self.n, bb2, np.uint64)
        t = np.full(self.n, turn, np.int32)
        self.env["F"].check(self.env["L"].az_match_set_positions(self.mt, a.ctypes.data, b.ctypes.data, t.ctypes.data))

    def step(self, fresh, n_plies=1):
        F, L = self.env["F"], self.env["L"]
        F.check(L.az_match_step_players(self.mt, self.models[0], self.models[1], self.playouts[0], self.playouts[1], self.K, 0,
                                        fresh, n_plies, F._stream()))

    def ply_by_hand(self, fresh, probe=None):
        """One ply as the calls az_match_step_players documents.  probe(side): called between search and finish.
        False: the match is over."""
        F, L = self.env["F"], self.env["L"]
        s, mover = F._stream(), C.c_int()
        F.check(L.az_match_begin_ply(self.mt, s, C.byref(mover)))
        if mover.value == 0:
            return False
        i = 0 if mover.value > 0 else 1
        if (fresh >> i) & 1:
            F.check(L.az_mcts_dev_reset_masked(self.e[i], self.ones.data_ptr(), s))
        if self.models[i] is None:
            F.check(L.az_mcts_dev_rollout_search(self.e[i], self.playouts[i], 0, s))
        else:
            F.check(L.az_mcts_dev_search(self.e[i], self.models[i], self.playouts[i], self.K, 0, s))
        if probe is not None:
            probe(i)
        F.check(L.az_match_finish_ply(self.mt, s))
        return True

    def remaining(self):
        left = C.c_int64()
        self.env["F"].check(self.env["L"].az_match_remaining(self.mt, C.byref(left)))
        return left.value

    def results(self):
        w, ln, t = np.zeros(self.n, np.int32), np.zeros(self.n, np.int32), (C.c_int64 * 4)()
        moves = np.zeros((42, self.n), np.int32)
        self.env["F"].check(self.env["L"].az_match_results(self.mt, w.ctypes.data, ln.ctypes.data, C.byref(t)))
        self.env["F"].check(self.env["L"].az_match_moves(self.mt, moves.ctypes.data))
        return dict(winner=w, length=ln, moves=moves, running=t[3])

    def root_n(self, side):
        torch = self.env["torch"]
        st = torch.zeros((self.n, 6 + 8 * 7), dtype=torch.float32, device="cuda")
        self.env["F"].check(self.env["L"].az_mcts_dev_root_stats(self.e[side], st.data_ptr(), self.env["F"]._stream()))
        torch.cuda.synchronize()
        return st[:, 0].cpu().numpy().astype(np.int64)

    def capacities(self):
        return tuple(int(self.env["L"].az_mcts_capacity(e)) for e in self.e)


def rollout_match(env, n, playouts, seeds=(1, 2)):
    return Match(env, [rollout_engine(env, n, s) for s in seeds], (None, None), playouts, n)


def play_out(mt, fresh, by_hand):
    for _ in range(42):
        if by_hand:
            if not mt.ply_by_hand(fresh):
                break
        else:
            mt.step(fresh)
            if mt.remaining() == 0:
                break
    r = mt.results()
    assert r["running"] == 0
    return r


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("moves", "winner", "length"))


# ---------------------------------------------------------------------------------------- R1

def test_step_players_equals_the_plies_issued_by_hand_rollout_players(env):
    runs = []
    for by_hand in (False, True, False):
        mt = rollout_match(env, 16, (48, 12))
        runs.append(play_out(mt, 3, by_hand))
        mt.close()
    assert same(runs[0], runs[1]), "az_match_step_players against begin / reset / search / finish"
    assert same(runs[0], runs[2]), "the same seeds give the same match"
    assert len({tuple(runs[0]["moves"][:, i]) for i in range(16)}) > 4      # the playouts' randomness makes games differ


def test_step_players_equals_the_plies_issued_by_hand_network_against_rollout(env):
    """A salted hash model as player +1 that KEEPS its trees against a fresh-tree rollout player."""
    L, runs = env["L"], []
    for by_hand in (False, True, False):
        model = C.c_void_p()
        env["F"].check(L.az_nn_model_create_hash_salted(0, SALT, C.byref(model)))
        mt = Match(env, [network_engine(env, 16, 5), rollout_engine(env, 16, 6)], (model, None), (24, 24), 16, K=4)
        runs.append(play_out(mt, 2, by_hand))
        mt.close()
        L.az_nn_model_destroy(model)
    assert same(runs[0], runs[1]) and same(runs[0], runs[2])


# ---------------------------------------------------------------------------------------- R2

def test_fresh_trees_are_fresh(env):
    """Played in halves: a fresh-tree mover's root holds exactly its n_playout visits in every running game from its
    second search on; a mover that keeps its subtree holds more in at least one game."""
    playouts = (48, 12)
    seen = {}
    for fresh in (3, 0):
        mt = rollout_match(env, 16, playouts)
        rows = []

        def probe(side):
            played = len(rows)
            running = mt.results()["length"] == played              # still running before this ply
            rows.append((side, mt.root_n(side), running))
        for _ in range(42):
            if not mt.ply_by_hand(fresh, probe):
                break
        mt.close()
        seen[fresh] = rows
    for ply, (side, n, running) in enumerate(seen[3]):
        if ply >= 2 and running.any():
            assert (n[running] == playouts[side]).all(), (ply, side, n[running])
    assert any((n[running] > playouts[side]).any() for ply, (side, n, running) in enumerate(seen[0]) if ply >= 2)


def test_step_players_starts_fresh_tree_movers_from_empty_trees(env):
    """The same through az_match_step_players, seen from behind the re-rooting that ends a ply: a search of n
    simulations from an empty tree gives the root n visits and its children n - 1 between them, so the subtree kept
    under the move holds at most n - 1; a mover that keeps its subtrees passes that in at least one game.  And the
    arenas of a fresh-tree player stay as they are after the first plies."""
    playouts = (48, 12)
    over = {}
    for fresh in (3, 0):
        mt = rollout_match(env, 16, playouts)
        over[fresh], caps = False, []
        for ply in range(42):
            mt.step(fresh)
            side = ply % 2
            n = mt.root_n(side)
            if fresh:
                assert (n <= playouts[side] - 1).all(), (ply, n)
            over[fresh] = over[fresh] or bool((n > playouts[side] - 1).any())
            caps.append(mt.capacities())
            if mt.remaining() == 0:
                break
        if fresh:
            assert len(caps) > 4 and caps[3] == caps[-1], caps
        mt.close()
    assert over[0] and not over[3]


# ---------------------------------------------------------------------------------------- R3, R4

def test_rollout_player_plays_the_forced_move(env):
    """Three in a row on the bottom, the mover wins in column 3 (the position of test_rollout_search_on_device): 128
    playouts find it in every game (oracle: 0 of 2048 trees miss it at 64 and at 128 playouts)."""
    mt = rollout_match(env, 32, (128, 128))
    bb1 = sum(1 << (c * 7) for c in range(3))                      # row 5 of columns 0-2
    bb2 = sum(1 << (c * 7 + 1) for c in range(3))                  # row 4
    mt.set_positions(bb1, bb2, 1)
    mt.step(3, 2)
    r = mt.results()
    mt.close()
    assert (r["moves"][0] == 3).all(), r["moves"][0]
    assert (r["length"] == 1).all() and (r["winner"] == 1).all() and r["running"] == 0


def test_more_playouts_win(env):
    """64 games per colour, rollout 128 against rollout 8, fresh trees: the stronger side scores at least 0.85 (the
    same match on the CPU oracle scores 0.97, tests/test_elo_cpu.py; 0.85 leaves more than five binomial standard
    deviations below that; a player that ignores its search scores 0.5)."""
    points = 0.0
    for strong_side, playouts, seeds in ((1, (128, 8), (1, 2)), (-1, (8, 128), (3, 4))):
        mt = rollout_match(env, 64, playouts, seeds)
        for _ in range(7):
            mt.step(3, 6)
            if mt.remaining() == 0:
                break
        r = mt.results()
        mt.close()
        assert r["running"] == 0
        points += float((r["winner"] == strong_side).sum()) + 0.5 * float((r["winner"] == 0).sum())
    print("rollout 128 against rollout 8 scores", points / 128)
    assert points / 128 >= 0.85, points / 128


# ---------------------------------------------------------------------------------------- R5

def test_python_side(env, monkeypatch):
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")          # batches this small: ask for the native loop (one call per step)
    M = env["M"]
    net = env["H"].HashEvaluator("cuda", salt=SALT)
    mt = M.EvaluationMatch(net, M.RolloutPlayer(32), 8, n_playout=16, vl_batch=4, eval_noise_eps=0.0, eval_temp=0.0,
                           fresh_trees=(False, True), record_moves=True, seed=3)
    assert mt.sides[1].fused is None and mt.native_models()[1] is None
    w = mt.play()
    res = mt.results()
    assert w.shape == (8,) and res["running"] == 0 and res["p1_wins"] + res["p2_wins"] + res["draws"] == 8
    moves = mt.moves()
    for g in range(8):                                             # a dead game plays nothing
        assert (moves[:res["length"][g], g] >= 0).all() and (moves[res["length"][g]:, g] == -1).all()
    first, second = M.rating_games(net, 4, 16, 32, vl_batch=4, seed=5)
    assert first.shape == second.shape == (4,) and set(np.unique(np.concatenate([first, second]))) <= {-1, 0, 1}
    one = M.rating_games(net, 1, 16, 32, vl_batch=4, seed=5)       # the reference's round
    assert one[0].shape == one[1].shape == (1,)
    from src.elo import Elo, rate
    a, b = rate(Elo(), first, second)
    assert a >= 1500 and b >= 1500
