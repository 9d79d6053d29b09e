"""Team play in the native match driver (az_match_create_teams, the team form of k_match_ply and k_match_team_roots in
csrc/match_kernels.hip, `EvaluationMatch(n_trees=, sym_ensemble=)` in src/match.py) on the GPU:

G1  az_match_team_roots against the restated symmetries (tests/team_harness.py, pinned to the reference by fixture G21
    in tests/test_team_cpu.py): every tree, both games, ensemble on and off;
G2  az_match_team_sample against numpy, exact: the summed row, the move, the per-tree moves, at T = 0 and (through
    az_match_sample on the summed row) at T = 0.2; one tree gives az_match_sample's bytes;
G3  the team match against the CPU oracle bit for bit, an ensemble for +1 only, for -1 only and for both;
G4  against the public entry points with everything random on: root-parallel network trees against root-parallel rollout
    trees, fresh trees, an ensemble that keeps its subtrees - moves, results and all counters after every ply;
G5  invariance: a plain team of deterministic trees plays the single-tree match; {1, 1, 0, 0} is az_match_create;
G6  argument checks, the begin / finish route with a team, a tape with -1 entries;
G7  rating_games with root-parallel and ensemble network sides: the engines' live configs.

Shapes: 19 Connect4 games (two full wavefronts of 8-lane groups and a partial one), 3 Othello games (a wavefront each).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import match_harness as MH
import scenarios as S
import team_harness as TH
from oracle import oracle as O
from test_match_gpu import C_INIT, DET, SALT, connect4_openings, dev_seed, hash_nets, othello_positions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
AZ_ERR_ARG = 1
GID = {"Connect4": 0, "Othello": 1}
N_GAMES = {"Connect4": 19, "Othello": 3}
N_PLAYOUT = {"Connect4": 24, "Othello": 16}
SINGLE = (1, False)


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import torch
    from src import MCTS_cpp, abi, fused, hash_eval, match
    return dict(torch=torch, W=MCTS_cpp, F=fused, H=hash_eval, M=match, A=abi, L=fused.lib())


class _OracleC4(O.BatchedMCTS_Connect4):
    """TEST ONLY: the oracle as the wrapper's native backend."""


class _OracleOthello(O.BatchedMCTS_Othello):
    """TEST ONLY: the oracle as the wrapper's native backend."""


def ensemble_of(game):
    return (len(TH.SYM_IDS[game]), True)


def dev_i32(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def dev_u64(env, a):
    return env["torch"].from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).cuda()


def host_u64(t):
    return t.cpu().numpy().view(np.uint64)


def positions_of(game, n):
    """n positions reached by the project's own game step: (boards int8, turns)."""
    rng = np.random.default_rng(11)
    return S.random_openings(rng, n, 20) if game == "Connect4" else S.ot_openings(rng, n, 30)


HOOK_TEAMS = {"Connect4": [SINGLE, (2, False), (2, True), (3, False)], "Othello": [SINGLE, (4, True), (3, False)]}


# ---------------------------------------------------------------------------------------- G1

@pytest.mark.parametrize("game", ["Connect4", "Othello"])
def test_team_roots_equal_the_restated_symmetries(env, game):
    torch, F, L = env["torch"], env["F"], env["L"]
    n = N_GAMES[game]
    boards, turns = positions_of(game, n)
    b1, b2 = TH.bitboards(boards, game)
    d1, d2, dt = dev_u64(env, b1), dev_u64(env, b2), dev_i32(env, turns)
    for team in HOOK_TEAMS[game]:
        trees, ens = team
        # sentinels around the outputs: the launch writes n * trees entries and nothing else
        o1 = torch.full((n * trees + 2,), -1, dtype=torch.int64, device="cuda")
        o2, ot = o1.clone(), torch.full((n * trees + 2,), 77, dtype=torch.int32, device="cuda")
        F.check(L.az_match_team_roots(GID[game], d1.data_ptr(), d2.data_ptr(), dt.data_ptr(), trees, int(ens),
                                      o1[1:].data_ptr(), o2[1:].data_ptr(), ot[1:].data_ptr(), n, F._stream()))
        torch.cuda.synchronize()
        w1, w2, wt = TH.team_root_bitboards(boards, turns, game, team)
        assert np.array_equal(host_u64(o1[1:-1]), w1), team
        assert np.array_equal(host_u64(o2[1:-1]), w2), team
        assert np.array_equal(ot[1:-1].cpu().numpy(), wt), team
        assert o1[0] == -1 and o1[-1] == -1 and o2[0] == -1 and o2[-1] == -1 and ot[0] == 77 and ot[-1] == 77
        if ens:                                            # the trees of an ensemble see different boards
            assert any(len({int(v) for v in row}) > 1 for row in (w1 | w2).reshape(n, trees))


# ---------------------------------------------------------------------------------------- G2

def team_count_rows(game, n, team, rng):
    """Count rows [n][trees][A].  In the GAME's frame (each tree holds its share at the action's index in its own frame):
    game 0 all zero; game 1 a tie after the sum between action 2 and the last action (Othello: the pass) and nothing
    else; game 2 random with the last action the strict maximum; the rest random, a third of the entries zero."""
    A = TH.ACTIONS[game]
    c = rng.integers(0, 40, (n, team[0], A)).astype(np.int32)
    c[rng.random((n, team[0], A)) < 0.33] = 0
    c[0] = 0
    c[1] = 0
    for j, s in enumerate(TH.team_syms(game, team)):
        c[1, j, TH.sym_action(2, s, game)] = 5 + j
        c[1, j, TH.sym_action(A - 1, s, game)] = 5 + j
        c[2, j, TH.sym_action(A - 1, s, game)] = 1000
    summed = TH.team_sum(c[1], game, team)[0]
    assert summed[2] == summed[A - 1] == summed.max() and summed.sum() == 2 * summed[2] > 0
    return c


@pytest.mark.parametrize("game", ["Connect4", "Othello"])
def test_team_sample_equals_numpy(env, game):
    torch, F, L = env["torch"], env["F"], env["L"]
    n, A, gid = N_GAMES[game], TH.ACTIONS[game], GID[game]
    rng = np.random.default_rng(3)
    seed, ply = dev_seed(7), 5
    out_teams = [ensemble_of(game), (3, False)]

    def sample(counts, team, temp, out_team=None, want_summed=True):
        trees, ens = team
        summed = torch.full((n + 1, A), -7, dtype=torch.int32, device="cuda")
        actions = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
        ot, oe = out_team or (1, False)
        tree_actions = torch.full((n * ot + 1,), -7, dtype=torch.int32, device="cuda")
        F.check(L.az_match_team_sample(gid, counts.data_ptr(), trees, int(ens), temp, seed, ply,
                                       summed.data_ptr() if want_summed else None, actions.data_ptr(), ot, int(oe),
                                       tree_actions.data_ptr() if out_team else None, n, F._stream()))
        torch.cuda.synchronize()
        assert actions[n] == -7 and tree_actions[n * ot] == -7 and (summed[n] == -7).all()      # nothing past the end
        return summed[:n].cpu().numpy(), actions[:n].cpu().numpy(), tree_actions[:n * ot].cpu().numpy()

    def plain_sample(rows, temp):
        actions = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        F.check(L.az_match_sample(gid, rows.data_ptr(), temp, seed, ply, actions.data_ptr(), n, F._stream()))
        torch.cuda.synchronize()
        return actions.cpu().numpy()

    for team in HOOK_TEAMS[game]:
        c = team_count_rows(game, n, team, rng)
        counts = dev_i32(env, c.reshape(n * team[0], A))
        want_sum = TH.team_sum(c.reshape(n * team[0], A), game, team)
        want_act = TH.pick(want_sum, 0.0)
        assert want_act[0] == 0 and want_act[1] == 2 and want_act[2] == A - 1       # empty row, first maximum, the last column
        for out_team in out_teams:
            summed, actions, tree_actions = sample(counts, team, 0.0, out_team)
            assert np.array_equal(summed, want_sum), (team, out_team)
            assert np.array_equal(actions, want_act), (team, out_team)
            assert np.array_equal(tree_actions, TH.team_actions(want_act, game, out_team)), (team, out_team)
        # without the optional outputs
        assert np.array_equal(sample(counts, team, 0.0, None, want_summed=False)[1], want_act)
        # T = 0.2: the pick of az_match_sample on the summed row, same seed and ply
        summed, actions, tree_actions = sample(counts, team, 0.2, out_teams[0])
        assert np.array_equal(summed, want_sum)
        want_drawn = plain_sample(dev_i32(env, want_sum), 0.2)
        assert np.array_equal(actions, want_drawn), team
        assert np.array_equal(tree_actions, TH.team_actions(want_drawn, game, out_teams[0]))
        assert all(want_sum[g, a] > 0 for g, a in enumerate(want_drawn) if g != 0) and want_drawn[0] == 0
        if team == SINGLE:                                 # one tree: az_match_sample byte for byte
            for temp in (0.0, 0.2, 1.0):
                assert sample(counts, team, temp)[1].tobytes() == plain_sample(counts, temp).tobytes()
    # the draws are keyed by the game, not by the tree: over many plies a drawn move is not always the arg-max
    c = team_count_rows(game, n, (3, False), rng)
    counts = dev_i32(env, c.reshape(n * 3, A))
    drawn = set()
    for ply in range(8):
        drawn |= {tuple(sample(counts, (3, False), 1.0)[1].tolist())}
    assert len(drawn) > 1


# ---------------------------------------------------------------------------------------- G3

_ORACLE = {}


def oracle_team_match(env, monkeypatch, game, teams):
    """tests/team_harness.py's loop on the oracle backend, once per case for the whole module."""
    key = (game, teams)
    if key in _ORACLE:
        return _ORACLE[key]
    n = N_GAMES[game]
    with monkeypatch.context() as mp:
        mp.setitem(env["W"]._BACKENDS, "Connect4", _OracleC4)
        mp.setitem(env["W"]._BACKENDS, "Othello", _OracleOthello)
        if game == "Connect4":
            from src.env_cpp.connect4 import Env
            kw = dict(openings=connect4_openings(n))
            nets = (env["H"].NumpyHashEvaluator(0), env["H"].NumpyHashEvaluator(SALT))
        else:
            from src.env_cpp.othello import Env
            kw = dict(positions=othello_positions(n))
            nets = (MH.OthelloNumpyHashEvaluator(0), MH.OthelloNumpyHashEvaluator(SALT))
        ws = [env["W"].BatchedMCTS(n * t[0], c_init=c, c_base=500, alpha=0.3, n_playout=N_PLAYOUT[game], game_name=game,
                                   noise_epsilon=0.0, use_symmetry=False) for c, t in zip(C_INIT, teams)]
        ref = TH.team_eval_games(ws[0], ws[1], nets[0], nets[1], Env, n, game, teams=teams, vl_batch=4, eval_temp=0.0, **kw)
        ref["positions"] = MH.env_bitboards(MH.start_envs(Env, n, **kw))
    _ORACLE[key] = ref
    return ref


def team_keywords(teams):
    return dict(n_trees=(teams[0][0], teams[1][0]), sym_ensemble=(teams[0][1], teams[1][1]))


def native_team_match(env, game, teams, ref, **kw):
    return env["M"].EvaluationMatch(*hash_nets(env, game), N_GAMES[game], n_playout=N_PLAYOUT[game], vl_batch=4, c_init=C_INIT,
                                    eval_temp=0.0, game=game, positions=ref["positions"], record_moves=True,
                                    **dict(DET, **team_keywords(teams)), **kw)


def check_against(mt, ref):
    res = mt.results()
    assert res["running"] == 0 and res["p1_wins"] + res["p2_wins"] + res["draws"] == mt.B
    assert np.array_equal(mt.moves(), MH.moves_table(ref["moves"], mt.MAX_PLIES))
    assert np.array_equal(res["winner"], ref["winner"]) and np.array_equal(res["length"], ref["length"])
    assert (res["p1_wins"], res["p2_wins"], res["draws"]) == tuple(int((ref["winner"] == v).sum()) for v in (1, -1, 0))


def games_that_differ(a, b):
    ta, tb = MH.moves_table(a["moves"], 126), MH.moves_table(b["moves"], 126)
    return sum(not np.array_equal(ta[:, i], tb[:, i]) for i in range(ta.shape[1]))


@pytest.mark.parametrize("game", ["Connect4", "Othello"])
@pytest.mark.parametrize("who", ["p1", "p2", "both"])
def test_team_match_equals_the_oracle(env, monkeypatch, game, who):
    E = ensemble_of(game)
    teams = {"p1": (E, SINGLE), "p2": (SINGLE, E), "both": (E, E)}[who]
    ref = oracle_team_match(env, monkeypatch, game, teams)
    # not vacuous, on the ORACLE alone: the ensemble changes at least a quarter of the single-tree match's games
    single = oracle_team_match(env, monkeypatch, game, (SINGLE, SINGLE))
    n = N_GAMES[game]
    assert 4 * games_that_differ(ref, single) >= n
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")          # batches this small: ask for the native loop
    mt = native_team_match(env, game, teams, ref)
    assert mt.native_models() is not None and mt.B == n
    assert [s.B for s in mt.sides] == [n * t[0] for t in teams]
    winners = mt.play()
    assert winners.dtype == np.int32 and winners.shape == (n,) and np.array_equal(winners, ref["winner"])
    check_against(mt, ref)


# ---------------------------------------------------------------------------------------- G4

def play_teams_by_public_calls(env, mt, temp, seed):
    """One match on the engines and models of `mt` (whose own match object stays unused) as a loop over the public entry
    points, in the driver's order.  Returns moves, winners, lengths, both engines' counters after every ply, and whether
    the trees of some running game ever held different counts."""
    torch, F, L = env["torch"], env["F"], env["L"]
    n, A, gid = mt.B, mt.A, mt.sides[0].game_id
    T, ens = mt.trees, mt.ensemble
    models = mt.native_models()
    assert models is not None
    z = dict(device="cuda")
    start = (0, 0) if gid == 0 else ((1 << 28) | (1 << 35), (1 << 27) | (1 << 36))
    bb1 = torch.full((n,), start[0], dtype=torch.int64, **z)
    bb2 = torch.full((n,), start[1], dtype=torch.int64, **z)
    turn = torch.ones(n, dtype=torch.int32, **z)
    aux = torch.zeros(n, dtype=torch.int32, **z)
    roots = [(torch.zeros(n * t, dtype=torch.int64, **z), torch.zeros(n * t, dtype=torch.int64, **z),
              torch.zeros(n * t, dtype=torch.int32, **z)) for t in T]
    counts = [torch.zeros((n * t, A), dtype=torch.int32, **z) for t in T]
    tree_actions = [torch.zeros(n * t, dtype=torch.int32, **z) for t in T]
    ones = [torch.ones(n * t, dtype=torch.uint8, **z) for t in T]
    actions = torch.zeros(n, dtype=torch.int32, **z)
    done = torch.zeros(n, dtype=torch.uint8, **z)
    win_now = torch.zeros(n, dtype=torch.int32, **z)
    dead = torch.zeros(n, dtype=torch.bool, **z)
    winner = torch.zeros(n, dtype=torch.int32, **z)
    length = torch.zeros(n, dtype=torch.int32, **z)
    moves, counters, diverged = [], [], False
    s = F._stream()
    hs = [side.h for side in mt.sides]
    for ply in range(mt.MAX_PLIES):
        if bool(dead.all()):
            break
        m = 0 if ply % 2 == 0 else 1
        r1, r2, rt = roots[m]
        F.check(L.az_match_team_roots(gid, bb1.data_ptr(), bb2.data_ptr(), turn.data_ptr(), T[m], int(ens[m]), r1.data_ptr(),
                                      r2.data_ptr(), rt.data_ptr(), n, s))
        F.check(L.az_mcts_dev_set_roots(hs[m], r1.data_ptr(), r2.data_ptr(), rt.data_ptr(), s))
        if (mt.fresh_trees >> m) & 1:
            F.check(L.az_mcts_dev_reset_masked(hs[m], ones[m].data_ptr(), s))
        if models[m] is not None:
            F.check(L.az_mcts_dev_search(hs[m], models[m], mt.sides[m].n_playout, mt.vl_batch, 0, s))
        else:
            F.check(L.az_mcts_dev_rollout_search(hs[m], mt.sides[m].n_playout, 0, s))
        F.check(L.az_mcts_dev_counts(hs[m], counts[m].data_ptr(), s))
        for e in range(2):
            F.check(L.az_match_team_sample(gid, counts[m].data_ptr(), T[m], int(ens[m]), temp, dev_seed(seed), ply, None,
                                           actions.data_ptr(), T[e], int(ens[e]), tree_actions[e].data_ptr(), n, s))
        actions.masked_fill_(dead, -1)                  # a finished game is dead: action -1 to every tree of both engines
        for e in range(2):
            tree_actions[e].masked_fill_(dead.repeat_interleave(T[e]), -1)
            F.check(L.az_mcts_dev_prune_roots(hs[e], tree_actions[e].data_ptr(), s))
        F.check(L.az_game_dev_step(gid, bb1.data_ptr(), bb2.data_ptr(), turn.data_ptr(), aux.data_ptr(), actions.data_ptr(),
                                   done.data_ptr(), win_now.data_ptr(), n, 0, s))
        masks = [done.repeat_interleave(T[e]).contiguous() for e in range(2)]
        for e in range(2):
            F.check(L.az_mcts_dev_reset_masked(hs[e], masks[e].data_ptr(), s))
        c = counts[m].view(n, T[m], A)[~dead]
        diverged = diverged or bool((c != c[:, :1]).any())
        length += (~dead).to(torch.int32)
        winner = torch.where(done.bool(), win_now, winner)
        dead |= done.bool()
        moves.append(actions.cpu().numpy().copy())
        counters.append(tuple(F.counters(h) for h in hs))
    return np.array(moves, np.int32), winner.cpu().numpy(), length.cpu().numpy(), counters, diverged


# name: (game, network side, rollout side, n_games, network trees, ensemble, rollout trees, noise, fresh_trees, playouts)
PUBLIC_CASES = {
    "c4_root_parallel": ("Connect4", 0, 1, 8, 3, False, 2, 0.05, False, (16, 24)),
    "c4_fresh_trees": ("Connect4", 1, 0, 8, 3, False, 2, 0.05, True, (16, 24)),
    "ot_ensemble_keeps_subtrees": ("Othello", 0, 1, 3, 1, True, 2, 0.0, False, (12, 16)),
}


@pytest.mark.parametrize("name", sorted(PUBLIC_CASES))
def test_team_match_equals_the_public_entry_points(env, monkeypatch, name):
    game, net_side, _, n, trees, ensemble, rollout_trees, eps, fresh, playouts = PUBLIC_CASES[name]
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")
    net = (env["H"].HashEvaluator if game == "Connect4" else env["H"].OthelloHashEvaluator)("cuda", salt=SALT)
    players = [None, None]
    players[net_side], players[1 - net_side] = net, env["M"].RolloutPlayer(playouts[1], 1.0, n_trees=rollout_trees)
    kw = dict(n_playout=playouts[0], vl_batch=4, c_init=1.4, c_base=500, alpha=0.3, eval_noise_eps=eps, eval_temp=0.2,
              use_symmetry=True, seed=7, game=game, record_moves=True, fresh_trees=fresh, n_trees=trees, sym_ensemble=ensemble)
    nat = env["M"].EvaluationMatch(players[0], players[1], n, **kw)
    want_trees = [0, 0]
    want_trees[net_side], want_trees[1 - net_side] = (len(TH.SYM_IDS[game]) if ensemble else trees), rollout_trees
    assert list(nat.trees) == want_trees and nat.ensemble[net_side] == ensemble and not nat.ensemble[1 - net_side]
    nat_counters = []
    while nat.remaining() > 0:
        nat.step(1)
        nat_counters.append(nat.engine_counters())
    by_hand = env["M"].EvaluationMatch(players[0], players[1], n, **kw)
    moves, winner, length, counters, diverged = play_teams_by_public_calls(env, by_hand, 0.2, 7)
    res = nat.results()
    assert np.array_equal(nat.moves(), MH.moves_table(moves, nat.MAX_PLIES))
    assert np.array_equal(res["winner"], winner) and np.array_equal(res["length"], length)
    assert res["running"] == 0 and len({tuple(moves[:, i]) for i in range(n)}) > n // 2
    assert len(nat_counters) == len(counters)
    for p, (a, b) in enumerate(zip(nat_counters, counters)):
        assert a == b, p
    # the trees of a game are not copies of each other: noise and playouts are drawn per tree, an ensemble's frames differ
    assert diverged


# ---------------------------------------------------------------------------------------- G5

def test_a_plain_deterministic_team_plays_the_single_tree_match(env, monkeypatch):
    single = oracle_team_match(env, monkeypatch, "Connect4", (SINGLE, SINGLE))
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")
    mt = native_team_match(env, "Connect4", ((3, False), (2, False)), single)
    mt.play()
    check_against(mt, single)
    # and the harness says the same of the oracle
    assert games_that_differ(oracle_team_match(env, monkeypatch, "Connect4", ((3, False), (2, False))), single) == 0


def raw_engine(env, game_id, n, seed, noise=0.25, symmetry=1):
    L = env["L"]
    h = C.c_void_p()
    assert L.az_mcts_create(game_id, n, -1, C.byref(h)) == 0, L.az_last_error()
    cfg = L.az_mcts_config(h).contents
    cfg.c_init, cfg.c_base, cfg.dirichlet_alpha, cfg.noise_epsilon, cfg.use_symmetry = 1.4, 500.0, 0.3, noise, symmetry
    assert L.az_mcts_set_seed(h, seed) == 0
    return h


def test_teams_of_one_are_az_match_create(env):
    L, A = env["L"], env["A"]
    n = 19
    m1, m2 = C.c_void_p(), C.c_void_p()
    assert L.az_nn_model_create_hash_salted(0, 0, C.byref(m1)) == 0 and L.az_nn_model_create_hash_salted(0, SALT, C.byref(m2)) == 0
    runs = []
    for with_teams in (False, True):
        e1, e2, mt = raw_engine(env, 0, n, 3), raw_engine(env, 0, n, 4), C.c_void_p()
        cfg = A.MatchConfig(0.2, 1)
        if with_teams:
            teams = A.MatchTeams(1, 1, 0, 0)
            assert L.az_match_create_teams(e1, e2, C.byref(cfg), C.byref(teams), C.byref(mt)) == 0, L.az_last_error()
        else:
            assert L.az_match_create(e1, e2, C.byref(cfg), C.byref(mt)) == 0, L.az_last_error()
        counters, left = [], C.c_int64(n)
        for _ in range(42):
            assert L.az_match_step(mt, m1, m2, 16, 4, 0, 1, None) == 0, L.az_last_error()
            counters.append(tuple(env["F"].counters(e) for e in (e1, e2)))
            assert L.az_match_remaining(mt, C.byref(left)) == 0
            if left.value == 0:
                break
        assert left.value == 0
        moves, winner = np.zeros((42, n), np.int32), np.zeros(n, np.int32)
        assert L.az_match_moves(mt, moves.ctypes.data) == 0 and L.az_match_results(mt, winner.ctypes.data, None, None) == 0
        runs.append((moves, winner, counters))
        L.az_match_destroy(mt)
        L.az_mcts_destroy(e1); L.az_mcts_destroy(e2)
    L.az_nn_model_destroy(m1); L.az_nn_model_destroy(m2)
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])
    assert runs[0][2] == runs[1][2]
    assert len({tuple(runs[0][0][:, i]) for i in range(n)}) > n // 2


# ---------------------------------------------------------------------------------------- G6

def test_argument_checks(env):
    L, A = env["L"], env["A"]
    c8, c9, c12, same9, ot8 = (raw_engine(env, 0, 8, 0), raw_engine(env, 0, 9, 1), raw_engine(env, 0, 12, 2), raw_engine(env, 0, 9, 3),
                               raw_engine(env, 1, 8, 4))
    cfg, mt = A.MatchConfig(0.0, 1), C.c_void_p()

    def create(e1, e2, teams, c=cfg, out=mt):
        t = C.byref(A.MatchTeams(*teams)) if teams is not None else None
        return L.az_match_create_teams(e1, e2, C.byref(c) if c is not None else None, t, C.byref(out) if out is not None else None)
    bad = [
        (None, c9, (1, 1, 0, 0)), (c9, None, (1, 1, 0, 0)), (c9, same9, None),               # null arguments
        (c9, same9, (0, 1, 0, 0)), (c9, same9, (1, -2, 0, 0)),                               # a tree count below 1
        (c9, c8, (2, 2, 0, 0)),                                                              # 9 trees in teams of 2
        (c8, c9, (2, 1, 0, 0)), (c8, c12, (2, 2, 0, 0)), (c9, c8, (1, 1, 0, 0)),             # unequal game counts
        (c9, c9, (1, 1, 0, 0)), (c8, ot8, (1, 1, 0, 0)),                                     # what az_match_create refuses
        (c12, c8, (3, 2, 1, 0)), (c8, c12, (2, 3, 0, 1)),                                    # Connect4's ensemble is two trees
        (ot8, ot8, (2, 2, 1, 1)),
    ]
    for e1, e2, teams in bad:
        assert create(e1, e2, teams) == AZ_ERR_ARG, teams
    assert create(c9, same9, (1, 1, 0, 0), c=None) == AZ_ERR_ARG and create(c9, same9, (1, 1, 0, 0), out=None) == AZ_ERR_ARG
    assert L.az_match_create(c9, c8, C.byref(cfg), C.byref(mt)) == AZ_ERR_ARG
    # 12 trees in teams of 3 against 8 in an ensemble: four games
    assert create(c12, c8, (3, 2, 0, 1)) == 0, L.az_last_error()
    left = C.c_int64()
    assert L.az_match_remaining(mt, C.byref(left)) == 0 and left.value == 4
    winner, length, totals = np.full(5, 9, np.int32), np.full(5, 9, np.int32), (C.c_int64 * 4)()
    assert L.az_match_results(mt, winner.ctypes.data, length.ctypes.data, C.byref(totals)) == 0
    assert list(totals) == [0, 0, 0, 4] and winner.tolist() == [0, 0, 0, 0, 9] and length.tolist() == [0, 0, 0, 0, 9]
    L.az_match_destroy(mt)
    for e in (c8, c9, c12, same9, ot8):
        L.az_mcts_destroy(e)


def test_begin_finish_route_with_a_team(env, monkeypatch):
    """az_match_begin_ply / az_match_finish_ply around FusedSearch (no native model object: AZ_FUSED_NATIVE=0): the
    caller searches the mover's engine over all its trees."""
    teams = (ensemble_of("Connect4"), SINGLE)
    ref = oracle_team_match(env, monkeypatch, "Connect4", teams)
    monkeypatch.setenv("AZ_FUSED_NATIVE", "0")
    mt = native_team_match(env, "Connect4", teams, ref)
    assert mt.native_models() is None
    assert np.array_equal(mt.play(), ref["winner"])
    check_against(mt, ref)


def test_a_tape_with_idle_entries(env, monkeypatch):
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")
    tape = np.array([[3, 3, -1, 2], [3, -1, -1, 2], [3, 3, -1, 0], [2, 3, 6, -1]], np.int32)
    mt = env["M"].EvaluationMatch(*hash_nets(env, "Connect4"), 4, n_playout=8, vl_batch=4, record_moves=True, n_trees=(2, 3),
                                  sym_ensemble=(True, False))
    assert [s.B for s in mt.sides] == [8, 12]
    mt.set_action_tape(tape)
    mt.step(4)
    res = mt.results()
    assert res["running"] == 4 and res["length"].tolist() == [4, 3, 1, 3] and (res["winner"] == 0).all()
    assert np.array_equal(mt.moves(), MH.moves_table(tape, 42))
    mt.set_action_tape(None)                           # the pick takes over, in every game
    mt.step(1)
    assert mt.results()["length"].tolist() == [5, 4, 2, 4]
    with pytest.raises(AssertionError):                # a tape row has one entry per GAME
        mt.set_action_tape(np.zeros((2, 8), np.int32))


# ---------------------------------------------------------------------------------------- G7

def test_rating_games_with_teams(env, monkeypatch):
    M, L = env["M"], env["L"]
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")
    made = []

    class Recording(M.EvaluationMatch):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    monkeypatch.setattr(M, "EvaluationMatch", Recording)
    net = env["H"].HashEvaluator("cuda", salt=SALT)

    def live(mt):
        """per side: (trees in the engine, live noise epsilon, live use_symmetry, is a network side)"""
        out = []
        for s in mt.sides:
            cfg = L.az_mcts_config(s.h).contents
            out.append((L.az_mcts_num_envs(s.h), round(float(cfg.noise_epsilon), 6), int(cfg.use_symmetry), s.fused is not None))
        return out

    first, second = M.rating_games(net, 4, 16, 24, n_trees=2, rollout_trees=3, seed=5)
    assert first.shape == second.shape == (4,) and len(made) == 2
    assert live(made[0]) == [(8, 0.05, 1, True), (12, 0.0, 0, False)]
    assert live(made[1]) == [(12, 0.0, 0, False), (8, 0.05, 1, True)]
    assert all(mt.results()["running"] == 0 and mt.fresh_trees == 3 for mt in made)
    assert made[0].trees == (2, 3) and made[1].trees == (3, 2) and made[0].ensemble == (False, False)
    del made[:]
    first, second = M.rating_games(net, 4, 16, 24, sym_ensemble=True, seed=5)
    assert live(made[0]) == [(8, 0.0, 0, True), (4, 0.0, 0, False)]
    assert live(made[1]) == [(4, 0.0, 0, False), (8, 0.0, 0, True)]
    assert made[0].ensemble == (True, False) and made[1].ensemble == (False, True)
    assert all(mt.results()["running"] == 0 for mt in made)
    assert set(first.tolist()) | set(second.tolist()) <= {1, -1, 0}
    del made[:]
    # the caller's own noise wins
    M.rating_games(net, 4, 16, 24, n_trees=2, eval_noise_eps=0.1, seed=5)
    assert live(made[0])[0] == (8, 0.1, 1, True)
    # select_best passes the keywords through
    del made[:]
    ok, rate = M.select_best(net, env["H"].HashEvaluator("cuda", salt=0), 8, 0.5, n_playout=16, sym_ensemble=(True, False), seed=5)
    assert isinstance(ok, bool) and 0.0 <= rate <= 1.0
    assert [mt.trees for mt in made] == [(2, 1), (2, 1)] and all(mt.B == 4 for mt in made)
