"""Team play in the native self-play driver (az_selfplay_create_teams, the team form of k_sp_pick, k_team_root_stats in
csrc/selfplay_kernels.hip, `NativeSelfPlay(n_trees=, sym_ensemble=)` in src/selfplay.py, `team_root_stats` in src/match.py)
on the GPU:

T1  az_selfplay_team_sample against numpy, exact: the summed row, the move, the per-tree moves; at T = 0 and T = 1 the move
    is az_selfplay_sample's on the summed row with the same (seed, call) - the draws are keyed by the game; one tree gives
    az_selfplay_sample's bytes;
T2  az_mcts_dev_team_root_stats against fixture G22 (what the reference's inverse_sym_stats gave), compared as uint32, also
    with the fixture's games tiled to n = 9 and n = 70;
T3  the driver against the harness on the CPU oracle bit for bit: ensemble teams in both games and a root-parallel team of
    3, openings from a tape, then the picks, recording on; export() equals store_games(drain()) of an identical run;
T4  drawn moves (T = 1) with refill: the drained games replayed as a tape through the harness give the same rows; slots,
    totals, and every tree of a refilled game starts empty;
T5  noise_steps > 0 with a team of 2: the oracle's root noise replayed through az_mcts_dev_replay, the harness sets the
    epsilon per ply as game.py:87-91 does; counts bit-equal after every ply for every tree;
T6  everything random on (alpha 0.3, epsilon 0.25, root-parallel 3): the loop over the public entry points reproduces the
    driver's positions and every engine counter after every ply;
T7  {1, 0} is az_selfplay_create; the begin / finish route with a team; StreamedSelfPlay with teams; argument checks.

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
import team_selfplay_harness as TS
from oracle import oracle as O
from test_match_gpu import SALT, dev_seed
from test_team_match_gpu import HOOK_TEAMS, SINGLE, dev_i32, raw_engine, team_count_rows

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
G22 = os.path.join(ROOT, "tests", "golden", "g22_team_stats.npz")
AZ_ERR_ARG = 1
GID = {"Connect4": 0, "Othello": 1}
N_GAMES = {"Connect4": 19, "Othello": 3}
N_PLAYOUT = {"Connect4": 24, "Othello": 16}
TAPE_PLIES = {"Connect4": 4, "Othello": 2}
MAX_PLIES = {"Connect4": 42, "Othello": 126}
# the search of every driver below and of the harness's wrapper
SEARCH = dict(c_init=1.4, c_base=500, alpha=0.3, fpu_reduction=0.2, mlh_slope=0.1, mlh_cap=0.2, value_decay=1.0,
              score_utility_factor=0.0, score_scale=8.0)


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import torch
    from src import MCTS_cpp, abi, fused, hash_eval, match, replay, selfplay
    return dict(torch=torch, W=MCTS_cpp, F=fused, H=hash_eval, M=match, A=abi, SP=selfplay, RP=replay, L=fused.lib())


class _OracleC4(O.BatchedMCTS_Connect4):
    """TEST ONLY: the oracle as the wrapper's native backend."""


class _OracleOthello(O.BatchedMCTS_Othello):
    """TEST ONLY: the oracle as the wrapper's native backend."""


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def team_keywords(team):
    return dict(n_trees=team[0], sym_ensemble=team[1])


def hash_net(env, game, salt=SALT):
    return (env["H"].HashEvaluator if game == "Connect4" else env["H"].OthelloHashEvaluator)("cuda", salt=salt)


def numpy_net(env, game, salt=SALT):
    return env["H"].NumpyHashEvaluator(salt) if game == "Connect4" else MH.OthelloNumpyHashEvaluator(salt)


def opening_tape(game, n, plies):
    """[plies][n]: n distinct openings of `plies` random legal moves each from the initial position."""
    rng = np.random.default_rng(5)
    rows, seen = [], set()
    while len(rows) < n:
        b, t, seq = (np.zeros((6, 7), np.int8) if game == "Connect4" else S.ot_start()), 1, []
        for _ in range(plies):
            if game == "Connect4":
                a = int(rng.choice(S.np_valid(b)))
                S.np_drop(b, a, t)
            else:
                a = int(rng.choice(S.ot_moves(b, t)))
                S.ot_play(b, t, a)
            seq.append(a)
            t = -t
        if b.tobytes() not in seen:
            seen.add(b.tobytes())
            rows.append(seq)
    return np.array(rows, np.int32).T.copy()


# ---------------------------------------------------------------------------------------- T1

def sp_config(env, temperature, temp_endgame=0.0, temp_decay_moves=0):
    return env["A"].SelfPlayConfig(temperature, temp_endgame, temp_decay_moves, 0, 0, 0, 0, 0.25, 0.1)


@pytest.mark.parametrize("game", ["Connect4", "Othello"])
def test_team_sample_equals_numpy(env, game):
    torch, F, L = env["torch"], env["F"], env["L"]
    n, A, gid = N_GAMES[game], TH.ACTIONS[game], GID[game]
    rng = np.random.default_rng(3)
    seed, call = dev_seed(7), 5
    ply = torch.zeros(n, dtype=torch.int32, device="cuda")

    def team_sample(counts, team, temp, want_summed=True, want_tree=True, call=call):
        trees, ens = team
        summed = torch.full((n + 1, A), -7, dtype=torch.int32, device="cuda")
        actions = torch.full((n + 1,), -7, dtype=torch.int32, device="cuda")
        tree_actions = torch.full((n * trees + 1,), -7, dtype=torch.int32, device="cuda")
        cfg = sp_config(env, temp)
        F.check(L.az_selfplay_team_sample(gid, counts.data_ptr(), ply.data_ptr(), C.byref(cfg), trees, int(ens), seed, call,
                                          summed.data_ptr() if want_summed else None, actions.data_ptr(),
                                          tree_actions.data_ptr() if want_tree else None, n, F._stream()))
        torch.cuda.synchronize()
        assert actions[n] == -7 and tree_actions[n * trees] == -7 and (summed[n] == -7).all()      # nothing past the end
        if not want_summed:
            assert (summed == -7).all()
        if not want_tree:
            assert (tree_actions == -7).all()
        return summed[:n].cpu().numpy(), actions[:n].cpu().numpy(), tree_actions[:n * trees].cpu().numpy()

    def plain_sample(rows, temp, call=call):
        actions = torch.full((n,), -7, dtype=torch.int32, device="cuda")
        cfg = sp_config(env, temp)
        F.check(L.az_selfplay_sample(gid, rows.data_ptr(), ply.data_ptr(), C.byref(cfg), seed, call, actions.data_ptr(), n,
                                     F._stream()))
        torch.cuda.synchronize()
        return actions.cpu().numpy()

    for team in HOOK_TEAMS[game]:
        # game 0 empty, game 1 a tie whose first maximum (action 2) only shows once every tree's row is read through its
        # symmetry, game 2 the last action
        c = team_count_rows(game, n, team, rng)
        counts = dev_i32(env, c.reshape(n * team[0], A))
        want_sum = TH.team_sum(c.reshape(n * team[0], A), game, team)
        want_act = TH.pick(want_sum, 0.0)
        assert want_act[0] == 0 and want_act[1] == 2 and want_act[2] == A - 1
        summed, actions, tree_actions = team_sample(counts, team, 0.0)
        assert np.array_equal(summed, want_sum), team
        assert np.array_equal(actions, want_act), team
        assert np.array_equal(tree_actions, TH.team_actions(want_act, game, team)), team
        assert np.array_equal(team_sample(counts, team, 0.0, want_summed=False, want_tree=False)[1], want_act)
        for temp in (0.0, 1.0):                            # the pick of az_selfplay_sample on the summed row: keyed by game
            summed, actions, tree_actions = team_sample(counts, team, temp)
            want = plain_sample(dev_i32(env, want_sum), temp)
            assert np.array_equal(actions, want), (team, temp)
            assert np.array_equal(tree_actions, TH.team_actions(want, game, team)), (team, temp)
            assert all(want_sum[g, a] > 0 for g, a in enumerate(want) if g != 0) and want[0] == 0
        if team == SINGLE:                                 # one tree: az_selfplay_sample byte for byte
            for temp in (0.0, 0.5, 1.0):
                assert team_sample(counts, team, temp)[1].tobytes() == plain_sample(counts, temp).tobytes()
    # drawn, not the arg-max every time, and the temperature schedule reads the GAME's ply
    c = team_count_rows(game, n, (3, False), rng)
    counts = dev_i32(env, c.reshape(n * 3, A))
    assert len({tuple(team_sample(counts, (3, False), 1.0, call=k)[1].tolist()) for k in range(8)}) > 1
    ply[n // 2:] = 9
    cfg = sp_config(env, 1.0, 0.0, 8)
    actions = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    F.check(L.az_selfplay_team_sample(gid, counts.data_ptr(), ply.data_ptr(), C.byref(cfg), 3, 0, seed, call, None,
                                      actions.data_ptr(), None, n, F._stream()))
    torch.cuda.synchronize()
    greedy = TH.pick(TH.team_sum(c.reshape(n * 3, A), game, (3, False)), 0.0)
    assert np.array_equal(actions.cpu().numpy()[n // 2:], greedy[n // 2:])


# ---------------------------------------------------------------------------------------- T2

STATS_CASES = [("c4_real", "Connect4"), ("c4_real_salted", "Connect4"), ("ot_real", "Othello"), ("ot_real_salted", "Othello"),
               ("c4_rand_ens", "Connect4"), ("ot_rand_ens", "Othello"), ("c4_rand_3", "Connect4"), ("c4_rand_7", "Connect4"),
               ("ot_rand_3", "Othello"), ("ot_rand_7", "Othello"), ("c4_sp_ens", "Connect4"), ("ot_sp_ens", "Othello")]


@pytest.mark.parametrize("name,game", STATS_CASES)
def test_team_root_stats_kernel_equals_the_reference(env, name, game):
    torch, M = env["torch"], env["M"]
    g = np.load(G22)
    stats, want = g[name + "_stats"], g[name + "_merged"]
    trees = stats.shape[1]
    ens = bool(g[name + "_team"][1]) if name + "_team" in g.files else bool(g[name + "_settings"][0])
    n0, width = stats.shape[0], stats.shape[2]
    for n in (n0, 9, 70):                                  # one partial wavefront; more games than a block's groups
        pick = np.arange(n) % n0
        rows = torch.from_numpy(np.ascontiguousarray(stats[pick].reshape(n * trees, width))).cuda()
        padded = torch.full((n + 2, width), -7.0, dtype=torch.float32, device="cuda")
        F, L = env["F"], env["L"]
        F.check(L.az_mcts_dev_team_root_stats(GID[game], rows.data_ptr(), trees, int(ens), padded[1:].data_ptr(), n, F._stream()))
        torch.cuda.synchronize()
        assert (padded[0] == -7).all() and (padded[-1] == -7).all()                  # n rows and nothing else
        assert np.array_equal(u32(padded[1:-1].cpu().numpy()), u32(want[pick])), n
        got = M.team_root_stats(rows, game, trees, ensemble=ens)                      # a GPU tensor: the kernel route
        assert got.is_cuda and np.array_equal(u32(got.cpu().numpy()), u32(want[pick])), n
        assert np.array_equal(u32(M.team_root_stats(rows, game, trees, ensemble=ens, route="torch").cpu().numpy()), u32(want[pick]))


# ---------------------------------------------------------------------------------------- T3

_ORACLE = {}


def oracle_selfplay(env, monkeypatch, game, team, tape=None, **kw):
    """tests/team_selfplay_harness.py's loop on the oracle backend (deterministic search), once per case for the module."""
    key = (game, team, None if tape is None else tape.tobytes(), tuple(sorted(kw.items())))
    if key in _ORACLE:
        return _ORACLE[key]
    n = N_GAMES[game]
    with monkeypatch.context() as mp:
        mp.setitem(env["W"]._BACKENDS, "Connect4", _OracleC4)
        mp.setitem(env["W"]._BACKENDS, "Othello", _OracleOthello)
        if game == "Connect4":
            from src.env_cpp.connect4 import Env
        else:
            from src.env_cpp.othello import Env
        w = env["W"].BatchedMCTS(n * team[0], n_playout=N_PLAYOUT[game], game_name=game, noise_epsilon=0.0, use_symmetry=False,
                                 **SEARCH)
        ref = TS.team_selfplay_games(w, numpy_net(env, game), Env, n, game, team, vl_batch=4,
                                     tape=opening_tape(game, n, TAPE_PLIES[game]) if tape is None else tape, **kw)
    _ORACLE[key] = ref
    return ref


def native_selfplay(env, game, team, **kw):
    args = dict(n_playout=N_PLAYOUT[game], vl_batch=4, noise_epsilon=0.0, use_symmetry=False, temperature=0.0, temp_endgame=0.0,
                temp_decay_moves=0, seed=5, record=True, refill=False, sampler="tape", game=game, **SEARCH)
    args.update(team_keywords(team))
    args.update(kw)
    return env["SP"].NativeSelfPlay(hash_net(env, game), N_GAMES[game], **args)


def check_drained(per_game, per_row, finished, game):
    """az_selfplay_drain's arrays against the harness's finished games: order, figures, every row, floats as uint32."""
    A = TH.ACTIONS[game]
    assert len(per_game["slot"]) == len(finished)
    at = 0
    for k, g in enumerate(finished):
        T = g["length"]
        assert (int(per_game["slot"][k]), int(per_game["length"][k]), int(per_game["winner"][k]), int(per_game["finish_ply"][k]),
                int(per_game["row_start"][k])) == (g["slot"], T, g["winner"], g["finish_ply"], at), k
        b1, b2 = TH.bitboards(np.array(g["board"], np.int8), game)
        rows = slice(at, at + T)
        assert np.array_equal(per_row["bb_p1"][rows], np.asarray(b1, np.uint64)) and np.array_equal(per_row["bb_p2"][rows], np.asarray(b2, np.uint64)), k
        assert per_row["turn"][rows].tolist() == g["turn"], k
        assert (int(per_row["bb_p1"][at + T]), int(per_row["bb_p2"][at + T]), int(per_row["turn"][at + T])) == g["end"], k
        assert np.array_equal(u32(per_row["prob"][rows]), u32(np.array(g["prob"]))), k
        assert np.array_equal(u32(per_row["wdl"][rows]), u32(np.array(g["wdl"]))), k
        assert np.array_equal(per_row["mask"][rows], np.array(g["mask"], np.uint8)), k
        assert not per_row["prob"][at + T].any() and not per_row["wdl"][at + T].any() and not per_row["mask"][at + T].any()
        assert per_row["prob"].shape[1] == A
        at += T + 1
    assert at == len(per_row["turn"])


def games_that_differ(a, b):
    moves = [{g["slot"]: g["moves"] for g in r["finished"]} for r in (a, b)]
    return sum(moves[0][s] != moves[1][s] for s in moves[0])


@pytest.mark.parametrize("game,team", [("Connect4", (2, True)), ("Othello", (4, True)), ("Connect4", (3, False))])
def test_team_selfplay_equals_the_oracle(env, monkeypatch, game, team):
    n = N_GAMES[game]
    ref = oracle_selfplay(env, monkeypatch, game, team)
    assert len(ref["finished"]) == n and ref["plies"] <= MAX_PLIES[game]
    single = oracle_selfplay(env, monkeypatch, game, SINGLE)
    if team[1]:        # not vacuous, on the ORACLE alone: the ensemble changes at least a quarter of the single-tree games
        assert 4 * games_that_differ(ref, single) >= n
    else:              # deterministic trees of one root are copies of each other
        assert games_that_differ(ref, single) == 0
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")          # batches this small: ask for the native loop
    tape = opening_tape(game, n, TAPE_PLIES[game])
    runs = []
    for _ in range(2):
        sp = native_selfplay(env, game, team)
        assert sp.fused._native_model() is not None and sp.B == n and sp.n_envs == n * team[0] == sp.search.batch_size
        assert env["L"].az_mcts_num_envs(sp.h) == n * team[0] and not sp.search.mcts.config.use_symmetry
        sp.set_action_tape(tape)
        sp.step(len(tape))
        sp.set_action_tape(None)                       # the picks take over
        sp.step(ref["plies"] - len(tape))
        assert sp.finished()[0] == n and sp.finished()[2] == 0
        tot = sp.read_totals()
        assert tot["positions"] == n * ref["plies"] and tot["games"] == n
        assert (tot["p1_wins"], tot["p2_wins"], tot["draws"]) == tuple(sum(g["winner"] == v for g in ref["finished"]) for v in (1, -1, 0))
        runs.append(sp)
    # drain(): the raw arrays it reads against the harness, the assembled games into a host buffer
    raw = []
    real = env["SP"].drain_native
    monkeypatch.setattr(env["SP"], "drain_native", lambda *a: raw.append(real(*a)) or raw[-1])
    games = runs[0].drain()
    check_drained(raw[0][0], raw[0][1], ref["finished"], game)
    assert runs[0].finished()[:2] == (0, 0)
    assert [g[2] for g in games] == [g["slot"] for g in ref["finished"]] and all(len(g[1]) == r["length"] + 1 for g, r in zip(games, ref["finished"]))
    # export() of the identical second run equals the host route over that drain()
    from test_replay_export_gpu import same_buffers
    dev, host = env["RP"].ReplayTensors(game, 997, "cuda"), env["RP"].ReplayTensors(game, 997, "cpu")
    host.store_games(games)
    info = runs[1].export(dev)
    assert info["slot"].tolist() == [g["slot"] for g in ref["finished"]] and info["length"].tolist() == [g["length"] for g in ref["finished"]]
    same_buffers(dev, host)


# ---------------------------------------------------------------------------------------- T4

def move_between(game, before, after):
    """The move that leads from one position (bb_p1, bb_p2) to the next: the square that became occupied."""
    new = (int(after[0]) | int(after[1])) & ~(int(before[0]) | int(before[1]))
    if game == "Connect4":
        assert bin(new).count("1") == 1
        return (new.bit_length() - 1) // 7
    assert bin(new).count("1") <= 1
    return new.bit_length() - 1 if new else 64


@pytest.mark.parametrize("game,team", [("Connect4", (2, True)), ("Othello", (4, True))])
def test_drawn_moves_and_refill(env, monkeypatch, game, team):
    torch, F, L = env["torch"], env["F"], env["L"]
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")
    n, A, trees = N_GAMES[game], TH.ACTIONS[game], team[0]
    plies = 30 if game == "Connect4" else 70
    sp = native_selfplay(env, game, team, temperature=1.0, refill=True, sampler="device", seed=11)
    model = sp.fused._native_model()
    stats = torch.zeros((n * trees, 6 + 8 * A), dtype=torch.float32, device="cuda")
    s = F._stream()
    snaps, root_n = [sp.positions()], []
    for _ in range(plies):
        F.check(L.az_selfplay_begin_ply(sp._sp, s))
        F.check(L.az_mcts_dev_search(sp.h, model, sp.n_playout, 4, 0, s))
        F.check(L.az_mcts_dev_root_stats(sp.h, stats.data_ptr(), s))
        F.check(L.az_selfplay_finish_ply(sp._sp, s))
        snaps.append(sp.positions())                   # synchronises
        root_n.append(stats[:, 0].cpu().numpy().reshape(n, trees).copy())
    tot = sp.read_totals()
    assert tot["positions"] == n * plies and tot["games"] >= n // 2 and tot["games"] == sp.finished()[0]
    per_game, per_row = env["SP"].drain_native(L, sp._sp, A)
    assert (per_game["slot"] < n).all() and (per_game["slot"] >= 0).all() and len(set(per_game["slot"].tolist())) > 1
    # the moves of every ply: a game that ended on ply p shows them in its last two rows, the others in the positions
    ended = {(int(p), int(sl)): k for k, (p, sl) in enumerate(zip(per_game["finish_ply"], per_game["slot"]))}
    tape = np.zeros((plies, n), np.int32)
    for p in range(plies):
        for i in range(n):
            if (p, i) in ended:
                k = ended[p, i]
                r = int(per_game["row_start"][k]) + int(per_game["length"][k])
                before, after = (per_row["bb_p1"][r - 1], per_row["bb_p2"][r - 1]), (per_row["bb_p1"][r], per_row["bb_p2"][r])
                assert snaps[p + 1]["ply"][i] == 0
            else:
                before, after = ((snaps[q]["bb_p1"][i], snaps[q]["bb_p2"][i]) for q in (p, p + 1))
                assert snaps[p + 1]["ply"][i] == snaps[p]["ply"][i] + 1
            tape[p, i] = move_between(game, before, after)
    assert len({tuple(tape[:6, i]) for i in range(n)}) > n // 2      # drawn: the games differ
    ref = oracle_selfplay(env, monkeypatch, game, team, tape=tape, max_plies=plies, refill=True)
    check_drained(per_game, per_row, ref["finished"], game)
    # a refilled game's trees are ALL reset: on the next ply each starts from an empty tree, as at ply 0, while trees that
    # kept their subtree start with more
    fresh = root_n[0]
    assert (fresh == fresh[0, 0]).all()
    restarted = [(p + 1, i) for (p, i) in ended if p + 1 < plies]
    assert restarted and all((root_n[p][i] == fresh[0, 0]).all() for p, i in restarted)
    assert any((root_n[p] > fresh[0, 0]).any() for p in range(1, plies))


# ---------------------------------------------------------------------------------------- T5

def test_noise_epsilons_are_per_tree(env, monkeypatch):
    """Connect4, a root-parallel team of 2, noise decaying over 4 plies, 6 plies (no game can end): the oracle searches with
    ONE epsilon per ply (game.py:87-91) and records the noise it drew; the driver gets that noise through az_mcts_dev_replay
    and must give every tree its game's epsilon - the trees with index >= n_games catch an array written per game."""
    from test_replay_gpu import _noise_by_edge
    torch, F, L = env["torch"], env["F"], env["L"]
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")
    game, team, n, n_playout, K, plies = "Connect4", (2, False), 5, 24, 4, 6
    noise_steps, eps_init, eps_min = 4, 0.25, 0.05
    tape = opening_tape(game, n, 2)
    # the oracle
    m = O.BatchedMCTS_Connect4(n * team[0])
    S.apply_cfg(m, dict(S.ACTOR_CFG, c_base=500.0, use_symmetry=False))
    m.set_seed(31)
    boards, turns = np.zeros((n, 6, 7), np.int8), np.ones(n, np.int32)
    rec = dict(noise_search=[], noise_prune=[], counts=[], eps=[])
    for p in range(plies):
        eps = eps_min + (eps_init - eps_min) * max(0.0, 1.0 - p / noise_steps)
        m.config.noise_epsilon = eps
        rec["eps"].append(np.float32(eps))
        tb, tt = TH.team_boards(boards, turns, game, team)
        first = {}

        def hook(i, first=first, tb=tb, tt=tt):
            if i == 0:
                first["noise"] = _noise_by_edge(S.C4Game, np.array(m.get_all_root_stats(), np.float32), tb, tt)
        S.playout(m, tb, tt, n_playout, K, None, None, S.C4Game, after_backprop=hook)
        rec["noise_search"].append(first["noise"])
        counts = S.counts_of(m, n * team[0])
        rec["counts"].append(counts)
        actions = tape[p] if p < len(tape) else TH.pick(TH.team_sum(counts, game, team), 0.0)
        m.prune_roots(TH.team_actions(actions, game, team))
        for i in range(n):
            turns[i] = S.C4Game.advance(boards[i], int(turns[i]), int(actions[i]))
        tb, tt = TH.team_boards(boards, turns, game, team)
        rec["noise_prune"].append(_noise_by_edge(S.C4Game, np.array(m.get_all_root_stats(), np.float32), tb, tt))
    assert len(set(float(e) for e in rec["eps"])) == noise_steps + 1 and all((r > 0).any() for r in rec["noise_prune"])
    # the trees of a game drew different noise: they are no copies of each other
    assert any((c.reshape(n, 2, 7)[:, 0] != c.reshape(n, 2, 7)[:, 1]).any() for c in rec["counts"])
    # the driver
    sp = env["SP"].NativeSelfPlay(env["H"].HashEvaluator("cuda"), n, n_playout=n_playout, vl_batch=K, c_init=1.4, c_base=500,
                                  alpha=0.3, noise_epsilon=eps_init, use_symmetry=False, temperature=0.0, temp_endgame=0.0,
                                  temp_decay_moves=0, seed=99, refill=False, sampler="tape", noise_steps=noise_steps,
                                  noise_eps_min=eps_min, n_trees=2)
    sp.set_action_tape(tape)
    model = sp.fused._native_model()
    assert model is not None
    noise = torch.zeros((n * 2, 7), dtype=torch.float32, device="cuda")
    counts = torch.zeros((n * 2, 7), dtype=torch.int32, device="cuda")
    s = F._stream()
    sp.fused.replay(None, noise)
    try:
        for p in range(plies):
            if p == len(tape):
                sp.set_action_tape(None)
            noise.copy_(torch.from_numpy(rec["noise_search"][p]))
            F.check(L.az_selfplay_begin_ply(sp._sp, s))
            F.check(L.az_mcts_dev_search(sp.h, model, n_playout, K, 0, s))
            F.check(L.az_mcts_dev_counts(sp.h, counts.data_ptr(), s))
            got = counts.cpu().numpy()
            assert np.array_equal(got[:n], rec["counts"][p][:n]), p
            assert np.array_equal(got[n:], rec["counts"][p][n:]), p        # trees past the number of games
            noise.copy_(torch.from_numpy(rec["noise_prune"][p]))
            F.check(L.az_selfplay_finish_ply(sp._sp, s))
            torch.cuda.synchronize()
    finally:
        sp.fused.replay(None, None)
    assert sp.read_totals()["positions"] == n * plies and sp.positions()["ply"].tolist() == [plies] * n


# ---------------------------------------------------------------------------------------- T6

def play_by_public_calls(env, sp, temperature, temp_decay_moves, seed, plies):
    """`plies` plies on the engine and model of `sp` (whose own driver object stays unused) as a loop over the public entry
    points, in the driver's order.  Per ply: positions and ply counters after it, the engine's counters, the raw counts."""
    torch, F, L = env["torch"], env["F"], env["L"]
    n, A, gid, T, ens = sp.B, sp.search.action_size, sp.game_id, sp.trees, int(sp.ensemble)
    model = sp.fused._native_model()
    assert model is not None
    z = dict(device="cuda")
    start = (0, 0) if gid == 0 else ((1 << 28) | (1 << 35), (1 << 27) | (1 << 36))
    bb1 = torch.full((n,), start[0], dtype=torch.int64, **z)
    bb2 = torch.full((n,), start[1], dtype=torch.int64, **z)
    turn, aux, ply = torch.ones(n, dtype=torch.int32, **z), torch.zeros(n, dtype=torch.int32, **z), torch.zeros(n, dtype=torch.int32, **z)
    r1, r2, rt = torch.zeros(n * T, dtype=torch.int64, **z), torch.zeros(n * T, dtype=torch.int64, **z), torch.zeros(n * T, dtype=torch.int32, **z)
    counts = torch.zeros((n * T, A), dtype=torch.int32, **z)
    actions, tree_actions = torch.zeros(n, dtype=torch.int32, **z), torch.zeros(n * T, dtype=torch.int32, **z)
    done, win_now = torch.zeros(n, dtype=torch.uint8, **z), torch.zeros(n, dtype=torch.int32, **z)
    dead = torch.zeros(n, dtype=torch.bool, **z)
    cfg = sp_config(env, temperature, 0.0, temp_decay_moves)
    s, h = F._stream(), sp.h
    out = []
    for p in range(plies):
        F.check(L.az_match_team_roots(gid, bb1.data_ptr(), bb2.data_ptr(), turn.data_ptr(), T, ens, r1.data_ptr(), r2.data_ptr(),
                                      rt.data_ptr(), n, s))
        F.check(L.az_mcts_dev_set_roots(h, r1.data_ptr(), r2.data_ptr(), rt.data_ptr(), s))
        F.check(L.az_mcts_dev_search(h, model, sp.n_playout, sp.vl_batch, 0, s))
        F.check(L.az_mcts_dev_counts(h, counts.data_ptr(), s))
        F.check(L.az_selfplay_team_sample(gid, counts.data_ptr(), ply.data_ptr(), C.byref(cfg), T, ens, dev_seed(seed), p, None,
                                          actions.data_ptr(), tree_actions.data_ptr(), n, s))
        actions.masked_fill_(dead, -1)                  # a finished game is dead: action -1 to every tree
        tree_actions.masked_fill_(dead.repeat_interleave(T), -1)
        F.check(L.az_mcts_dev_prune_roots(h, tree_actions.data_ptr(), s))
        F.check(L.az_game_dev_step(gid, bb1.data_ptr(), bb2.data_ptr(), turn.data_ptr(), aux.data_ptr(), actions.data_ptr(),
                                   done.data_ptr(), win_now.data_ptr(), n, 0, s))
        mask = done.repeat_interleave(T).contiguous()
        F.check(L.az_mcts_dev_reset_masked(h, mask.data_ptr(), s))
        ply += (~dead).to(torch.int32)
        running = counts.view(n, T, A)[~dead]
        dead |= done.bool()
        out.append(dict(bb_p1=bb1.cpu().numpy().view(np.uint64).copy(), bb_p2=bb2.cpu().numpy().view(np.uint64).copy(),
                        turn=turn.cpu().numpy().copy(), ply=ply.cpu().numpy().copy(), counters=F.counters(h),
                        diverged=bool((running != running[:, :1]).any()), dead=int(dead.sum())))
    return out


def test_team_selfplay_equals_the_public_entry_points(env, monkeypatch):
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")
    n, plies, seed = 8, 30, 7
    kw = dict(n_playout=16, vl_batch=4, c_init=1.4, c_base=500, alpha=0.3, noise_epsilon=0.25, use_symmetry=True, temperature=1.0,
              temp_decay_moves=4, temp_endgame=0.0, seed=seed, refill=False, n_trees=3)
    nat = env["SP"].NativeSelfPlay(hash_net(env, "Connect4"), n, **kw)
    assert nat.trees == 3 and not nat.ensemble and nat.fused._native_model() is not None
    got = []
    for _ in range(plies):
        nat.step(1)
        got.append(dict(nat.positions(), counters=nat.engine_counters()))
    by_hand = env["SP"].NativeSelfPlay(hash_net(env, "Connect4"), n, **kw)
    want = play_by_public_calls(env, by_hand, 1.0, 4, seed, plies)
    for p, (a, b) in enumerate(zip(got, want)):
        for k in ("bb_p1", "bb_p2", "turn", "ply"):
            assert np.array_equal(a[k], b[k]), (p, k)
        assert a["counters"] == b["counters"], p
    # in some running game the trees' count rows differ (noise and symmetry ids are drawn per tree); some games ended on
    # the way (dead slots, reset trees), and the games are not copies of each other
    assert any(w["diverged"] for w in want) and want[-1]["dead"] > 0
    assert nat.read_totals()["games"] == want[-1]["dead"]
    assert len({(int(a), int(b)) for a, b in zip(want[5]["bb_p1"], want[5]["bb_p2"])}) > n // 2


# ---------------------------------------------------------------------------------------- T7

def raw_drain(env, sp, A):
    return env["SP"].drain_native(env["L"], sp, A)


def test_teams_of_one_are_az_selfplay_create(env):
    L, A = env["L"], env["A"]
    n = 19
    model = C.c_void_p()
    assert L.az_nn_model_create_hash_salted(0, SALT, C.byref(model)) == 0
    runs = []
    for with_teams in (False, True):
        e, sp = raw_engine(env, 0, n, 3), C.c_void_p()
        cfg = A.SelfPlayConfig(1.0, 0.0, 6, 1, 1, 4, 0, 0.25, 0.05)
        if with_teams:
            assert L.az_selfplay_create_teams(e, C.byref(cfg), C.byref(A.SelfPlayTeams(1, 0)), C.byref(sp)) == 0, L.az_last_error()
        else:
            assert L.az_selfplay_create(e, C.byref(cfg), C.byref(sp)) == 0, L.az_last_error()
        assert L.az_selfplay_step(sp, model, 16, 4, 0, 40, None) == 0, L.az_last_error()
        tot = (C.c_int64 * 5)()
        assert L.az_selfplay_totals(sp, C.byref(tot)) == 0
        per_game, per_row = raw_drain(env, sp, 7)
        runs.append((list(tot), per_game, per_row, env["F"].counters(e)))
        L.az_selfplay_destroy(sp)
        L.az_mcts_destroy(e)
    L.az_nn_model_destroy(model)
    assert runs[0][0] == runs[1][0] and runs[0][0][1] >= n and runs[0][3] == runs[1][3]
    for a, b in zip(runs[0][1:3], runs[1][1:3]):
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def test_begin_finish_route_with_a_team(env, monkeypatch):
    """az_selfplay_begin_ply / az_selfplay_finish_ply around FusedSearch (no native model object: AZ_FUSED_NATIVE=0) equal
    az_selfplay_step: the caller searches the whole engine, all trees."""
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")
    game, team = "Connect4", (2, True)
    kw = dict(alpha=0.3, noise_epsilon=0.25, use_symmetry=True, temperature=1.0, temp_decay_moves=6, refill=True, sampler="device", seed=3)
    a = native_selfplay(env, game, team, **kw)
    assert a.fused._native_model() is not None
    a.step(30)
    monkeypatch.setenv("AZ_FUSED_NATIVE", "0")
    b = native_selfplay(env, game, team, **kw)
    assert b.fused._native_model() is None
    b.step(30)
    assert a.read_totals() == b.read_totals() and a.read_totals()["games"] > 0 and a.engine_counters() == b.engine_counters()
    pa, pb = a.positions(), b.positions()
    assert all(np.array_equal(pa[k], pb[k]) for k in pa)
    ga, gb = raw_drain(env, a._sp, 7), raw_drain(env, b._sp, 7)
    assert all(x[k].tobytes() == y[k].tobytes() for x, y in zip(ga, gb) for k in x)


def test_streamed_native_with_teams_equals_its_drivers_run_alone(env):
    from test_native_selfplay_gpu import same_games
    net = hash_net(env, "Connect4")
    kw = dict(n_playout=16, vl_batch=4, temp_decay_moves=6, record=True, td_steps=2, n_trees=2)
    plies = 24
    sp = env["SP"].StreamedSelfPlay(net, 700, streams=2, seed=3, driver="native", **kw)     # 350 games, 700 trees per driver
    assert all(isinstance(p, env["SP"].NativeSelfPlay) and p.trees == 2 and p.B == 350 and p.n_envs == 700 for p in sp.parts)
    sp.step(plies)
    sp.synchronize()
    tot = sp.read_totals()
    assert tot["positions"] == plies * 700 and tot["games"] > 0
    assert sp.engine_counters()["sims"] == plies * 1400 * 16
    games = sp.drain()
    assert len(games) == tot["games"] and max(g[2] for g in games) >= 350
    for i, part in enumerate(sp.parts):
        alone = env["SP"].NativeSelfPlay(net, sp.sizes[i], seed=3 * 2 + i, **kw)
        alone.step(plies)
        a, b = alone.positions(), part.positions()
        assert all(np.array_equal(a[k], b[k]) for k in a)
        assert alone.read_totals() == part.read_totals()
        mine = [(w, play, slot - sp.offsets[i]) for (w, play, slot) in games if sp.offsets[i] <= slot < sp.offsets[i] + sp.sizes[i]]
        same_games(alone.drain(), mine)
    sp.close()


def test_argument_checks(env):
    L, A = env["L"], env["A"]
    c9, c12, ot8 = raw_engine(env, 0, 9, 0), raw_engine(env, 0, 12, 1), raw_engine(env, 1, 8, 2)
    cfg, sp = A.SelfPlayConfig(0.0, 0.0, 0, 0, 1, 0, 0, 0.25, 0.1), C.c_void_p()

    def create(e, teams, c=cfg, out=sp):
        t = C.byref(A.SelfPlayTeams(*teams)) if teams is not None else None
        return L.az_selfplay_create_teams(e, C.byref(c) if c is not None else None, t, C.byref(out) if out is not None else None)
    bad = [(None, (1, 0)), (c9, None),                                  # null arguments
           (c9, (0, 0)), (c9, (-2, 0)),                                 # trees < 1
           (c9, (2, 0)), (c12, (5, 0)),                                 # n_envs is no multiple of the trees per game
           (c9, (3, 1)), (c12, (4, 1)), (c12, (1, 1)), (ot8, (2, 1))]   # an ensemble has az_game_num_augment(game) trees
    for e, teams in bad:
        assert create(e, teams) == AZ_ERR_ARG, teams
    assert create(c9, (1, 0), c=None) == AZ_ERR_ARG and create(c9, (1, 0), out=None) == AZ_ERR_ARG
    # 12 trees in teams of 3: four games; every per-game array has four entries
    assert create(c12, (3, 0)) == 0, L.az_last_error()
    guard = [np.full(5, 9, t) for t in (np.uint64, np.uint64, np.int32, np.int32)]
    assert L.az_selfplay_positions(sp, *(g.ctypes.data for g in guard)) == 0
    assert guard[0].tolist() == [0, 0, 0, 0, 9] and guard[2].tolist() == [1, 1, 1, 1, 9] and guard[3].tolist() == [0, 0, 0, 0, 9]
    L.az_selfplay_destroy(sp)
    assert create(ot8, (4, 1)) == 0, L.az_last_error()                   # Othello's ensemble: two games
    assert L.az_selfplay_positions(sp, *(g.ctypes.data for g in guard)) == 0
    assert guard[2].tolist() == [1, 1, 1, 1, 9] and guard[0][2] == 0 and guard[0][0] == (1 << 28) | (1 << 35)
    L.az_selfplay_destroy(sp)
    for e in (c9, c12, ot8):
        L.az_mcts_destroy(e)
    with pytest.raises(AssertionError):                # a tape row has one entry per GAME
        native_selfplay(env, "Connect4", (2, True)).set_action_tape(np.zeros((2, 38), np.int32))
