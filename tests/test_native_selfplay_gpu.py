"""The native self-play driver (az_selfplay_* in include/az_mcts.h, `NativeSelfPlay` in src/selfplay.py).

1. the reference harness's play data (fixtures G10, G11, G12, G14) through the native driver, bit for bit:
   the moves of every game are read off the fixture's successive states and played from an action tape;
2. the same games as the Python driver (`DeviceSelfPlay`) when nothing random separates the two: every ply
   greedy, noise and symmetry on (both draw them from the engine's generator in the same order);
3. the sampler (k_sp_pick through az_selfplay_sample) draws N^(1/T) / sum - chi-square at the level and row
   counts of tests/test_devrng_gpu.py, with a check that the test can reject a wrong exponent;
4. the C ABI alone through ctypes: whole plies without a torch call in between, drained games replayed
   through the oracle's Env;
5. `StreamedSelfPlay(driver="native")` equals its drivers run alone.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import oracle as O
from test_oracle_golden import bits, load

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
P_REJECT = 1e-4                      # tests/test_devrng_gpu.py
ROWS = 200000


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import torch
    from src import MCTS_cpp, fused, hash_eval, selfplay
    return dict(torch=torch, W=MCTS_cpp, F=fused, H=hash_eval, SP=selfplay, L=fused.lib())


# ---------------------------------------------------------------------------------------- 1. fixtures

def actions_from_states(states, game):
    """The moves of one game from its successive `state` arrays (own / opponent planes + the turn sign):
    the one square that became occupied; Othello: no new stone = pass (64)."""
    occ = (states[:, 0] != 0) | (states[:, 1] != 0)
    acts = []
    for t in range(len(states) - 1):
        new = np.argwhere(occ[t + 1] & ~occ[t])
        if game == "Othello":
            assert len(new) <= 1
            acts.append(int(new[0][0]) * 8 + int(new[0][1]) if len(new) else 64)
        else:
            assert len(new) == 1
            acts.append(int(new[0][1]))
    return acts


def tape_from_fixture(g, n_games, game):
    per_game = [actions_from_states(g[f"g{i}_state"], game) for i in range(n_games)]
    tape = np.full((max(len(a) for a in per_game), n_games), -1, np.int32)
    for i, a in enumerate(per_game):
        tape[:len(a), i] = a
    return tape


FIXTURE_CASES = {
    # constructor arguments of tests/test_fused_gpu.py:736-895
    "g10_selfplay_numpy_rng": (16, "Connect4", 8, dict(
        n_playout=48, vl_batch=4, c_init=1.4, c_base=240, alpha=0.0, noise_epsilon=0.25, fpu_reduction=0.2,
        use_symmetry=False, mlh_slope=0.1, mlh_cap=0.2, temperature=1.0, temp_decay_moves=8, temp_endgame=0, seed=3,
        record=True, td_steps=2, refill=False)),
    "g11_selfplay_plain_search": (8, "Connect4", 7, dict(
        n_playout=40, vl_batch=1, c_init=1.25, c_base=500, alpha=0.0, noise_epsilon=0.0, fpu_reduction=0.4,
        use_symmetry=False, mlh_slope=0.0, mlh_cap=0.2, value_decay=0.98, temperature=0.8, temp_decay_moves=0,
        temp_endgame=0, seed=1, record=True, td_steps=0, refill=False)),
    "g12_selfplay_othello": (8, "Othello", 8, dict(
        n_playout=32, vl_batch=4, c_init=1.4, c_base=160, alpha=0.0, noise_epsilon=0.25, fpu_reduction=0.2,
        use_symmetry=False, mlh_slope=0.0, temperature=1.0, temp_decay_moves=10, temp_endgame=0, seed=4, record=True,
        td_steps=2, refill=False, game="Othello", score_utility_factor=0.15, score_scale=8.0)),
    "g14_selfplay_noise_decay": (12, "Connect4", 8, dict(
        n_playout=48, vl_batch=4, c_init=1.4, c_base=240, alpha=0.0, noise_epsilon=0.25, fpu_reduction=0.2,
        use_symmetry=False, mlh_slope=0.1, mlh_cap=0.2, temperature=1.0, temp_decay_moves=8, temp_endgame=0, seed=3,
        record=True, td_steps=2, refill=False, noise_steps=6, noise_eps_min=0.05)),
}


@pytest.mark.parametrize("name", sorted(FIXTURE_CASES))
def test_reference_play_data_through_the_native_driver(env, name):
    """Recording, epsilon decay, both games, K = 1 and K = 4 and the td-step column against the compiled
    reference's output: every column of every game, floats as uint32."""
    n_games, game, n_cols, kw = FIXTURE_CASES[name]
    g = load(name)
    net = env["H"].HashEvaluator("cuda") if game == "Connect4" else env["H"].OthelloHashEvaluator("cuda")
    tape = tape_from_fixture(g, n_games, game)
    sp = env["SP"].NativeSelfPlay(net, n_games, sampler="tape", **kw)
    sp.set_action_tape(tape)
    sp.step(tape.shape[0])
    assert sp.finished()[0] == n_games and sp.finished()[2] == 0
    with pytest.raises(RuntimeError, match="tape"):                    # AZ_ERR_STATE past the tape's end
        sp.step(1)
    games = sorted(sp.drain(), key=lambda t: t[2])
    assert [t[2] for t in games] == list(range(n_games))
    for i, (winner, play, _slot) in enumerate(games):
        assert winner == int(g[f"g{i}_winner"][0]), i
        assert all(len(t) == n_cols for t in play)
        for j, nm in enumerate(("state", "prob", "z", "steps", "aux", "root_wdl", "mask", "fut")[:n_cols]):
            got = np.array([np.asarray(t[j]) for t in play])
            ref = g[f"g{i}_{nm}"]
            assert got.shape == ref.shape and got.dtype == ref.dtype, (i, nm, got.shape, ref.shape, got.dtype, ref.dtype)
            if ref.dtype.kind == "f":
                assert np.array_equal(bits(got), bits(ref)), (i, nm)
            else:
                assert np.array_equal(got, ref), (i, nm)
    if name == "g10_selfplay_numpy_rng":
        # the actor's upload body: same structure as the reference client's (byte for byte where the
        # pickling environment is the generator's)
        import pickle
        mine = env["SP"].pack_upload(games)
        ref_payload = g["upload_payload"].tobytes()
        if (list(g["upload_numpy_version"]) == [int(x) for x in np.__version__.split(".")[:2]]
                and list(g["upload_python_version"]) == list(sys.version_info[:2])):
            assert mine == ref_payload
        a, b = pickle.loads(mine), pickle.loads(ref_payload)
        assert len(a["data"]) == len(b["data"]) == n_games
        for pa, pb in zip(a["data"], b["data"]):
            assert len(pa) == len(pb)
            for ta, tb in zip(pa, pb):
                assert len(ta) == len(tb) and all(type(x) is type(y) and np.array_equal(x, y) for x, y in zip(ta, tb))
    assert sp.drain() == []


# ---------------------------------------------------------------------------------------- 2. against DeviceSelfPlay

def same_games(a, b):
    assert len(a) == len(b)
    for (w0, play0, slot0), (w1, play1, slot1) in zip(a, b):
        assert w0 == w1 and slot0 == slot1 and len(play0) == len(play1)
        for x, y in zip(play0, play1):
            assert len(x) == len(y)
            for u, v in zip(x, y):
                u, v = np.asarray(u), np.asarray(v)
                assert u.dtype == v.dtype and u.shape == v.shape
                assert np.array_equal(bits(u), bits(v)) if u.dtype.kind == "f" else np.array_equal(u, v)


def check_equals_python_driver(env, monkeypatch, game, n_games, plies, python_search=False, **extra):
    torch = env["torch"]
    net = env["H"].HashEvaluator("cuda") if game == "Connect4" else env["H"].OthelloHashEvaluator("cuda")
    kw = dict(n_playout=24, vl_batch=4, seed=5, temperature=0.0, temp_endgame=0.0, record=True, td_steps=2, refill=True,
              game=game, **extra)
    if not python_search:
        # batches this small replay the Python loop from a hipGraph by default (fused.py): ask for the native
        # loop, where a step of the native driver is ONE az_selfplay_step call
        monkeypatch.setenv("AZ_FUSED_GRAPH", "0")
    dev = env["SP"].DeviceSelfPlay(net, n_games, **kw)
    for _ in range(plies):
        dev.step()
    torch.cuda.synchronize()
    if python_search:
        monkeypatch.setenv("AZ_FUSED_NATIVE", "0")                      # begin_ply / FusedSearch.search / finish_ply
    nat = env["SP"].NativeSelfPlay(net, n_games, **kw)
    assert (nat.fused._native_model() is None) == python_search
    nat.step(plies // 2)
    nat.step(plies - plies // 2)
    tot = nat.read_totals()
    assert tot == dev.read_totals() and tot["positions"] == plies * n_games and tot["games"] > n_games // 2
    assert nat.engine_counters() == dev.engine_counters()
    pos = nat.positions()
    assert np.array_equal(pos["bb_p1"].view(np.int64), dev.bb_p1.cpu().numpy())
    assert np.array_equal(pos["bb_p2"].view(np.int64), dev.bb_p2.cpu().numpy())
    assert np.array_equal(pos["turn"], dev.turn.cpu().numpy()) and np.array_equal(pos["ply"], dev.ply.cpu().numpy())
    assert nat.finished()[2] == int(dev.n_dropped.item()) == 0
    same_games(dev.drain(), nat.drain())


def test_same_games_as_the_python_driver_connect4(env, monkeypatch):
    check_equals_python_driver(env, monkeypatch, "Connect4", 256, 60)


def test_same_games_as_the_python_driver_othello(env, monkeypatch):
    check_equals_python_driver(env, monkeypatch, "Othello", 64, 80)


def test_same_games_through_begin_and_finish_ply(env, monkeypatch):
    check_equals_python_driver(env, monkeypatch, "Connect4", 256, 60, python_search=True)


def test_same_games_with_the_table_on(env, monkeypatch):
    check_equals_python_driver(env, monkeypatch, "Connect4", 256, 60, table_log2=14)


# ---------------------------------------------------------------------------------------- 3. the sampler

def sample(env, game, counts, ply, seed, call, temperature=1.0, temp_endgame=0.0, temp_decay_moves=0):
    torch, SP = env["torch"], env["SP"]
    c = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda()
    p = torch.from_numpy(np.ascontiguousarray(ply, np.int32)).cuda()
    out = torch.full((c.shape[0],), -7, dtype=torch.int32, device="cuda")
    cfg = SP.SelfPlayConfig(temperature, temp_endgame, temp_decay_moves, 1, 0, 0, 0, 0.25, 0.1)
    env["F"].check(env["L"].az_selfplay_sample(0 if game == "Connect4" else 1, c.data_ptr(), p.data_ptr(), C.byref(cfg),
                                               seed, call, out.data_ptr(), c.shape[0], env["F"]._stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def expected_p(vec, T):
    v = np.asarray(vec, np.float64)
    w = np.where(v > 0, v ** (1.0 / T), 0.0)
    return w / w.sum()


def chisq_p(actions, p):
    from scipy import stats
    obs = np.bincount(actions, minlength=len(p)).astype(np.float64)
    assert obs[p == 0].sum() == 0, "an action with N = 0 was drawn"
    if (p > 0).sum() == 1:
        return 1.0
    return stats.chisquare(obs[p > 0], p[p > 0] * obs.sum()).pvalue


def othello_vec(pairs):
    v = np.zeros(65, np.int64)
    for a, n in pairs:
        v[a] = n
    return v


VECTORS = {
    "Connect4": [np.array([10, 20, 30, 5, 0, 40, 95]), np.array([0, 0, 0, 200, 0, 0, 0]), np.array([7] * 7),
                 np.array([4, 4, 150, 4, 4, 4, 30])],
    "Othello": [othello_vec([(0, 10), (9, 20), (18, 30), (27, 5), (40, 40), (63, 95)]), othello_vec([(64, 50)]),
                othello_vec([(a, 6) for a in (2, 3, 11, 19, 20, 26, 37, 44, 53, 62)]),
                othello_vec([(5, 4), (12, 4), (21, 150), (33, 4), (47, 30), (64, 8)])],
}


@pytest.mark.parametrize("game", ["Connect4", "Othello"])
def test_sampler_draws_the_reference_distribution(env, game):
    problems = []
    for vi, vec in enumerate(VECTORS[game]):
        counts = np.tile(vec, (ROWS, 1))
        ply = np.zeros(ROWS, np.int32)
        for T in (1.0, 0.5, 2.0):
            acts = sample(env, game, counts, ply, seed=1000 + vi, call=int(T * 10), temperature=T)
            assert acts.min() >= 0 and acts.max() < len(vec)
            p = chisq_p(acts, expected_p(vec, T))
            print("chi-square", game, vi, T, "p = %.3g" % p)
            if p < P_REJECT:
                problems.append("%s vector %d, T = %.1f: p = %.2e" % (game, vi, T, p))
    assert not problems, "\n".join(problems)
    # power: the T = 0.5 sample is not the T = 1 distribution
    vec = VECTORS[game][0]
    acts = sample(env, game, np.tile(vec, (ROWS, 1)), np.zeros(ROWS, np.int32), seed=77, call=3, temperature=0.5)
    assert chisq_p(acts, expected_p(vec, 0.5)) >= P_REJECT
    assert chisq_p(acts, expected_p(vec, 1.0)) < P_REJECT


def test_sampler_streams_are_independent_and_reproducible(env):
    from scipy import stats
    vec = VECTORS["Connect4"][2]                                       # seven equally likely actions
    counts, ply = np.tile(vec, (ROWS, 1)), np.zeros(ROWS, np.int32)
    a = sample(env, "Connect4", counts, ply, seed=9, call=4)
    b = sample(env, "Connect4", counts, ply, seed=9, call=5)

    def contingency_p(x, y):
        table = np.zeros((7, 7))
        np.add.at(table, (x, y), 1)
        return stats.chi2_contingency(table)[1]
    assert contingency_p(a[:-1], a[1:]) >= P_REJECT, "draws of neighbouring games depend on each other"
    assert contingency_p(a, b) >= P_REJECT, "draws of consecutive calls depend on each other"
    assert contingency_p(a, a) < P_REJECT                              # the check sees a shared stream
    assert np.array_equal(a, sample(env, "Connect4", counts, ply, seed=9, call=4))
    assert not np.array_equal(a, sample(env, "Connect4", counts, ply, seed=10, call=4))
    assert not np.array_equal(a, b)


def test_sampler_greedy_ties_and_temperature_schedule(env):
    # T = 0: the first maximum, exactly; a root without visits plays action 0
    c4 = np.array([[5, 9, 9, 3, 0, 9, 1], [0] * 7, [0, 0, 0, 0, 0, 0, 3], [2, 2, 2, 2, 2, 2, 2]])
    assert sample(env, "Connect4", c4, np.zeros(4, np.int32), 1, 1, temperature=0.0).tolist() == [1, 0, 6, 0]
    ot = np.stack([othello_vec([(10, 7), (64, 7)]), othello_vec([(64, 3)]), othello_vec([]), othello_vec([(63, 2), (5, 2)]),
                   othello_vec([(20, 5), (64, 9)])])
    assert sample(env, "Othello", ot, np.zeros(5, np.int32), 1, 1, temperature=0.0).tolist() == [10, 64, 0, 5, 64]
    # a root without visits plays 0 at any temperature
    assert sample(env, "Connect4", np.zeros((3, 7)), np.zeros(3, np.int32), 1, 1, temperature=1.0).tolist() == [0, 0, 0]
    # game.py:55-63: `temperature` while ply < temp_decay_moves, `temp_endgame` after; constant when <= 0
    vec = VECTORS["Connect4"][0]
    ply = np.repeat(np.array([0, 7, 8, 20], np.int32), ROWS // 4)
    counts = np.tile(vec, (len(ply), 1))
    acts = sample(env, "Connect4", counts, ply, seed=5, call=2, temperature=1.0, temp_endgame=0.0, temp_decay_moves=8)
    assert (acts[ply >= 8] == 6).all()
    assert chisq_p(acts[ply < 8], expected_p(vec, 1.0)) >= P_REJECT
    acts = sample(env, "Connect4", counts, ply, seed=5, call=2, temperature=1.0, temp_endgame=0.5, temp_decay_moves=8)
    assert chisq_p(acts[ply >= 8], expected_p(vec, 0.5)) >= P_REJECT
    assert chisq_p(acts[ply >= 8], expected_p(vec, 1.0)) < P_REJECT
    acts = sample(env, "Connect4", counts, ply, seed=5, call=2, temperature=1.0, temp_endgame=0.0, temp_decay_moves=0)
    assert chisq_p(acts, expected_p(vec, 1.0)) >= P_REJECT


# ---------------------------------------------------------------------------------------- 4. the C ABI alone

class RawConfig(C.Structure):
    _fields_ = [("temperature", C.c_float), ("temp_endgame", C.c_float), ("temp_decay_moves", C.c_int32),
                ("refill", C.c_int32), ("record", C.c_int32), ("noise_steps", C.c_int32),
                ("max_finished_games", C.c_int64), ("noise_eps_init", C.c_double), ("noise_eps_min", C.c_double)]


class RawGames(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("slot", "length", "winner", "finish_ply", "row_start", "bb_p1", "bb_p2",
                                          "turn", "prob", "wdl", "mask")]


def raw_drain(L, sp, A):
    n, rows, dropped = C.c_int64(), C.c_int64(), C.c_int64()
    assert L.az_selfplay_finished(sp, C.byref(n), C.byref(rows), C.byref(dropped)) == 0
    n, rows = n.value, rows.value
    a = dict(slot=np.zeros(n, np.int32), length=np.zeros(n, np.int32), winner=np.zeros(n, np.int32),
             finish_ply=np.zeros(n, np.int64), row_start=np.zeros(n, np.int64), bb_p1=np.zeros(rows, np.uint64),
             bb_p2=np.zeros(rows, np.uint64), turn=np.zeros(rows, np.int8), prob=np.zeros((rows, A), np.float32),
             wdl=np.zeros((rows, 3), np.float32), mask=np.zeros((rows, A), np.uint8))
    out = RawGames(**{k: v.ctypes.data for k, v in a.items()})
    assert L.az_selfplay_drain(sp, C.byref(out), C.c_int64(n), C.c_int64(rows)) == 0, L.az_last_error()
    return a, dropped.value


def check_legal_games(a, game):
    """Every drained game replayed through the oracle's Env: every move legal, winner and final position agree."""
    n = len(a["slot"])
    order = list(zip(a["finish_ply"].tolist(), a["slot"].tolist()))
    assert order == sorted(order)
    at = 0
    for g in range(n):
        T, r0 = int(a["length"][g]), int(a["row_start"][g])
        assert r0 == at and T > 0
        at += T + 1
        e = O.Connect4Env() if game == "Connect4" else O.OthelloEnv()
        for t in range(T + 1):
            assert e.bitboards == (int(a["bb_p1"][r0 + t]), int(a["bb_p2"][r0 + t])) and e.turn == int(a["turn"][r0 + t]), (g, t)
            if t == T:
                break
            assert not e.done()
            assert a["mask"][r0 + t].astype(bool).tolist() == list(e.valid_mask()), (g, t)
            assert abs(float(a["prob"][r0 + t].sum()) - 1.0) < 1e-6 and (a["prob"][r0 + t][a["mask"][r0 + t] == 0] == 0).all()
            occ0 = int(a["bb_p1"][r0 + t]) | int(a["bb_p2"][r0 + t])
            new = (int(a["bb_p1"][r0 + t + 1]) | int(a["bb_p2"][r0 + t + 1])) & ~occ0
            if game == "Connect4":
                assert bin(new).count("1") == 1
                move = (new.bit_length() - 1) // 7
            else:
                assert bin(new).count("1") <= 1
                move = new.bit_length() - 1 if new else 64
            assert a["mask"][r0 + t][move] == 1, (g, t, move)
            e.step(move)
        assert e.done() and e.winPlayer() == int(a["winner"][g]), g
    assert at == len(a["turn"])


def test_c_abi_alone_via_ctypes(env):
    """Engine, hash model and driver through ctypes only: 3 x 30 plies with no torch call in between."""
    L = C.CDLL(os.path.join(PKG, "lib", "libaz_mcts.so"))
    L.az_last_error.restype = C.c_char_p
    vp = C.c_void_p
    L.az_selfplay_step.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.az_selfplay_create.argtypes = [vp, C.POINTER(RawConfig), C.POINTER(vp)]
    L.az_selfplay_destroy.argtypes = [vp]
    L.az_selfplay_destroy.restype = None
    L.az_selfplay_drain.argtypes = [vp, C.POINTER(RawGames), C.c_int64, C.c_int64]
    L.az_selfplay_finished.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.az_selfplay_totals.argtypes = [vp, C.POINTER(C.c_int64 * 5)]
    L.az_selfplay_set_action_tape.argtypes = [vp, vp, C.c_int64]
    L.az_mcts_counters.argtypes = [vp, C.POINTER(C.c_int64 * 8)]
    L.az_mcts_destroy.argtypes = [vp]
    L.az_mcts_destroy.restype = None
    L.az_nn_model_create_hash.argtypes = [C.c_int, C.POINTER(vp)]
    L.az_nn_model_destroy.argtypes = [vp]
    for game_id, game, n, n_playout, A in ((0, "Connect4", 96, 16, 7), (1, "Othello", 24, 8, 65)):
        m, model, sp = vp(), vp(), vp()
        assert L.az_mcts_create(game_id, n, -1, C.byref(m)) == 0, L.az_last_error()
        assert L.az_mcts_set_seed(m, 11) == 0
        assert L.az_nn_model_create_hash(game_id, C.byref(model)) == 0
        cfg = RawConfig(1.0, 0.0, 8, 1, 1, 4, 0, 0.25, 0.05)
        assert L.az_selfplay_create(m, C.byref(cfg), C.byref(sp)) == 0, L.az_last_error()
        for _ in range(3):
            assert L.az_selfplay_step(sp, model, n_playout, 4, 0, 30, None) == 0, L.az_last_error()
        tot = (C.c_int64 * 5)()
        assert L.az_selfplay_totals(sp, C.byref(tot)) == 0
        cnt = (C.c_int64 * 8)()
        assert L.az_mcts_counters(m, C.byref(cnt)) == 0, L.az_last_error()
        assert tot[0] == 90 * n and cnt[0] == 90 * n * n_playout
        assert tot[1] == tot[2] + tot[3] + tot[4]
        a, dropped = raw_drain(L, sp, A)
        assert dropped == 0 and len(a["slot"]) == tot[1] and tot[1] >= (n if game == "Connect4" else 1)
        check_legal_games(a, game)
        assert raw_drain(L, sp, A)[0]["slot"].size == 0                  # draining empties the store
        L.az_selfplay_destroy(sp)

        # a small store: the overflow is dropped and counted, what is kept is well formed
        small = RawConfig(1.0, 0.0, 8, 1, 1, 0, 5, 0.25, 0.1)
        assert L.az_selfplay_create(m, C.byref(small), C.byref(sp)) == 0, L.az_last_error()
        plies = 60 if game == "Connect4" else 126
        assert L.az_selfplay_step(sp, model, n_playout, 4, 0, plies, None) == 0, L.az_last_error()
        assert L.az_selfplay_totals(sp, C.byref(tot)) == 0
        a, dropped = raw_drain(L, sp, A)
        assert len(a["slot"]) == 5 and dropped == tot[1] - 5 > 0
        check_legal_games(a, game)
        assert L.az_selfplay_step(sp, model, n_playout, 4, 0, plies, None) == 0, L.az_last_error()
        a, dropped2 = raw_drain(L, sp, A)
        assert L.az_selfplay_totals(sp, C.byref(tot)) == 0
        assert len(a["slot"]) == 5 and dropped2 == tot[1] - 10
        check_legal_games(a, game)
        L.az_selfplay_destroy(sp)

        # running past an action tape is AZ_ERR_STATE (4) and enqueues nothing
        torch = env["torch"]
        tape = torch.zeros((2, n), dtype=torch.int32, device="cuda")
        tape[:, :] = 3 if game == "Connect4" else -1
        if game == "Othello":
            tape[0, :] = 19                                              # d3, legal for the first player
        torch.cuda.synchronize()
        assert L.az_selfplay_create(m, C.byref(RawConfig(1.0, 0.0, 8, 0, 0, 0, 0, 0.25, 0.1)), C.byref(sp)) == 0
        assert L.az_selfplay_set_action_tape(sp, tape.data_ptr(), 2) == 0
        assert L.az_selfplay_step(sp, model, n_playout, 4, 0, 2, None) == 0, L.az_last_error()
        assert L.az_selfplay_step(sp, model, n_playout, 4, 0, 1, None) == 4 and b"tape" in L.az_last_error()
        assert L.az_selfplay_totals(sp, C.byref(tot)) == 0 and tot[0] == 2 * n
        L.az_selfplay_destroy(sp)
        L.az_nn_model_destroy(model)
        L.az_mcts_destroy(m)


# ---------------------------------------------------------------------------------------- 5. streams

def test_streamed_native_equals_its_drivers_run_alone(env):
    net = env["H"].HashEvaluator("cuda")
    kw = dict(n_playout=24, vl_batch=4, temp_decay_moves=6, record=True, td_steps=2)
    plies = 30
    sp = env["SP"].StreamedSelfPlay(net, 1300, streams=2, seed=3, driver="native", **kw)     # 650 per driver: the native loop
    assert all(isinstance(p, env["SP"].NativeSelfPlay) for p in sp.parts)
    sp.step(plies)
    sp.synchronize()
    tot = sp.read_totals()
    assert tot["positions"] == plies * 1300 and tot["games"] == tot["p1_wins"] + tot["p2_wins"] + tot["draws"] > 0
    assert sp.engine_counters()["sims"] == plies * 1300 * 24
    games = sp.drain()
    assert len(games) == tot["games"] and max(g[2] for g in games) >= 650
    for i, part in enumerate(sp.parts):
        assert part.fused._native_model() is not None
        alone = env["SP"].NativeSelfPlay(net, sp.sizes[i], seed=3 * 2 + i, **kw)
        alone.step(plies)
        a, b = alone.positions(), part.positions()
        assert all(np.array_equal(a[k], b[k]) for k in a)
        assert alone.read_totals() == part.read_totals()
        mine = [(w, play, slot - sp.offsets[i]) for (w, play, slot) in games if sp.offsets[i] <= slot < sp.offsets[i] + sp.sizes[i]]
        same_games(alone.drain(), mine)
    sp.close()
