"""The native evaluation-match driver (az_match_* in include/az_mcts.h, k_match_ply in csrc/match_kernels.hip,
src/match.py) on the GPU:

G1  against the CPU oracle bit for bit: tests/match_harness.py (the reference's `_batched_eval_games`, pinned to the
    compiled reference by fixture G17 in tests/test_match_cpu.py) on the oracle backend plays the same openings with
    the numpy salted hash evaluators; moves, winners and lengths must be equal.  37 Connect4 games (four full
    wavefronts of lane groups and a partial one), K = 4 and K = 1; 5 Othello games with a forced pass;
G2  against the public entry points with everything random on: az_match_step equals a loop of az_mcts_dev_* calls,
    az_match_sample and az_game_dev_step written here;
G3  the begin / finish halves around FusedSearch, and the action tape;
G4  argument checks, and that a finished match stays as it is.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import match_harness as MH
import scenarios as S
from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
G = os.path.join(ROOT, "tests", "golden")
SALT = 0x5A17C0DE1234ABCD
AZ_ERR_ARG, AZ_ERR_STATE = 1, 4


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import torch
    from src import MCTS_cpp, az_net, fused, hash_eval, match
    return dict(torch=torch, W=MCTS_cpp, F=fused, H=hash_eval, M=match, N=az_net, L=fused.lib())


class _OracleC4(O.BatchedMCTS_Connect4):
    """TEST ONLY: the oracle as the wrapper's native backend."""


class _OracleOthello(O.BatchedMCTS_Othello):
    """TEST ONLY: the oracle as the wrapper's native backend."""


# ---------------------------------------------------------------------------------------- openings

# 40 plies towards the full board whose cell (r, c) holds +1 iff ((r + 1) // 2 + c) is even - no four in any
# direction, 21 stones each; columns 5 and 6 keep one free cell and either way of filling them is a draw
NEARLY_FULL = [1, 0, 0, 1, 0, 0, 3, 0, 0, 1, 1, 2, 1, 1, 2, 3, 2, 2, 5, 2, 2, 3, 3, 4, 3, 3, 4, 5, 4, 5, 5, 4, 5, 6, 6, 4, 6, 6, 4, 6]
WIN_IN_ONE = [3, 0, 3, 0, 3, 1]            # +1 to move with three in column 3


def connect4_openings(n=37):
    """n distinct even-length openings (player +1 to move in all of them): the empty board, WIN_IN_ONE, NEARLY_FULL,
    then random legal sequences of 2, 4 and 6 plies that end nowhere."""
    rng = np.random.default_rng(37)
    out, seen = [[], WIN_IN_ONE, NEARLY_FULL], set()
    for seq in out:
        b = np.zeros((6, 7), np.int8)
        for k, a in enumerate(seq):
            S.np_drop(b, a, 1 if k % 2 == 0 else -1)
        assert not S.np_done(b)
        seen.add(b.tobytes())
    while len(out) < n:
        plies = (2, 4, 6)[len(out) % 3]
        b, seq = np.zeros((6, 7), np.int8), []
        for k in range(plies):
            a = int(rng.choice(S.np_valid(b)))
            S.np_drop(b, a, 1 if k % 2 == 0 else -1)
            seq.append(a)
        if S.np_done(b) or b.tobytes() in seen:
            continue
        seen.add(b.tobytes())
        out.append(seq)
    assert {len(s) for s in out} >= {0, 2, 4, 6}
    return out


def othello_positions(n=5):
    """n distinct Othello positions with player +1 to move: one of the stored endgame positions where +1 must pass
    (tests/golden/ot_endgames_passes.npz, the inputs of scenario ot_endgames_passes), then openings of 0, 2, 4, ...
    random plies."""
    g = np.load(os.path.join(G, "ot_endgames_passes.npz"))
    forced = [i for i in range(len(g["in_turns"])) if g["in_turns"][i] == 1 and not S.ot_moves(g["in_boards"][i], 1)
              and not S.ot_over(g["in_boards"][i])]
    boards = [g["in_boards"][forced[-1]].copy()]
    rng = np.random.default_rng(5)
    for i in range(n - 1):
        b, t = S.ot_start(), 1
        for _ in range(2 * i):
            S.ot_play(b, t, int(rng.choice(S.ot_moves(b, t))))
            t = -t
        assert t == 1 and S.ot_moves(b, 1)
        boards.append(b)
    return np.array(boards, np.int8), np.ones(n, np.int32)


C_INIT = (1.25, 1.6)                       # the two engines differ
DET = dict(c_base=500, alpha=0.3, eval_noise_eps=0.0, use_symmetry=False)


_ORACLE = {}


def oracle_match(env, monkeypatch, game, K):
    """The reference loop on the oracle backend, once per case for the whole module."""
    key = (game, K)
    if key in _ORACLE:
        return _ORACLE[key]
    with monkeypatch.context() as mp:
        mp.setitem(env["W"]._BACKENDS, "Connect4", _OracleC4)
        mp.setitem(env["W"]._BACKENDS, "Othello", _OracleOthello)
        if game == "Connect4":
            from src.env_cpp.connect4 import Env
            n, n_playout, kw = 37, 24, dict(openings=connect4_openings())
            nets = (env["H"].NumpyHashEvaluator(0), env["H"].NumpyHashEvaluator(SALT))
        else:
            from src.env_cpp.othello import Env
            n, n_playout, kw = 5, 20, dict(positions=othello_positions())
            nets = (MH.OthelloNumpyHashEvaluator(0), MH.OthelloNumpyHashEvaluator(SALT))
        ws = [env["W"].BatchedMCTS(n, c_init=c, c_base=500, alpha=0.3, n_playout=n_playout, game_name=game, noise_epsilon=0.0,
                                   use_symmetry=False) for c in C_INIT]
        ref = MH.batched_eval_games(ws[0], ws[1], nets[0], nets[1], Env, n, vl_batch=K, eval_temp=0.0, **kw)
        ref["positions"] = MH.env_bitboards(MH.start_envs(Env, n, **kw))
    # the games are not trivial (asserted on the ORACLE's results)
    if game == "Connect4":
        assert (ref["winner"] == 1).any() and (ref["winner"] == -1).any() and (ref["winner"] == 0).any()
        assert ref["length"][1] == 1 and ref["winner"][1] == 1            # WIN_IN_ONE dies on the first ply
        assert ref["length"][2] == 2 and ref["winner"][2] == 0            # NEARLY_FULL ends drawn
        assert ref["length"].max() > 8
    else:
        assert (ref["moves"] == S.OT_PASS).any() and ref["moves"][0, 0] == S.OT_PASS
    # the openings are distinct, so the games are; most of their continuations differ too
    assert len({tuple(ref["moves"][:, i]) for i in range(n)}) > n // 2
    _ORACLE[key] = ref
    return ref


def hash_nets(env, game, swap=False):
    make = env["H"].HashEvaluator if game == "Connect4" else env["H"].OthelloHashEvaluator
    salts = (SALT, 0) if swap else (0, SALT)
    return tuple(make("cuda", salt=s) for s in salts)


def check_against(mt, ref):
    res = mt.results()
    assert res["running"] == 0 and res["p1_wins"] + res["p2_wins"] + res["draws"] == mt.B
    assert np.array_equal(res["winner"], ref["winner"])
    assert np.array_equal(res["length"], ref["length"])
    assert np.array_equal(mt.moves(), MH.moves_table(ref["moves"], mt.MAX_PLIES))
    assert (res["p1_wins"], res["p2_wins"], res["draws"]) == tuple(int((ref["winner"] == v).sum()) for v in (1, -1, 0))


# ---------------------------------------------------------------------------------------- G1

@pytest.mark.parametrize("game,K", [("Connect4", 4), ("Connect4", 1), ("Othello", 4)])
def test_native_match_equals_the_oracle(env, monkeypatch, game, K):
    ref = oracle_match(env, monkeypatch, game, K)
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")          # batches this small: ask for the native loop (one az_match_step)
    n = len(ref["winner"])
    mt = env["M"].EvaluationMatch(*hash_nets(env, game), n, n_playout=24 if game == "Connect4" else 20, vl_batch=K,
                                  c_init=C_INIT, eval_temp=0.0, game=game, positions=ref["positions"], record_moves=True, **DET)
    assert mt.native_models() is not None
    winners = mt.play()
    assert winners.dtype == np.int32 and np.array_equal(winners, ref["winner"])
    check_against(mt, ref)


class RawSearchConfig(C.Structure):
    """az_search_config (include/az_mcts.h)."""
    _fields_ = [(n, C.c_float) for n in ("c_init", "c_base", "dirichlet_alpha", "noise_epsilon", "fpu_reduction", "mlh_slope",
                                         "mlh_cap", "score_utility_factor", "score_scale", "value_decay")] + \
               [("use_symmetry", C.c_uint8), ("vl_count", C.c_int32)]


class RawMatchConfig(C.Structure):
    _fields_ = [("temperature", C.c_float), ("record_moves", C.c_int32)]


def raw_lib():
    L = C.CDLL(os.path.join(PKG, "lib", "libaz_mcts.so"))
    vp, i32, i64 = C.c_void_p, C.c_int, C.c_int64
    L.az_last_error.restype = C.c_char_p
    L.az_mcts_create.argtypes = [i32, i32, i32, C.POINTER(vp)]
    L.az_mcts_destroy.argtypes = [vp]; L.az_mcts_destroy.restype = None
    L.az_mcts_config.argtypes = [vp]; L.az_mcts_config.restype = C.POINTER(RawSearchConfig)
    L.az_mcts_set_seed.argtypes = [vp, i32]
    L.az_mcts_counters.argtypes = [vp, C.POINTER(i64 * 8)]
    L.az_nn_model_create_hash_salted.argtypes = [i32, C.c_uint64, C.POINTER(vp)]
    L.az_nn_model_destroy.argtypes = [vp]
    L.az_match_create.argtypes = [vp, vp, C.POINTER(RawMatchConfig), C.POINTER(vp)]
    L.az_match_destroy.argtypes = [vp]; L.az_match_destroy.restype = None
    L.az_match_set_positions.argtypes = [vp, vp, vp, vp]
    L.az_match_step.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp]
    L.az_match_remaining.argtypes = [vp, C.POINTER(i64)]
    L.az_match_results.argtypes = [vp, vp, vp, C.POINTER(i64 * 4)]
    L.az_match_moves.argtypes = [vp, vp]
    L.az_match_max_plies.argtypes = [vp]
    return L


def raw_engine(L, game_id, n, c_init, seed):
    m = C.c_void_p()
    assert L.az_mcts_create(game_id, n, -1, C.byref(m)) == 0, L.az_last_error()
    cfg = L.az_mcts_config(m).contents
    cfg.c_init, cfg.c_base, cfg.dirichlet_alpha, cfg.noise_epsilon, cfg.use_symmetry = c_init, 500.0, 0.3, 0.0, 0
    assert L.az_mcts_set_seed(m, seed) == 0
    return m


def test_native_match_equals_the_oracle_c_abi_alone(env, monkeypatch):
    """The same Connect4 match (K = 4) through ctypes only: engines, salted hash models and the match object, no
    torch call and no Python class in between."""
    ref = oracle_match(env, monkeypatch, "Connect4", 4)
    L = raw_lib()
    n = 37
    e1, e2 = raw_engine(L, 0, n, C_INIT[0], 0), raw_engine(L, 0, n, C_INIT[1], 1)
    m1, m2, mt = C.c_void_p(), C.c_void_p(), C.c_void_p()
    assert L.az_nn_model_create_hash_salted(0, 0, C.byref(m1)) == 0 and L.az_nn_model_create_hash_salted(0, SALT, C.byref(m2)) == 0
    assert L.az_match_create(e1, e2, C.byref(RawMatchConfig(0.0, 1)), C.byref(mt)) == 0, L.az_last_error()
    assert L.az_match_max_plies(mt) == 42
    bb1, bb2, turns = ref["positions"]
    assert L.az_match_set_positions(mt, bb1.ctypes.data, bb2.ctypes.data, turns.ctypes.data) == 0, L.az_last_error()
    left = C.c_int64(n)
    for _ in range(42 // 6):
        assert L.az_match_step(mt, m1, m2, 24, 4, 0, 6, None) == 0, L.az_last_error()
        assert L.az_match_remaining(mt, C.byref(left)) == 0
        if left.value == 0:
            break
    assert left.value == 0
    winner, length, totals = np.zeros(n, np.int32), np.zeros(n, np.int32), (C.c_int64 * 4)()
    moves = np.zeros((42, n), np.int32)
    assert L.az_match_results(mt, winner.ctypes.data, length.ctypes.data, C.byref(totals)) == 0
    assert L.az_match_moves(mt, moves.ctypes.data) == 0
    assert np.array_equal(winner, ref["winner"]) and np.array_equal(length, ref["length"])
    assert np.array_equal(moves, MH.moves_table(ref["moves"], 42))
    assert list(totals) == [int((ref["winner"] == v).sum()) for v in (1, -1, 0)] + [0]
    L.az_match_destroy(mt)
    L.az_nn_model_destroy(m1); L.az_nn_model_destroy(m2)
    L.az_mcts_destroy(e1); L.az_mcts_destroy(e2)


# ---------------------------------------------------------------------------------------- G2

def dev_seed(seed):
    """What az_mcts_set_seed(seed >= 0) leaves as the device generator's seed (include/az_mcts.h, az_match_sample)."""
    return ((int(seed) & 0xFFFFFFFF) * 0x9E3779B97F4A7C15 + 1) & ((1 << 64) - 1)


def random_c4_net(env, seed):
    torch = env["torch"]
    torch.manual_seed(seed)
    net = env["N"].Connect4Net(device="cuda").eval()
    with torch.no_grad():                               # a fresh network's heads are zero: uniform outputs
        for lin in (net.policy_head.out, net.dual_head.value_out, net.dual_head.aux_out):
            lin.weight.normal_(0.0, 0.3)
    return net


def play_by_public_calls(env, mt, temp, seed):
    """One match on the engines and models of `mt` (whose own match object stays unused) as a loop over the public
    entry points - the calls az_match_step documents, in its order.  Returns moves, winners, lengths and both
    engines' counters after every ply."""
    torch, F, L = env["torch"], env["F"], env["L"]
    n, A, gid = mt.B, mt.A, mt.sides[0].game_id
    models = mt.native_models()
    assert models is not None
    z = dict(device="cuda")
    start = (0, 0) if gid == 0 else ((1 << 28) | (1 << 35), (1 << 27) | (1 << 36))
    bb1 = torch.full((n,), start[0], dtype=torch.int64, **z)
    bb2 = torch.full((n,), start[1], dtype=torch.int64, **z)
    turn = torch.ones(n, dtype=torch.int32, **z)
    aux = torch.zeros(n, dtype=torch.int32, **z)
    counts = torch.zeros((n, A), dtype=torch.int32, **z)
    actions = torch.zeros(n, dtype=torch.int32, **z)
    done = torch.zeros(n, dtype=torch.uint8, **z)
    win_now = torch.zeros(n, dtype=torch.int32, **z)
    dead = torch.zeros(n, dtype=torch.bool, **z)
    winner = torch.zeros(n, dtype=torch.int32, **z)
    length = torch.zeros(n, dtype=torch.int32, **z)
    moves, counters = [], []
    s = F._stream()
    hs = [side.h for side in mt.sides]
    for ply in range(mt.MAX_PLIES):
        if bool(dead.all()):
            break
        m = 0 if ply % 2 == 0 else 1
        F.check(L.az_mcts_dev_set_roots(hs[m], bb1.data_ptr(), bb2.data_ptr(), turn.data_ptr(), s))
        F.check(L.az_mcts_dev_search(hs[m], models[m], mt.n_playout, mt.vl_batch, 0, s))
        F.check(L.az_mcts_dev_counts(hs[m], counts.data_ptr(), s))
        F.check(L.az_match_sample(gid, counts.data_ptr(), temp, dev_seed(seed), ply, actions.data_ptr(), n, s))
        actions.masked_fill_(dead, -1)                  # a finished game is dead: action -1 to both engines
        for h in hs:
            F.check(L.az_mcts_dev_prune_roots(h, actions.data_ptr(), s))
        F.check(L.az_game_dev_step(gid, bb1.data_ptr(), bb2.data_ptr(), turn.data_ptr(), aux.data_ptr(), actions.data_ptr(),
                                   done.data_ptr(), win_now.data_ptr(), n, 0, s))
        for h in hs:
            F.check(L.az_mcts_dev_reset_masked(h, done.data_ptr(), s))
        length += (~dead).to(torch.int32)
        winner = torch.where(done.bool(), win_now, winner)
        dead |= done.bool()
        moves.append(actions.cpu().numpy().copy())
        counters.append(tuple(F.counters(h) for h in hs))
    return np.array(moves, np.int32), winner.cpu().numpy(), length.cpu().numpy(), counters


def check_equals_public_calls(env, monkeypatch, game, nets, n, n_playout, swapped_nets):
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")          # the native loop below 512 trees too
    kw = dict(n_playout=n_playout, vl_batch=4, c_init=1.4, c_base=500, alpha=0.3, eval_noise_eps=0.05, eval_temp=0.2,
              use_symmetry=True, seed=7, game=game, record_moves=True)
    nat = env["M"].EvaluationMatch(nets[0], nets[1], n, **kw)
    assert nat.native_models() is not None
    nat_counters = []
    while nat.remaining() > 0:
        nat.step(1)
        nat_counters.append(nat.engine_counters())
    by_hand = env["M"].EvaluationMatch(nets[0], nets[1], n, **kw)
    moves, winner, length, counters = play_by_public_calls(env, by_hand, 0.2, 7)
    res = nat.results()
    assert np.array_equal(nat.moves(), MH.moves_table(moves, nat.MAX_PLIES))
    assert np.array_equal(res["winner"], winner) and np.array_equal(res["length"], length)
    assert res["running"] == 0 and len({tuple(moves[:, i]) for i in range(n)}) > n // 2
    # Counters: ALL eight of az_mcts_counters, of BOTH engines, after EVERY ply - not only up to the first ply on
    # which a game ends.  A dead slot costs the native driver what it costs the loop above: its final position goes
    # into the mover's engine with the rest of the batch and is searched as the terminal root it is, its trees are
    # reset by the re-rooting with action -1; the loop issues the very same calls, so the figures stay equal.
    assert len(nat_counters) == len(counters)
    first_end = int(length.min())
    for p, (a, b) in enumerate(zip(nat_counters, counters)):
        assert a == b, (p, first_end)
    # the players matter: the same match with the models swapped is another match
    swapped = env["M"].EvaluationMatch(swapped_nets[0], swapped_nets[1], n, **kw)
    swapped.play()
    assert not np.array_equal(swapped.moves(), nat.moves())


def test_match_step_equals_the_public_entry_points_connect4(env, monkeypatch):
    a, b = random_c4_net(env, 1), random_c4_net(env, 2)
    check_equals_public_calls(env, monkeypatch, "Connect4", (a, b), 64, 32, (b, a))


def test_match_step_equals_the_public_entry_points_othello(env, monkeypatch):
    check_equals_public_calls(env, monkeypatch, "Othello", hash_nets(env, "Othello"), 6, 16, hash_nets(env, "Othello", swap=True))


# ---------------------------------------------------------------------------------------- G3

def test_halves_around_fused_search(env, monkeypatch):
    """az_match_begin_ply / az_match_finish_ply around FusedSearch with the torch HashEvaluator (no native model
    object: AZ_FUSED_NATIVE=0) play G1's Connect4 games."""
    ref = oracle_match(env, monkeypatch, "Connect4", 4)
    monkeypatch.setenv("AZ_FUSED_NATIVE", "0")
    mt = env["M"].EvaluationMatch(*hash_nets(env, "Connect4"), 37, n_playout=24, vl_batch=4, c_init=C_INIT, eval_temp=0.0,
                                  positions=ref["positions"], record_moves=True, **DET)
    assert mt.native_models() is None
    assert np.array_equal(mt.play(), ref["winner"])
    check_against(mt, ref)


def test_action_tape_replays_g17(env, monkeypatch):
    g = np.load(os.path.join(G, "g17_eval_match.npz"))
    monkeypatch.setenv("AZ_FUSED_GRAPH", "0")
    for name in ("c4_k1", "c4_k4"):
        tape = g[name + "_moves"]
        mt = env["M"].EvaluationMatch(*hash_nets(env, "Connect4"), tape.shape[1], n_playout=8, vl_batch=4, record_moves=True)
        mt.set_action_tape(tape)
        mt.step(tape.shape[0])
        res = mt.results()
        assert res["running"] == 0
        assert np.array_equal(res["winner"], g[name + "_winner"]) and np.array_equal(res["length"], g[name + "_length"])
        assert np.array_equal(mt.moves(), MH.moves_table(tape, 42))
    # running past the tape while games are running is AZ_ERR_STATE
    mt = env["M"].EvaluationMatch(*hash_nets(env, "Connect4"), tape.shape[1], n_playout=8, vl_batch=4)
    mt.set_action_tape(tape[:3])
    mt.step(3)
    with pytest.raises(RuntimeError, match="tape"):
        mt.step(1)
    res = mt.results()
    assert res["running"] == tape.shape[1] and (res["length"] == 3).all() and (res["winner"] == 0).all()
    mt.set_action_tape(None)                           # the pick takes over
    mt.step(1)
    assert (mt.results()["length"] == 4).all()


# ---------------------------------------------------------------------------------------- G4

def test_argument_checks_and_a_finished_match(env, monkeypatch):
    L = raw_lib()
    c4a, c4b, c4small, ot = raw_engine(L, 0, 9, 1.25, 0), raw_engine(L, 0, 9, 1.25, 1), raw_engine(L, 0, 8, 1.25, 2), raw_engine(L, 1, 9, 1.25, 3)
    cfg, mt = RawMatchConfig(0.0, 1), C.c_void_p()
    for bad in ((c4a, ot), (c4a, c4small), (c4a, c4a), (c4a, None)):
        assert L.az_match_create(bad[0], bad[1], C.byref(cfg), C.byref(mt)) == AZ_ERR_ARG
    assert L.az_match_create(c4a, c4b, None, C.byref(mt)) == AZ_ERR_ARG
    assert L.az_match_create(c4a, c4b, C.byref(cfg), C.byref(mt)) == 0, L.az_last_error()
    m1, m2 = C.c_void_p(), C.c_void_p()
    assert L.az_nn_model_create_hash_salted(0, 0, C.byref(m1)) == 0 and L.az_nn_model_create_hash_salted(0, SALT, C.byref(m2)) == 0
    # mixed sides to move
    bb1, bb2, turns = np.zeros(9, np.uint64), np.zeros(9, np.uint64), np.ones(9, np.int32)
    turns[4] = -1
    assert L.az_match_set_positions(mt, bb1.ctypes.data, bb2.ctypes.data, turns.ctypes.data) == AZ_ERR_ARG
    assert b"side to move" in L.az_last_error()
    # null models
    assert L.az_match_step(mt, None, m2, 8, 4, 0, 1, None) == AZ_ERR_ARG
    assert L.az_match_step(mt, m1, None, 8, 4, 0, 1, None) == AZ_ERR_ARG
    # a start position that is already over: finished at ply 0 with its winner and length 0
    # -1 moved last and holds the bottom row's first four cells; +1's four stones make no line
    bb2[3] = np.uint64(sum(1 << (7 * c) for c in range(4)))
    bb1[3] = np.uint64((1 << 1) | (1 << 8) | (1 << 15) | (1 << 28))
    turns[:] = 1
    assert L.az_match_set_positions(mt, bb1.ctypes.data, bb2.ctypes.data, turns.ctypes.data) == 0, L.az_last_error()
    winner, length, totals = np.zeros(9, np.int32), np.zeros(9, np.int32), (C.c_int64 * 4)()
    assert L.az_match_results(mt, winner.ctypes.data, length.ctypes.data, C.byref(totals)) == 0
    assert list(totals) == [0, 1, 0, 8] and winner[3] == -1 and (length == 0).all()
    assert L.az_match_step(mt, m1, m2, 8, 4, 0, 1, None) == 0, L.az_last_error()
    # after the first ply the positions are the match's
    assert L.az_match_set_positions(mt, bb1.ctypes.data, bb2.ctypes.data, turns.ctypes.data) == AZ_ERR_ARG
    assert b"begun" in L.az_last_error()
    left = C.c_int64(9)
    for _ in range(42):
        assert L.az_match_step(mt, m1, m2, 8, 4, 0, 1, None) == 0, L.az_last_error()
        assert L.az_match_remaining(mt, C.byref(left)) == 0
        if left.value == 0:
            break
    assert left.value == 0

    def snapshot():
        w, ln, t, mv = np.zeros(9, np.int32), np.zeros(9, np.int32), (C.c_int64 * 4)(), np.zeros((42, 9), np.int32)
        assert L.az_match_results(mt, w.ctypes.data, ln.ctypes.data, C.byref(t)) == 0 and L.az_match_moves(mt, mv.ctypes.data) == 0
        cnt = []
        for e in (c4a, c4b):
            c = (C.c_int64 * 8)()
            assert L.az_mcts_counters(e, C.byref(c)) == 0
            cnt.append(list(c))
        return w.tolist(), ln.tolist(), list(t), mv.tolist(), cnt
    before = snapshot()
    assert before[2][3] == 0 and before[1][3] == 0 and sum(before[2][:3]) == 9 and (np.array(before[3])[:, 3] == -1).all()
    assert L.az_match_step(mt, m1, m2, 8, 4, 0, 5, None) == 0, L.az_last_error()      # nothing left to play: a no-op
    assert snapshot() == before
    L.az_match_destroy(mt)
    L.az_nn_model_destroy(m1); L.az_nn_model_destroy(m2)
    for e in (c4a, c4b, c4small, ot):
        L.az_mcts_destroy(e)
