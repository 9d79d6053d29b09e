"""Finished self-play games as replay-buffer rows on the device (k_sp_export: az_selfplay_export and
az_replay_dev_store in include/az_mcts.h, `NativeSelfPlay.export` / `StreamedSelfPlay.export` in src/selfplay.py).

1. the reference harness's games (fixtures G11 + G10, G12) played from an action tape and exported equal what the
   reference's own ReplayBuffer.store left (fixture G15), bit for bit; G14 equals the host route of a twin driver;
2. at scale, with refill, noise and symmetry: exports every few plies into a ring that wraps several times equal
   a twin driver's drain() + `ReplayTensors.store_games` on the host;
3. az_replay_dev_store on drained arrays uploaded again, calls with more rows than the ring included;
4. no game is lost or exported twice across interleaved step / export calls on one stream;
5. the C ABI alone through ctypes, with its error cases;
6. `StreamedSelfPlay(driver="native").export` equals its drivers exported alone, one after the other.

The reference itself is never imported here: the golden file stands for it.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from test_oracle_golden import load
from test_replay_export_cpu import GOLDEN_CASES, TENSORS, buffer_arrays, differences, golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import torch
    from src import fused, hash_eval, replay, selfplay
    return dict(torch=torch, F=fused, H=hash_eval, SP=selfplay, RP=replay, L=fused.lib())


def hash_net(env, game):
    return env["H"].HashEvaluator("cuda") if game == "Connect4" else env["H"].OthelloHashEvaluator("cuda")


def same_buffers(got, expected):
    """`got`, `expected`: ReplayTensors (any device) or dicts of arrays; every tensor, every slot, every bit."""
    a = got if isinstance(got, dict) else buffer_arrays(got)
    b = expected if isinstance(expected, dict) else buffer_arrays(expected)
    assert differences(a, b) == []
    if not isinstance(got, dict) and not isinstance(expected, dict):
        assert got._ptr == expected._ptr


# ---------------------------------------------------------------------------------------- 1. fixtures

def actions_from_states(states, game):
    """The moves of one game from its successive `state` arrays (own / opponent planes + the turn sign): the one
    square that became occupied; Othello: no new stone = pass (64).  As tests/test_native_selfplay_gpu.py."""
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
    # constructor arguments of tests/test_native_selfplay_gpu.py
    "g10_selfplay_numpy_rng": (16, "Connect4", dict(
        n_playout=48, vl_batch=4, c_init=1.4, c_base=240, alpha=0.0, noise_epsilon=0.25, fpu_reduction=0.2,
        use_symmetry=False, mlh_slope=0.1, mlh_cap=0.2, temperature=1.0, temp_decay_moves=8, temp_endgame=0, seed=3,
        record=True, td_steps=2, refill=False)),
    "g11_selfplay_plain_search": (8, "Connect4", dict(
        n_playout=40, vl_batch=1, c_init=1.25, c_base=500, alpha=0.0, noise_epsilon=0.0, fpu_reduction=0.4,
        use_symmetry=False, mlh_slope=0.0, mlh_cap=0.2, value_decay=0.98, temperature=0.8, temp_decay_moves=0,
        temp_endgame=0, seed=1, record=True, td_steps=0, refill=False)),
    "g12_selfplay_othello": (8, "Othello", dict(
        n_playout=32, vl_batch=4, c_init=1.4, c_base=160, alpha=0.0, noise_epsilon=0.25, fpu_reduction=0.2,
        use_symmetry=False, mlh_slope=0.0, temperature=1.0, temp_decay_moves=10, temp_endgame=0, seed=4, record=True,
        td_steps=2, refill=False, game="Othello", score_utility_factor=0.15, score_scale=8.0)),
    "g14_selfplay_noise_decay": (12, "Connect4", dict(
        n_playout=48, vl_batch=4, c_init=1.4, c_base=240, alpha=0.0, noise_epsilon=0.25, fpu_reduction=0.2,
        use_symmetry=False, mlh_slope=0.1, mlh_cap=0.2, temperature=1.0, temp_decay_moves=8, temp_endgame=0, seed=3,
        record=True, td_steps=2, refill=False, noise_steps=6, noise_eps_min=0.05)),
}


def played_fixture(env, name):
    n_games, game, kw = FIXTURE_CASES[name]
    tape = tape_from_fixture(load(name), n_games, game)
    sp = env["SP"].NativeSelfPlay(hash_net(env, game), n_games, sampler="tape", **kw)
    sp.set_action_tape(tape)
    sp.step(tape.shape[0])
    assert sp.finished()[0] == n_games and sp.finished()[2] == 0
    return sp


def check_emptied(sp):
    n, rows, dropped = sp.finished()
    assert (n, rows, dropped) == (0, 0, 0) and sp.drain() == []


@pytest.mark.parametrize("key", sorted(GOLDEN_CASES))
def test_exported_fixture_games_equal_the_reference_buffer(env, key):
    game, names = GOLDEN_CASES[key]
    expected, ptr, cap = golden(key)
    buf = env["RP"].ReplayTensors(game, cap, "cuda")
    rows = 0
    for name in names:
        sp = played_fixture(env, name)
        n_games = FIXTURE_CASES[name][0]
        at = buf._ptr
        info = sp.export(buf)
        g = load(name)
        lens = [len(g[f"g{i}_state"]) - 1 for i in range(n_games)]
        order = sorted(range(n_games), key=lambda i: (lens[i], i))
        assert info["slot"].tolist() == order and info["length"].tolist() == [lens[i] for i in order]
        assert info["winner"].tolist() == [int(g[f"g{i}_winner"][0]) for i in order]
        assert info["finish_ply"].tolist() == [lens[i] - 1 for i in order]
        rows += sum(lens) + n_games
        assert buf._ptr == at + sum(lens) + n_games
        check_emptied(sp)
    assert buf._ptr == ptr == rows
    same_buffers(buffer_arrays(buf), expected)


def test_exported_noise_decay_games_equal_the_host_route(env):
    name = "g14_selfplay_noise_decay"
    game = FIXTURE_CASES[name][1]
    a, b = played_fixture(env, name), played_fixture(env, name)
    dev = env["RP"].ReplayTensors(game, 101, "cuda")
    host = env["RP"].ReplayTensors(game, 101, "cpu")
    dev._ptr = host._ptr = 77                                           # a buffer in use
    a.export(dev)
    host.store_games(b.drain())
    assert host._ptr == 77 + 258
    same_buffers(dev, host)
    check_emptied(a)


# ---------------------------------------------------------------------------------------- 2. at scale

@pytest.mark.parametrize("game,n_games,plies,every,capacity,at_least", [
    ("Connect4", 4096, 40, 8, 20011, 2000), ("Othello", 256, 140, 10, 4099, 300)])
def test_export_at_scale_equals_drain_and_store_games(env, game, n_games, plies, every, capacity, at_least):
    SP, RP = env["SP"], env["RP"]
    kw = dict(n_playout=16, vl_batch=4, seed=21, temp_decay_moves=10, record=True, td_steps=3, refill=True, game=game)
    net = hash_net(env, game)
    a, b = SP.NativeSelfPlay(net, n_games, **kw), SP.NativeSelfPlay(net, n_games, **kw)
    dev, host = RP.ReplayTensors(game, capacity, "cuda"), RP.ReplayTensors(game, capacity, "cpu")
    exported = 0
    for _ in range(plies // every):
        a.step(every)
        exported += len(a.export(dev)["slot"])
        b.step(every)
        host.store_games(b.drain())
    assert a.finished()[2] == b.finished()[2] == 0
    assert exported == a.read_totals()["games"] == b.read_totals()["games"] >= at_least
    assert dev._ptr >= 3 * capacity, "the ring must wrap several times"
    print("export at scale:", game, exported, "games,", dev._ptr, "rows into", capacity)
    same_buffers(dev, host)


# ---------------------------------------------------------------------------------------- 3. az_replay_dev_store

@pytest.mark.parametrize("game,n_games,plies", [("Connect4", 256, 40), ("Othello", 32, 130)])
def test_dev_store_on_uploaded_games(env, game, n_games, plies):
    torch, SP, RP, L, F = env["torch"], env["SP"], env["RP"], env["L"], env["F"]
    td = 2
    sp = SP.NativeSelfPlay(hash_net(env, game), n_games, n_playout=16, vl_batch=4, seed=9, temp_decay_moves=10, record=True,
                           td_steps=td, game=game)
    sp.step(plies)
    A = sp.search.action_size
    g, r = SP.drain_native(sp.L, sp._sp, A)
    n = len(g["slot"])
    assert n >= 20
    mask = r["mask"].view(np.bool_)
    bb1, bb2 = r["bb_p1"].view(np.int64), r["bb_p2"].view(np.int64)
    perm = np.random.default_rng(4).permutation(n)                       # source rows and destination rows differ

    def rows_of(k):
        i = int(perm[k])
        lo, hi = int(g["row_start"][i]), int(g["row_start"][i]) + int(g["length"][i]) + 1
        return bb1[lo:hi], bb2[lo:hi], r["turn"][lo:hi], r["prob"][lo:hi], r["wdl"][lo:hi], mask[lo:hi]
    games = SP.assemble_games(game, td, g["length"][perm], g["winner"][perm], g["slot"][perm], rows_of)
    up = {k: torch.from_numpy(np.ascontiguousarray(r[k])).cuda() for k in ("turn", "prob", "wdl", "mask")}
    up["bb_p1"], up["bb_p2"] = (torch.from_numpy(x.copy()).cuda() for x in (bb1, bb2))
    length = torch.from_numpy(np.ascontiguousarray(g["length"][perm])).cuda()
    winner = torch.from_numpy(np.ascontiguousarray(g["winner"][perm])).cuda()
    src = torch.from_numpy(np.ascontiguousarray(g["row_start"][perm])).cuda()
    lens = g["length"][perm].astype(np.int64) + 1
    dst = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)).cuda()
    total = int(lens.sum())
    games_dev = SP.SelfPlayGames(slot=None, length=length.data_ptr(), winner=winner.data_ptr(), finish_ply=None, row_start=None,
                                 **{k: up[k].data_ptr() for k in ("bb_p1", "bb_p2", "turn", "prob", "wdl", "mask")})
    for capacity, ptr in ((total + 57, 0), (total + 57, total + 30), (total // 3 + 1, 12345), (101, 7), (19, 0)):
        dev, host = RP.ReplayTensors(game, capacity, "cuda"), RP.ReplayTensors(game, capacity, "cpu")
        dev._ptr = host._ptr = ptr
        F.check(L.az_replay_dev_store(sp.game_id, C.byref(games_dev), src.data_ptr(), dst.data_ptr(), n,
                                      C.byref(RP.replay_tensors_c(dev, game, "cuda")), ptr, td, F._stream()))
        dev._ptr += total
        host.store_games(games)
        same_buffers(dev, host)


# ---------------------------------------------------------------------------------------- 4. conservation

def test_no_game_lost_or_doubled_across_interleaved_steps_and_exports(env):
    SP, RP = env["SP"], env["RP"]
    sp = SP.NativeSelfPlay(hash_net(env, "Connect4"), 512, n_playout=16, vl_batch=4, seed=2, temp_decay_moves=10, record=True,
                           td_steps=1, max_finished_games=96)
    buf = RP.ReplayTensors("Connect4", 5003, "cuda")
    seen, exported, rows = set(), 0, 0
    for chunk in (3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7):
        sp.step(chunk)                                                   # nothing between the two calls
        info = sp.export(buf)
        pairs = list(zip(info["slot"].tolist(), info["finish_ply"].tolist()))
        assert len(set(pairs)) == len(pairs) and not (seen & set(pairs))
        seen |= set(pairs)
        exported += len(pairs)
        rows += int(info["length"].sum()) + len(pairs)
    sp.step(2)
    in_store, _rows, dropped = sp.finished()
    assert dropped > 0, "the small store was meant to overflow"
    assert exported + in_store + dropped == sp.read_totals()["games"]
    assert buf._ptr == rows and exported > 300


# ---------------------------------------------------------------------------------------- 5. the C ABI alone

class RawConfig(C.Structure):
    _fields_ = [("temperature", C.c_float), ("temp_endgame", C.c_float), ("temp_decay_moves", C.c_int32),
                ("refill", C.c_int32), ("record", C.c_int32), ("noise_steps", C.c_int32),
                ("max_finished_games", C.c_int64), ("noise_eps_init", C.c_double), ("noise_eps_min", C.c_double)]


class RawGames(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("slot", "length", "winner", "finish_ply", "row_start", "bb_p1", "bb_p2",
                                          "turn", "prob", "wdl", "mask")]


class RawTensors(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TENSORS] + [("capacity", C.c_int64)]


class RawInfo(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("slot", "length", "winner", "finish_ply")]


def raw_finished(L, sp):
    n, rows, dropped = C.c_int64(), C.c_int64(), C.c_int64()
    assert L.az_selfplay_finished(sp, C.byref(n), C.byref(rows), C.byref(dropped)) == 0
    return n.value, rows.value, dropped.value


def raw_drain_games(SP, L, sp, game, A, td):
    n, rows, _ = raw_finished(L, sp)
    a = dict(slot=np.zeros(n, np.int32), length=np.zeros(n, np.int32), winner=np.zeros(n, np.int32),
             finish_ply=np.zeros(n, np.int64), row_start=np.zeros(n, np.int64), bb_p1=np.zeros(rows, np.uint64),
             bb_p2=np.zeros(rows, np.uint64), turn=np.zeros(rows, np.int8), prob=np.zeros((rows, A), np.float32),
             wdl=np.zeros((rows, 3), np.float32), mask=np.zeros((rows, A), np.uint8))
    out = RawGames(**{k: v.ctypes.data for k, v in a.items()})
    assert L.az_selfplay_drain(sp, C.byref(out), C.c_int64(n), C.c_int64(rows)) == 0, L.az_last_error()

    def rows_of(i):
        lo, hi = int(a["row_start"][i]), int(a["row_start"][i]) + int(a["length"][i]) + 1
        return (a["bb_p1"].view(np.int64)[lo:hi], a["bb_p2"].view(np.int64)[lo:hi], a["turn"][lo:hi], a["prob"][lo:hi],
                a["wdl"][lo:hi], a["mask"].view(np.bool_)[lo:hi])
    return a, SP.assemble_games(game, td, a["length"], a["winner"], a["slot"], rows_of)


def test_c_abi_alone_via_ctypes(env):
    torch, SP, RP = env["torch"], env["SP"], env["RP"]
    L = C.CDLL(os.path.join(PKG, "lib", "libaz_mcts.so"))
    L.az_last_error.restype = C.c_char_p
    vp, i64 = C.c_void_p, C.c_int64
    L.az_mcts_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.az_mcts_set_seed.argtypes = [vp, C.c_int]
    L.az_mcts_destroy.argtypes = [vp]
    L.az_mcts_destroy.restype = None
    L.az_nn_model_create_hash.argtypes = [C.c_int, C.POINTER(vp)]
    L.az_nn_model_destroy.argtypes = [vp]
    L.az_selfplay_create.argtypes = [vp, C.POINTER(RawConfig), C.POINTER(vp)]
    L.az_selfplay_destroy.argtypes = [vp]
    L.az_selfplay_destroy.restype = None
    L.az_selfplay_step.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, vp]
    L.az_selfplay_finished.argtypes = [vp, C.POINTER(i64), C.POINTER(i64), C.POINTER(i64)]
    L.az_selfplay_drain.argtypes = [vp, C.POINTER(RawGames), i64, i64]
    L.az_selfplay_totals.argtypes = [vp, C.POINTER(i64 * 5)]
    L.az_selfplay_export.argtypes = [vp, C.POINTER(RawTensors), i64, C.c_int, i64, i64, C.POINTER(RawInfo), C.POINTER(i64), vp]
    td = 2
    for game_id, game, n, n_playout, A, plies in ((0, "Connect4", 96, 16, 7, 30), (1, "Othello", 24, 8, 65, 70)):
        cap = 1009
        dev = RP.ReplayTensors(game, cap, "cuda")
        host = RP.ReplayTensors(game, cap, "cpu")
        torch.cuda.synchronize()
        tensors = RawTensors(*(getattr(dev, t).data_ptr() for t in TENSORS), cap)
        engines = []
        for _ in range(2):                                               # the exporting driver and its draining twin
            m, model, sp = vp(), vp(), vp()
            assert L.az_mcts_create(game_id, n, -1, C.byref(m)) == 0, L.az_last_error()
            assert L.az_mcts_set_seed(m, 11) == 0
            assert L.az_nn_model_create_hash(game_id, C.byref(model)) == 0
            cfg = RawConfig(1.0, 0.0, 8, 1, 1, 4, 0, 0.25, 0.05)
            assert L.az_selfplay_create(m, C.byref(cfg), C.byref(sp)) == 0, L.az_last_error()
            engines.append((m, model, sp))
        (m, model, sp), (m2, model2, twin) = engines
        ptr = 0
        exported = 0
        for _round in range(3):
            # step, count, export, and the next round's step right behind it: library calls only
            assert L.az_selfplay_step(sp, model, n_playout, 4, 0, plies, None) == 0, L.az_last_error()
            g, r, dropped = raw_finished(L, sp)
            assert dropped == 0
            info = dict(slot=np.zeros(g, np.int32), length=np.zeros(g, np.int32), winner=np.zeros(g, np.int32),
                        finish_ply=np.zeros(g, np.int64))
            new_ptr = i64(-1)
            assert L.az_selfplay_export(sp, C.byref(tensors), ptr, td, g, r, C.byref(RawInfo(**{k: v.ctypes.data for k, v in info.items()})),
                                        C.byref(new_ptr), None) == 0, L.az_last_error()
            assert new_ptr.value == ptr + r
            ptr = new_ptr.value
            exported += g
            assert L.az_selfplay_step(twin, model2, n_playout, 4, 0, plies, None) == 0, L.az_last_error()
            a, games = raw_drain_games(SP, L, twin, game, A, td)
            for k in info:
                assert np.array_equal(info[k], a[k]), k
            assert int(info["length"].sum()) + g == r
            host.store_games(games)
        tot = (i64 * 5)()
        assert L.az_selfplay_totals(sp, C.byref(tot)) == 0 and tot[1] == exported >= (n if game == "Connect4" else 1)
        assert raw_finished(L, sp)[:2] == (0, 0)
        dev._ptr = ptr
        assert ptr > cap
        same_buffers(dev, host)

        # the error cases: AZ_ERR_ARG (1) with a message, and the store is left as it was
        assert L.az_selfplay_step(sp, model, n_playout, 4, 0, plies, None) == 0, L.az_last_error()
        g, r, _ = raw_finished(L, sp)
        assert g > 0
        before = buffer_arrays(dev)
        assert L.az_selfplay_export(sp, C.byref(tensors), ptr, td, g + 1, r, None, None, None) == 1 and b"sizes differ" in L.az_last_error()
        assert L.az_selfplay_export(sp, C.byref(tensors), ptr, td, g, r - 1, None, None, None) == 1 and b"sizes differ" in L.az_last_error()
        bad = RawTensors(*(getattr(dev, t).data_ptr() for t in TENSORS), 0)
        assert L.az_selfplay_export(sp, C.byref(bad), ptr, td, g, r, None, None, None) == 1 and b"capacity" in L.az_last_error()
        bad = RawTensors(*(getattr(dev, t).data_ptr() for t in TENSORS), -5)
        assert L.az_selfplay_export(sp, C.byref(bad), ptr, td, g, r, None, None, None) == 1 and b"capacity" in L.az_last_error()
        for missing in TENSORS:
            bad = RawTensors(*(None if t == missing else getattr(dev, t).data_ptr() for t in TENSORS), cap)
            assert L.az_selfplay_export(sp, C.byref(bad), ptr, td, g, r, None, None, None) == 1 and b"null" in L.az_last_error(), missing
        assert L.az_selfplay_export(sp, None, ptr, td, g, r, None, None, None) == 1 and b"null" in L.az_last_error()
        assert L.az_selfplay_export(None, C.byref(tensors), ptr, td, g, r, None, None, None) == 1 and b"null" in L.az_last_error()
        assert raw_finished(L, sp)[:2] == (g, r)
        assert differences(buffer_arrays(dev), before) == []
        # info and new_ptr are optional
        assert L.az_selfplay_export(sp, C.byref(tensors), ptr, td, g, r, None, None, None) == 0, L.az_last_error()
        assert raw_finished(L, sp)[:2] == (0, 0)
        L.az_selfplay_destroy(sp)
        # a driver that does not record
        assert L.az_selfplay_create(m, C.byref(RawConfig(1.0, 0.0, 8, 1, 0, 0, 0, 0.25, 0.1)), C.byref(sp)) == 0
        assert L.az_selfplay_step(sp, model, n_playout, 4, 0, 2, None) == 0, L.az_last_error()
        assert L.az_selfplay_export(sp, C.byref(tensors), 0, td, 0, 0, None, None, None) == 1 and b"does not record" in L.az_last_error()
        L.az_selfplay_destroy(sp)
        L.az_selfplay_destroy(twin)
        for mm, mod in ((m, model), (m2, model2)):
            L.az_nn_model_destroy(mod)
            L.az_mcts_destroy(mm)


# ---------------------------------------------------------------------------------------- 6. streams

def test_streamed_export_equals_its_drivers_exported_alone(env):
    SP, RP = env["SP"], env["RP"]
    net = hash_net(env, "Connect4")
    kw = dict(n_playout=24, vl_batch=4, temp_decay_moves=6, record=True, td_steps=2)
    plies, cap = 30, 3001
    sp = SP.StreamedSelfPlay(net, 1300, streams=2, seed=3, driver="native", **kw)
    together, alone_buf = RP.ReplayTensors("Connect4", cap, "cuda"), RP.ReplayTensors("Connect4", cap, "cuda")
    sp.step(plies)
    info = sp.export(together)
    sp.synchronize()
    assert len(info["slot"]) == sp.read_totals()["games"] > 0 and info["slot"].max() >= 650
    assert sp.drain() == []
    infos = []
    for i in range(len(sp.parts)):
        alone = SP.NativeSelfPlay(net, sp.sizes[i], seed=3 * 2 + i, **kw)
        alone.step(plies)
        one = alone.export(alone_buf)
        one["slot"] = one["slot"] + np.int32(sp.offsets[i])
        infos.append(one)
    for k in info:
        assert np.array_equal(info[k], np.concatenate([x[k] for x in infos])), k
    assert together._ptr > cap
    same_buffers(together, alone_buf)
    sp.close()
    python_drivers = SP.StreamedSelfPlay(net, 64, streams=1, seed=3, driver="device", record=True)
    with pytest.raises(AssertionError):
        python_drivers.export(together)
    python_drivers.close()
