"""The device driver's ply tail as native launches (az_game_dev_pick and az_mcts_dev_ply_advance in include/az_mcts.h,
k_ply_pick and k_ply_advance in csrc/kernels.hip) against the torch tail it replaces, which AZ_PLY_TAIL=0 keeps.

1. two `DeviceSelfPlay` on the hash evaluator with one seed, one on each tail, B = 193 (a partial last wavefront
   and workgroup): after every one of 12 plies the moves, the visit counts, the positions, the ply counters, done,
   winner, the totals and the state of the torch generator are EQUAL (integers and bytes: no tolerance).  Games end
   inside the window, so the restart of a finished game (or, with refill off, its slot going dead with move -1)
   runs; a third setting makes the greedy branch run from ply 3 on.
2. the pick alone on hand-made counts - a row of zeros, a single non-zero entry, equal maxima, a count of n_playout -
   against torch.multinomial from the same generator state, and the greedy move against the lowest arg-max.
3. a driver whose temperature is not exactly 1 stays on torch's pick, and plays.
"""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")

B, N_PLAYOUT, VL, PLIES = 193, 16, 4, 12
FIELDS = ("actions", "counts", "bb_p1", "bb_p2", "turn", "ply", "done", "winner", "totals")


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import torch
    from src import fused, hash_eval, selfplay
    return dict(torch=torch, F=fused, H=hash_eval, SP=selfplay, L=fused.lib())


def driver(env, monkeypatch, tail, **kw):
    if tail:
        monkeypatch.delenv("AZ_PLY_TAIL", raising=False)
    else:
        monkeypatch.setenv("AZ_PLY_TAIL", "0")
    sp = env["SP"].DeviceSelfPlay(env["H"].HashEvaluator("cuda"), B, n_playout=N_PLAYOUT, vl_batch=VL, seed=11, **kw)
    monkeypatch.delenv("AZ_PLY_TAIL", raising=False)
    return sp


@pytest.mark.parametrize("kw", [dict(), dict(refill=False), dict(temp_decay_moves=3, temp_endgame=0)],
                         ids=["refill", "dead_slots", "greedy_from_ply_3"])
def test_native_tail_plays_the_torch_tails_games(env, monkeypatch, kw):
    torch = env["torch"]
    new, old = driver(env, monkeypatch, True, **kw), driver(env, monkeypatch, False, **kw)
    assert new._native_pick and new._native_advance and not old._native_pick and not old._native_advance
    kept = {f: getattr(new, f) for f in FIELDS + ("dead",)}
    minus_ones = 0
    for ply in range(PLIES):
        dead_before = new.dead.clone()
        new.step()
        old.step()
        assert torch.equal(new.actions == -1, dead_before), "ply %d: move -1 exactly in the dead slots" % ply
        minus_ones += int(dead_before.sum())
        for f in FIELDS:
            a, b = getattr(new, f), getattr(old, f)
            assert a.dtype == b.dtype and a.shape == b.shape, (ply, f)
            assert torch.equal(a, b), "ply %d: %s differs in %d places" % (ply, f, int((a != b).sum()))
        assert torch.equal(new.dead, old.dead), ply
        assert torch.equal(new.gen.get_state(), old.gen.get_state()), "ply %d: the generators moved apart" % ply
    # the native tail updates the driver's tensors in place
    assert all(getattr(new, f) is t for f, t in kept.items())
    tot = new.read_totals()
    assert tot["positions"] == PLIES * B
    assert tot["games"] >= 1, "no game ended inside the window: refill / death never ran"
    assert tot["games"] == tot["p1_wins"] + tot["p2_wins"] + tot["draws"]
    if kw.get("refill", True):
        assert minus_ones == 0 and int((new.ply < PLIES).sum()) == tot["games"]
    else:
        assert int(new.dead.sum()) == tot["games"]
        assert minus_ones >= 1, "no dead slot was ever given the move -1"


def test_pick_is_torch_multinomial_and_the_lowest_argmax(env):
    torch, F, L = env["torch"], env["F"], env["L"]
    A = 7
    rows = [[0, 0, 0, 0, 0, 0, 0],                         # nothing visited: uniform over all seven
            [0, 0, 0, 0, N_PLAYOUT, 0, 0],                 # one entry, and it holds every playout
            [0, 5, 0, 5, 1, 5, 0],                         # equal maxima: the greedy move is the lowest
            [3, 3, 3, 3, 3, 3, 3],
            [1, 0, 0, 0, 0, 0, N_PLAYOUT - 1],
            [0, 0, 0, 0, 0, 0, 1],
            [2, 1, 4, 1, 6, 1, 1]]
    n = 520                                                # more than two workgroups, the last one partial
    counts = torch.tensor(rows, dtype=torch.int32, device="cuda").repeat((n + len(rows) - 1) // len(rows), 1)[:n].contiguous()
    ply = (torch.arange(n, device="cuda", dtype=torch.int32) % 6).contiguous()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    state = gen.get_state()
    # the driver's torch chain at temperature 1
    visits = counts.to(torch.float32)
    w = torch.where(visits > 0, visits, torch.zeros_like(visits))
    safe = torch.where(w.sum(1, keepdim=True) > 0, w, torch.ones_like(w))
    want_sampled = torch.multinomial(safe, 1, generator=gen).squeeze(1).to(torch.int32)
    after = gen.get_state()
    want_greedy = visits.argmax(dim=1).to(torch.int32)
    lowest = torch.tensor([r.index(max(r)) for r in rows], dtype=torch.int32, device="cuda")
    assert torch.equal(want_greedy[:len(rows)], lowest)
    # the native pick from the same generator state
    gen.set_state(state)
    q = torch.empty((n, A), dtype=torch.float32, device="cuda")
    q.exponential_(1.0, generator=gen)
    assert torch.equal(gen.get_state(), after), "exponential_ on (n, A) moves the generator as multinomial does"
    actions = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    dead = torch.zeros(n, dtype=torch.bool, device="cuda")
    dead[3::50] = True

    def pick(decay, hot_early, hot_late, dead_ptr):
        actions.fill_(-7)
        F.check(L.az_game_dev_pick(0, counts.data_ptr(), q.data_ptr(), ply.data_ptr(), dead_ptr, actions.data_ptr(), n,
                                   decay, hot_early, hot_late, F._stream()))
        return actions.clone()

    assert torch.equal(pick(0, 1, 0, None), want_sampled)
    assert torch.equal(pick(0, 0, 1, None), want_greedy)
    mixed = torch.where(ply < 3, want_sampled, want_greedy)
    assert torch.equal(pick(3, 1, 0, None), mixed)
    assert torch.equal(pick(3, 1, 0, dead.data_ptr()), mixed.masked_fill(dead, -1))
    # a sampled move is a visited one, or any at all in a row of zeros
    got = pick(0, 1, 0, None).long()
    some = counts.sum(1) > 0
    assert bool((counts.gather(1, got.unsqueeze(1)).squeeze(1)[some] > 0).all())
    assert got[~some].unique().numel() > 1


def test_other_temperatures_keep_torchs_pick(env, monkeypatch):
    sp = env["SP"].DeviceSelfPlay(env["H"].HashEvaluator("cuda"), 64, n_playout=N_PLAYOUT, vl_batch=VL, seed=2,
                                  temperature=0.8)
    assert not sp._native_pick and sp._native_advance
    late = env["SP"].DeviceSelfPlay(env["H"].HashEvaluator("cuda"), 64, n_playout=N_PLAYOUT, vl_batch=VL, seed=2,
                                    temp_decay_moves=4, temp_endgame=0.5)
    assert not late._native_pick
    for _ in range(9):
        sp.step()
    tot = sp.read_totals()
    assert tot["positions"] == 9 * 64
    act = sp.actions.cpu()
    assert bool(((act >= 0) & (act < 7)).all())
    assert int(sp.ply.max()) <= 9 and int((sp.bb_p1 & sp.bb_p2).abs().sum()) == 0
