"""The copy of a kept subtree into a tree's other arena half (k_prune, csrc/kernels.hip) leaves nothing observable
behind: the same seeded self-play, once in an arena so large that no tree is ever copied and once with every tree
copied at every re-rooting, gives the same visit counts, moves and root statistics ply for ply.

What forces the copies: the arena of an engine never has fewer than 4096 records per half, which a Connect4 tree of
64 playouts per ply fills only every seventh ply or so, so a small `reserve_slots` alone would copy next to nothing.
The small run therefore keeps the smallest arena (reserve_slots=1) AND sets AZ_COMPACT_ALWAYS=1, the engine's switch
for compact_above = 0.  The test does not trust the switch: it reads the engine's occupancy (az_mcts_max_used) after
every ply.  A tree that was copied occupies its kept subtree only; a tree that re-rooted in place keeps everything
it allocated since its game began (the old root and the siblings of the move played at the least, so strictly more).
The games being equal, the copied run's largest tree must lie strictly below the in-place run's after every ply.
After eight plies the in-place tree holds eight plies' allocations and the copied one the subtree under the last
move - about one ply's worth plus the visits it inherited, a geometric tail - so the test also asks for a factor of
two between them; if the two runs re-rooted alike, it fails.

Othello (up to 33+ edges per node) runs the chunked form of the copy, Connect4 the whole-block form.
"""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")

PLIES, N_PLAYOUT = 8, 64


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


def run(env, game, n_games, reserve_slots):
    """[(counts, actions, root stats as bits)] per ply, the occupancy after every ply, the capacity at the end."""
    F, L, C = env["F"], env["L"], env["F"].C
    net = env["H"].HashEvaluator("cuda") if game == "Connect4" else env["H"].OthelloHashEvaluator("cuda")
    # a recording driver reads az_mcts_dev_root_stats on every ply, before the re-rooting
    sp = env["SP"].DeviceSelfPlay(net, n_games, n_playout=N_PLAYOUT, vl_batch=4, seed=9, game=game, record=True,
                                  max_finished_games=n_games, reserve_slots=reserve_slots)
    plies, occupancy = [], []
    for _ in range(PLIES):
        sp.step()
        plies.append((sp.counts.clone(), sp.actions.clone(), sp.stats.view(env["torch"].int32).clone()))
        used = C.c_int64()
        F.check(L.az_mcts_max_used(sp.h, C.byref(used)))
        occupancy.append(used.value)
    # the sticky error word: asked for, and read once it has arrived
    F.check(L.az_mcts_dev_check(sp.h, F._stream()))
    env["torch"].cuda.synchronize()
    F.check(L.az_mcts_dev_check(sp.h, F._stream()))
    return plies, occupancy, int(L.az_mcts_capacity(sp.h)), sp.search.action_size


@pytest.mark.parametrize("game,n_games", [("Connect4", 130), ("Othello", 66)])
def test_copied_trees_search_as_trees_left_in_place(env, monkeypatch, game, n_games):
    torch = env["torch"]
    monkeypatch.delenv("AZ_COMPACT_ALWAYS", raising=False)
    big, big_used, big_S, A = run(env, game, n_games, 1 << 16)
    monkeypatch.setenv("AZ_COMPACT_ALWAYS", "1")
    small, small_used, small_S, _ = run(env, game, n_games, 1)
    monkeypatch.delenv("AZ_COMPACT_ALWAYS", raising=False)
    print("%s: capacity %d / %d, occupancy in place %s, copied %s" % (game, big_S, small_S, big_used, small_used))
    assert big_S >= 1 << 16 and small_S < big_S
    # in the large arena nothing was ever past compact_above = S - 2 plies' growth: every re-rooting was in place
    assert max(big_used) + 2 * N_PLAYOUT * A < big_S
    for p in range(PLIES):
        assert 1 < small_used[p] < big_used[p], "ply %d: the copy dropped nothing (%d, %d)" % (p, small_used[p], big_used[p])
    # in place a tree only grows while its game lasts; copied, it shrinks to its subtree at every ply
    assert big_used[-1] > 2 * max(small_used), "the two runs re-root alike"
    for p, (a, b) in enumerate(zip(big, small)):
        for name, x, y in zip(("counts", "actions", "root stats"), a, b):
            assert torch.equal(x, y), "%s, ply %d: %s differ in %d places" % (game, p, name, int((x != y).sum()))
