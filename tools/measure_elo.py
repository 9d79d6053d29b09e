#!/usr/bin/env python3
"""The rating step on the device: what the one-kernel rollout search buys, in ONE warm process.

(a) The search alone.  Both games, B in {1, 256, 4096} trees, `--playouts` (1000) playouts from the initial position
    with the rollout player's configuration (player.py:84-88), two routes alternately, `--windows` (7) windows each
    after one warm-up of both:

      per_sim   az_mcts_search_rollout_dev: k_select, k_rollout, k_backprop, k_bump_call per simulation
      one       az_mcts_dev_import_roots + az_mcts_dev_rollout_search: k_rollout_search per chunk, one bump

    A window is a host clock from an idle device to a synchronise; trees are reset in between.  Reported per case:
    median / min / max of the windows in ms, `one_faster` = the one-kernel route's median lies below the other
    route's by more than that route's own min-max spread, and us_per_sim of the one-kernel route (the window's median
    over the playouts: what one simulation of the slowest tree costs a launch - the figure behind the chunk constant
    of az_mcts_dev_rollout_search).  `claim` is true when every case is `one_faster`.

(b) A rating round.  `match.rating_games` with a hash-evaluator network, `--games` (256) games per colour, against
    the per-ply Python loop over the wrapper - `Game.play`'s shape (game.py: the side to move searches, plays its
    most visited move, both players start over) with the games in lock step: `batch_playout(fused=True)` for the
    network side, `rollout_playout` with device playouts for the rollout side, numpy boards stepped per game.

One JSON line on stdout (kept under profiles/ when run on an MI355X); progress on stderr.

    python tools/measure_elo.py [--playouts N] [--windows N] [--games N] [--sizes 1,256,4096] [--skip-round | --skip-search]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
for p in (PKG, ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def log(msg):
    sys.stderr.write("[elo] %s\n" % msg)
    sys.stderr.flush()


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--playouts", type=int, default=1000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--sizes", default="1,256,4096")
    ap.add_argument("--round-playouts", type=int, default=64, help="the network side's n_playout in (b)")
    ap.add_argument("--round-rollouts", type=int, default=200, help="the rollout side's n_playout in (b)")
    ap.add_argument("--skip-round", action="store_true")
    ap.add_argument("--skip-search", action="store_true")
    a = ap.parse_args()

    import numpy as np
    import torch
    from src import abi as F, hash_eval, mcts_cpp
    from src.MCTS_cpp import BatchedMCTS
    from src.match import rating_games
    import scenarios as S
    L = F.lib()

    player = dict(c_init=1.0, c_base=500.0, dirichlet_alpha=0.0, noise_epsilon=0.0, fpu_reduction=0.0, use_symmetry=False)

    def search_case(game, B):
        cls = mcts_cpp.BatchedMCTS_Othello if game == "Othello" else mcts_cpp.BatchedMCTS_Connect4
        board = S.ot_start() if game == "Othello" else np.zeros((6, 7), np.int8)
        boards = np.ascontiguousarray(np.tile(board, (B, 1, 1)), np.int8)
        turns = np.ones(B, np.int32)
        d_boards, d_turns = torch.from_numpy(boards).cuda(), torch.from_numpy(turns).cuda()
        ones = torch.ones(B, dtype=torch.uint8, device="cuda")
        engines = {}
        for name in ("per_sim", "one"):
            m = cls(B)
            S.apply_cfg(m, player)
            m.set_seed(1)
            engines[name] = m

        def window(name):
            m, used = engines[name], C.c_int64()
            F.check(L.az_mcts_dev_reset_masked(m.handle, ones.data_ptr(), F._stream()))
            F.check(L.az_mcts_max_used(m.handle, C.byref(used)))      # waits; the host-side bound starts over with the trees
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "per_sim":
                F.check(L.az_mcts_search_rollout_dev(m.handle, boards.ctypes.data, turns.ctypes.data, B, a.playouts))
            else:
                F.check(L.az_mcts_dev_import_roots(m.handle, d_boards.data_ptr(), d_turns.data_ptr(), F._stream()))
                F.check(L.az_mcts_dev_rollout_search(m.handle, a.playouts, 0, F._stream()))
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0)
        for name in engines:
            log("%s B=%d warm-up %s: %.1f ms" % (game, B, name, window(name)))
        ms = {k: [] for k in engines}
        for _ in range(a.windows):
            for name in engines:
                ms[name].append(window(name))
        per_sim, one = spread(ms["per_sim"]), spread(ms["one"])
        faster = one["median"] < per_sim["median"] - (per_sim["max"] - per_sim["min"])
        log("%s B=%d per_sim %.1f ms  one %.1f ms  one_faster=%s" % (game, B, per_sim["median"], one["median"], faster))
        return dict(game=game, trees=B, per_sim_ms=per_sim, one_ms=one, one_faster=bool(faster),
                    us_per_sim=1e3 * one["median"] / max(1, a.playouts))

    out = dict(tool="measure_elo", playouts=a.playouts, windows=a.windows)
    if not a.skip_search:
        out["search"] = [search_case(g, int(b)) for g in ("Connect4", "Othello") for b in a.sizes.split(",")]
        out["claim"] = all(c["one_faster"] for c in out["search"])

    if not a.skip_round:
        net = hash_eval.HashEvaluator("cuda", salt=7)
        n, n_net, n_roll = a.games, a.round_playouts, a.round_rollouts

        def native(seed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            first, second = rating_games(net, n, n_net, n_roll, vl_batch=4, seed=seed)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, first, second

        def python_match(seed, net_side):
            az = BatchedMCTS(n, c_init=1.25, c_base=500, alpha=0.3, n_playout=n_net, noise_epsilon=0.0)
            ro = BatchedMCTS(n, c_init=1, c_base=500, alpha=0, n_playout=n_roll, noise_epsilon=0.0, fpu_reduction=0.0,
                             use_symmetry=False)
            az.seed(seed); ro.seed(seed + 1)
            ro._get_rollout_evaluator().device_rng = True
            boards = np.zeros((n, 6, 7), np.int8)
            live, winner, turn = np.ones(n, bool), np.zeros(n, np.int32), 1
            while live.any():
                turns = np.full(n, turn, np.int32)
                if turn == net_side:
                    az.batch_playout(net, boards, turns, vl_batch=4, fused=True)
                    visits = az.get_visits_count()
                else:
                    ro.rollout_playout(boards, turns)
                    visits = ro.get_visits_count()
                moves = visits.argmax(1)
                for i in np.nonzero(live)[0]:
                    S.np_drop(boards[i], int(moves[i]), turn)
                    if S.np_done(boards[i]):
                        live[i], winner[i] = False, S.np_winner(boards[i])
                        boards[i] = 0
                for i in range(n):                               # game.py:41: both players start over after every move
                    az.reset_env(i); ro.reset_env(i)
                turn = -turn
            return winner

        def python(seed):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            first, second = python_match(seed, 1), python_match(seed + 2, -1)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, first, second
        routes = dict(native=native, python=python)
        for name, fn in routes.items():
            log("rating round warm-up %s: %.2f s" % (name, fn(100)[0]))
        secs = {k: [] for k in routes}
        for r in range(3):
            for name, fn in routes.items():
                secs[name].append(fn(r)[0])
                log("rating round %s rep %d: %.2f s" % (name, r, secs[name][-1]))
        out["rating_round"] = dict(games_per_colour=n, n_playout=n_net, pure_mcts_n_playout=n_roll,
                                   native_s=spread(secs["native"]), python_s=spread(secs["python"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
