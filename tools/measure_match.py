#!/usr/bin/env python3
"""Evaluation matches between two networks: the native match driver against what a user does today, in ONE process.

Connect4, two random-init networks (HIP inference twins), `--games` games (4096), n_playout 200, virtual-loss batch 4,
the reference's evaluation settings (c_base 500, noise epsilon 0.05, temperature 0.2, symmetry on).  Two routes,
alternately, `--reps` times each after one warm-up of both:

  native   `EvaluationMatch.play()`: az_match_step, the ply tail in one kernel (k_match_ply), the host asks how many
           games are left every few plies
  python   the reference's `_batched_eval_games` loop (tests/match_harness.py, the restatement the suite pins to
           the compiled reference) over this project's `BatchedMCTS` wrapper with `fused=True` and the `Env`
           objects: per-ply Python, one numpy draw per game

Each route is timed by a host clock from an idle device to a device synchronise.  The two routes draw their moves
from different generators, so their games differ; rates are per route.

  games_per_s, positions_per_s   median / min / max over the repetitions
  host_ms_per_ply                the route's wall time over the plies it played (longest game)

With `--trees K` (root-parallel play, player.py:248-283) or `--ensemble` (one tree per board symmetry, player.py:285-329)
both players bring a team of trees per game: the native route is the team match (az_match_create_teams), the python
route tests/team_harness.py's `team_eval_games` - the same per-ply loop with the roots spread, the visits summed and the
moves mapped per tree in numpy.  Root-parallel trees keep noise epsilon 0.05, an ensemble plays without noise and with the
engine's own symmetry off, as `AlphaZeroPlayer.eval()` and `_make_mcts` set them.

One JSON line on stdout (kept under profiles/ when run on an MI355X); progress on stderr.

    python tools/measure_match.py [--games N] [--n-playout N] [--vl-batch K] [--reps N] [--trees K | --ensemble]
"""
import argparse
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
    sys.stderr.write("[match] %s\n" % msg)
    sys.stderr.flush()


def spread(xs):
    return dict(median=statistics.median(xs), min=min(xs), max=max(xs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--games", type=int, default=4096)
    ap.add_argument("--n-playout", type=int, default=200)
    ap.add_argument("--vl-batch", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trees", type=int, default=1, help="trees per game and player (root-parallel play)")
    ap.add_argument("--ensemble", action="store_true", help="both players are the game's symmetry ensemble (two trees per game)")
    a = ap.parse_args()
    team = (2, True) if a.ensemble else (max(1, a.trees), False)
    eps, use_symmetry = (0.0, False) if a.ensemble else (0.05, True)

    import numpy as np
    import torch
    from src import az_net
    from src.MCTS_cpp import BatchedMCTS
    from src.env_cpp.connect4 import Env
    from src.match import EvaluationMatch
    import match_harness as MH
    import team_harness as TH

    def net(seed):
        torch.manual_seed(seed)
        return az_net.Connect4Net(device="cuda").eval()
    nets = (net(1), net(2))
    search = dict(c_init=1.25, c_base=500, alpha=0.3)

    def native(seed):
        mt = EvaluationMatch(nets[0], nets[1], a.games, n_playout=a.n_playout, vl_batch=a.vl_batch, eval_noise_eps=eps,
                             eval_temp=0.2, use_symmetry=use_symmetry, seed=seed, n_trees=team[0], sym_ensemble=team[1], **search)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mt.play()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        res = mt.results()
        return dt, int(res["length"].sum()), int(res["length"].max())

    def python(seed):
        ws = [BatchedMCTS(a.games * team[0], n_playout=a.n_playout, noise_epsilon=eps, use_symmetry=use_symmetry, **search)
              for _ in range(2)]
        for i, w in enumerate(ws):
            w.seed(seed + i)
        np.random.seed(seed)

        class Fused:                                     # the wrapper's device loop, as a user asks for it
            def __init__(self, w):
                self.w = w

            def __getattr__(self, k):
                return getattr(self.w, k)

            def batch_playout(self, pv, boards, turns, vl_batch=1):
                return self.w.batch_playout(pv, boards, turns, vl_batch=vl_batch, fused=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if team == (1, False):
            out = MH.batched_eval_games(Fused(ws[0]), Fused(ws[1]), nets[0], nets[1], Env, a.games, vl_batch=a.vl_batch, eval_temp=0.2)
        else:
            out = TH.team_eval_games(Fused(ws[0]), Fused(ws[1]), nets[0], nets[1], Env, a.games, "Connect4", teams=(team, team),
                                     vl_batch=a.vl_batch, eval_temp=0.2)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        return dt, int(out["length"].sum()), int(out["length"].max())

    routes = dict(native=native, python=python)
    for name, fn in routes.items():
        log("warm-up %s: %.2f s" % (name, fn(100)[0]))
    runs = {k: [] for k in routes}
    for r in range(a.reps):
        for name, fn in routes.items():
            runs[name].append(fn(r))
            log("%s rep %d: %.2f s, %d positions, %d plies" % ((name, r) + runs[name][-1]))
    out = dict(tool="measure_match", game="Connect4", games=a.games, n_playout=a.n_playout, vl_batch=a.vl_batch, reps=a.reps,
               trees=team[0], ensemble=team[1])
    for name, rs in runs.items():
        out[name] = dict(games_per_s=spread([a.games / dt for dt, _, _ in rs]),
                         positions_per_s=spread([pos / dt for dt, pos, _ in rs]),
                         host_ms_per_ply=spread([1e3 * dt / plies for dt, _, plies in rs]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
