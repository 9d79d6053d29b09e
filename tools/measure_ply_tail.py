#!/usr/bin/env python3
"""The ply tail of self-play, Python driver against native driver, in ONE process.

bench.py's config 1 (Connect4, 8192 games, n_playout 200, vl_batch 4, the reference's CNN) - `--othello`:
config 3 (Othello, 4096 games, n_playout 400, score utility 0.15, OthelloNet) - run through `DeviceSelfPlay`
(what bench.py times) and through `NativeSelfPlay` (az_selfplay_step), alternately, warm, `--reps` times each:

  positions_per_s        `--plies` plies back to back, the stream drained once at the end
  host_enqueue_ms        wall time of ONE step() call on an idle stream (the host only enqueues: nothing it
                         waits for is outstanding), mean over `--enqueue-samples` calls per repetition
  tail_launches_per_ply  device activities (kernels, copies, memsets) of a ply that are not the search: a ply
                         under torch.profiler minus a bare FusedSearch.search() of the same engine

One JSON line on stdout (kept under profiles/); progress on stderr.  `--record` turns recording on in both.

    python tools/measure_ply_tail.py [--othello] [--record] [--games N] [--n-playout N] [--plies N] [--reps N]
                                     [--trees K | --ensemble]

`--trees K [--ensemble]` compares two NATIVE drivers instead: "team" - `NativeSelfPlay(n_trees=K)` (or the game's symmetry
ensemble, K trees) on `--games` games (default: the config's games // K) - against "single", the same driver with one tree
per game and K times the games, i.e. the same number of trees in the engine.  Both search the same number of trees per ply
and the team plays a K-th of the positions, so the expectation to confirm or refute is: the tail's launch count is the same,
and the time per ply follows the number of trees searched (ply_ms about equal, positions/s about 1/K).

`--trace-only DRIVER` plays `--plies` plies with one driver and exits: the program to put behind
`rocprofv3 --kernel-trace --stats --` for the tail's device time per ply (k_sp_* against the torch kernels).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

from src import selfplay as SP  # noqa: E402


def log(msg):
    sys.stderr.write("[ply-tail] %s\n" % msg)
    sys.stderr.flush()


def make_net(args, dev):
    torch.manual_seed(1234)
    if args.evaluator == "hash":
        from src.hash_eval import HashEvaluator, OthelloHashEvaluator
        return (OthelloHashEvaluator if args.othello else HashEvaluator)(dev)
    from src.az_net import Connect4Net, OthelloNet
    if args.othello:
        return OthelloNet(device=dev).to(memory_format=torch.channels_last)
    return Connect4Net(device=dev).eval()


def make_driver(kind, net, args):
    kw = dict(n_playout=args.n_playout, vl_batch=4, seed=0, record=args.record)
    if args.othello:
        kw.update(game="Othello", score_utility_factor=0.15, score_scale=8.0)
    if kind == "team":
        return SP.NativeSelfPlay(net, args.games, n_trees=args.trees, sym_ensemble=args.ensemble, **kw)
    if kind == "single":
        return SP.NativeSelfPlay(net, args.games * args.trees, **kw)
    cls = SP.NativeSelfPlay if kind == "native" else SP.DeviceSelfPlay
    return cls(net, args.games, **kw)


def step(sp, n):
    if isinstance(sp, SP.NativeSelfPlay):
        sp.step(n)
    else:
        for _ in range(n):
            sp.step()


def device_activities(fn):
    """Kernels, copies and memsets the device ran for fn()."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA"))


def tail_launches(sp):
    ply = device_activities(lambda: step(sp, 1))
    # a bare search on the same engine and roots (its results are thrown away by the next ply's re-rooting;
    # measured last, after the timed repetitions)
    search = device_activities(lambda: sp.fused.search(sp.n_playout, sp.vl_batch))
    return ply - search, ply, search


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--othello", action="store_true")
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--evaluator", choices=["cnn", "hash"], default="cnn")
    ap.add_argument("--games", type=int, default=None)
    ap.add_argument("--n-playout", type=int, default=None)
    ap.add_argument("--plies", type=int, default=None)
    ap.add_argument("--lead-in", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--enqueue-samples", type=int, default=4)
    ap.add_argument("--no-launch-count", action="store_true")
    ap.add_argument("--trace-only", choices=["device", "native"], default=None)
    ap.add_argument("--trees", type=int, default=1, help="compare a team of K trees per game with single trees (see above)")
    ap.add_argument("--ensemble", action="store_true", help="the team is the game's symmetry ensemble (K = 2 / 4)")
    args = ap.parse_args()
    if args.ensemble:
        args.trees = 4 if args.othello else 2
    teams = args.trees > 1
    assert not (teams and args.trace_only), "--trace-only takes no team"
    args.games = args.games or (4096 if args.othello else 8192) // args.trees
    args.n_playout = args.n_playout or (400 if args.othello else 200)
    args.plies = args.plies or (3 if args.othello else 20)
    args.lead_in = (2 if args.othello else 12) if args.lead_in is None else args.lead_in
    assert args.reps >= 3 or args.trace_only, "at least three repetitions per driver"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    net = make_net(args, dev)

    if args.trace_only:
        sp = make_driver(args.trace_only, net, args)
        step(sp, args.lead_in + args.plies)
        torch.cuda.synchronize()
        print(json.dumps({"driver": args.trace_only, "plies": args.lead_in + args.plies, "totals": sp.read_totals()}), flush=True)
        return

    kinds = ("team", "single") if teams else ("device", "native")
    drivers = {k: make_driver(k, net, args) for k in kinds}
    for k, sp in drivers.items():
        t = time.perf_counter()
        step(sp, args.lead_in)
        torch.cuda.synchronize()
        log("%s: lead-in of %d plies in %.2f s" % (k, args.lead_in, time.perf_counter() - t))
    res = {k: dict(positions_per_s=[], ply_ms=[], host_enqueue_ms=[]) for k in drivers}
    for rep in range(args.reps):
        for k, sp in drivers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(sp, args.plies)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            res[k]["positions_per_s"].append(sp.B * args.plies / el)
            res[k]["ply_ms"].append(el / args.plies * 1e3)
            enq = []
            for _ in range(args.enqueue_samples):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                step(sp, 1)
                enq.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            res[k]["host_enqueue_ms"].append(statistics.mean(enq))
            log("rep %d %s: %.0f positions/s, %.2f ms host enqueue per ply" % (rep, k, res[k]["positions_per_s"][-1], res[k]["host_enqueue_ms"][-1]))
    out = {"tool": "measure_ply_tail", "game": "Othello" if args.othello else "Connect4", "games": args.games,
           "n_playout": args.n_playout, "vl_batch": 4, "evaluator": args.evaluator, "record": args.record,
           "plies_per_repetition": args.plies, "repetitions": args.reps, "lead_in_plies": args.lead_in,
           "native_model": drivers[kinds[1]].fused._native_model() is not None}
    if teams:
        out.update(trees=args.trees, ensemble=args.ensemble, trees_in_engine=args.games * args.trees)
    for k, r in res.items():
        d = {}
        for name, v in r.items():
            d[name] = {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                       "all": [round(x, 3) for x in v]}
        if not args.no_launch_count:
            try:
                tail, ply, search = tail_launches(drivers[k])
                d["tail_launches_per_ply"] = tail
                d["launches_per_ply"] = ply
                d["launches_per_search"] = search
            except Exception as e:                                     # a profiler that cannot see the device
                d["tail_launches_per_ply"] = None
                d["tail_launches_error"] = repr(e)
        out[k] = d
    if teams:
        pt, ps = out["team"]["ply_ms"], out["single"]["ply_ms"]
        out["team_ply_ms_over_single"] = round(pt["median"] / ps["median"], 4)
        out["single_spread"] = round((ps["max"] - ps["min"]) / ps["median"], 4)
    else:
        pd, pn = out["device"]["positions_per_s"], out["native"]["positions_per_s"]
        out["native_over_device"] = round(pn["median"] / pd["median"], 4)
        out["device_spread"] = round((pd["max"] - pd["min"]) / pd["median"], 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
