#!/usr/bin/env python3
"""Finished games into a learner's replay buffer on the same GPU: the device route against the host route, in
ONE process.

bench.py's config 1 (Connect4, 8192 games, n_playout 200, vl_batch 4, the reference's CNN) through
`NativeSelfPlay` with `record=True`, warm.  A repetition plays `--plies` plies (timed, for the ply's wall time and
the rate of finished games), then empties the finished store by one of two routes, alternately, `--reps` times each:

  export   `NativeSelfPlay.export(buffer)`: k_sp_export writes the rows into a ReplayTensors on the device
  host     `drain()` (device to host, the reference's play_data tuples) + `ReplayTensors.store_games` into a host
           buffer + upload of the ring slots that were written (at most two slices per tensor) into the same
           device buffer - the route that existed before the export

Each route is timed by a host clock from an idle device to a device synchronise.

  rows_per_s             rows (positions + end states) that reached the device buffer per second of the route
  share_of_play_time     the route's seconds over the seconds of the plies that produced its games
  bytes_per_row          what k_sp_export reads and writes per row, from the shapes (no counter)

One JSON line on stdout (kept under profiles/); progress on stderr.

    python tools/measure_export.py [--othello] [--games N] [--n-playout N] [--plies N] [--reps N] [--capacity N]

`--trace-only` plays and exports `--reps` times and exits: the program to put behind `rocprofv3 --kernel-trace
--stats --` for the kernel's device time; it prints the rows and calls, and `--kernel-stats CSV --rows N` turns
that run's kernel_stats.csv into microseconds per call and bytes per second.
"""
import argparse
import csv
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


def log(msg):
    sys.stderr.write("[export] %s\n" % msg)
    sys.stderr.flush()


def bytes_per_row(game, td_steps):
    """Bytes k_sp_export reads from the finished store and writes to the ring for one row."""
    A, cells = (7, 42) if game == "Connect4" else (65, 64)
    read = 8 + 8 + 1 + 4 * A + 12 + A + (12 if td_steps > 0 else 0)
    write = 3 * cells + 4 * A + 1 + 2 + 2 + 12 + A + 12
    return read, write


def kernel_stats(path, rows, game, td_steps):
    for rec in csv.DictReader(open(path)):
        if "k_sp_export" in rec["Name"]:
            calls, total_ns = int(rec["Calls"]), float(rec["TotalDurationNs"])
            rd, wr = bytes_per_row(game, td_steps)
            return {"tool": "measure_export", "kernel": "k_sp_export", "game": game, "calls": calls, "rows": rows,
                    "total_us": round(total_ns / 1e3, 2), "avg_us": round(total_ns / 1e3 / calls, 2),
                    "min_us": round(float(rec["MinNs"]) / 1e3, 2), "max_us": round(float(rec["MaxNs"]) / 1e3, 2),
                    "bytes_read_per_row": rd, "bytes_written_per_row": wr,
                    "rows_per_s": round(rows / (total_ns * 1e-9)), "bytes_per_s": round(rows * (rd + wr) / (total_ns * 1e-9))}
    raise SystemExit("no k_sp_export in %s" % path)


def summary(v, digits=3):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "all": [round(x, digits) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--othello", action="store_true")
    ap.add_argument("--evaluator", choices=["cnn", "hash"], default="cnn")
    ap.add_argument("--games", type=int, default=None)
    ap.add_argument("--n-playout", type=int, default=None)
    ap.add_argument("--plies", type=int, default=None)
    ap.add_argument("--lead-in", type=int, default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--td-steps", type=int, default=2)
    ap.add_argument("--capacity", type=int, default=1 << 18)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--rows", type=int, default=0)
    args = ap.parse_args()
    game = "Othello" if args.othello else "Connect4"
    if args.kernel_stats:
        print(json.dumps(kernel_stats(args.kernel_stats, args.rows, game, args.td_steps)), flush=True)
        return
    args.games = args.games or (4096 if args.othello else 8192)
    args.n_playout = args.n_playout or (400 if args.othello else 200)
    args.plies = args.plies or (3 if args.othello else 6)
    args.lead_in = (60 if args.othello else 14) if args.lead_in is None else args.lead_in
    assert args.reps >= 3, "at least three repetitions per route"

    import torch
    from src import replay as RP, selfplay as SP
    assert torch.cuda.is_available(), "measure_export needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(1234)
    if args.evaluator == "hash":
        from src.hash_eval import HashEvaluator, OthelloHashEvaluator
        net = (OthelloHashEvaluator if args.othello else HashEvaluator)(dev)
    else:
        from src.az_net import Connect4Net, OthelloNet
        net = OthelloNet(device=dev).to(memory_format=torch.channels_last) if args.othello else Connect4Net(device=dev).eval()
    kw = dict(n_playout=args.n_playout, vl_batch=4, seed=0, record=True, td_steps=args.td_steps)
    if args.othello:
        kw.update(game="Othello", score_utility_factor=0.15, score_scale=8.0)
    sp = SP.NativeSelfPlay(net, args.games, **kw)
    on_dev = RP.ReplayTensors(game, args.capacity, dev)
    on_host = RP.ReplayTensors(game, args.capacity, "cpu")

    def route_export():
        return int(sp.export(on_dev)["length"].sum())

    def route_host():
        at = on_dev._ptr
        on_host._ptr = at
        games = sp.drain()
        n = on_host.store_games(games)
        cap = args.capacity
        lo, hi = at % cap, (at + min(n, cap)) % cap
        spans = [(lo, hi)] if lo < hi else [(lo, cap), (0, hi)]
        for name in RP.ReplayTensors.TENSORS:
            for a, b in spans:
                if b > a:
                    getattr(on_dev, name)[a:b].copy_(getattr(on_host, name)[a:b])
        on_dev._ptr = at + n
        return n - len(games)

    t0 = time.perf_counter()
    sp.step(args.lead_in)
    torch.cuda.synchronize()
    log("lead-in of %d plies in %.2f s" % (args.lead_in, time.perf_counter() - t0))
    for warm in (route_export, route_host):                          # every shape and code object once
        sp.step(args.plies)
        warm()
        torch.cuda.synchronize()

    if args.trace_only:
        rows = calls = 0
        for _ in range(args.reps):
            sp.step(args.plies)
            at = on_dev._ptr
            route_export()
            rows += on_dev._ptr - at
            calls += 1
        torch.cuda.synchronize()
        print(json.dumps({"tool": "measure_export", "trace_only": True, "game": game, "export_calls_after_warm_up": calls,
                          "rows_after_warm_up": rows, "note": "the warm-up made one more k_sp_export call"}), flush=True)
        return

    res = {k: dict(rows_per_s=[], route_ms=[], rows=[], games=[], share_of_play_time=[], ply_ms=[]) for k in ("export", "host")}
    for rep in range(args.reps):
        for k, route in (("export", route_export), ("host", route_host)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sp.step(args.plies)
            torch.cuda.synchronize()
            play = time.perf_counter() - t0
            n_games = sp.finished()[0]
            at = on_dev._ptr
            t0 = time.perf_counter()
            route()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            rows = on_dev._ptr - at
            r = res[k]
            r["rows"].append(rows); r["games"].append(n_games); r["route_ms"].append(el * 1e3)
            r["rows_per_s"].append(rows / el); r["share_of_play_time"].append(el / play); r["ply_ms"].append(play * 1e3 / args.plies)
            log("rep %d %-6s: %d games, %d rows in %.2f ms = %.0f rows/s; %.4f of the %d plies' %.1f ms" %
                (rep, k, n_games, rows, el * 1e3, rows / el, el / play, args.plies, play * 1e3))
    rd, wr = bytes_per_row(game, args.td_steps)
    out = {"tool": "measure_export", "game": game, "games": args.games, "n_playout": args.n_playout, "vl_batch": 4,
           "evaluator": args.evaluator, "td_steps": args.td_steps, "capacity": args.capacity, "plies_per_repetition": args.plies,
           "repetitions": args.reps, "lead_in_plies": args.lead_in, "kernel_bytes_read_per_row": rd, "kernel_bytes_written_per_row": wr}
    for k, r in res.items():
        out[k] = {"rows_per_s": summary(r["rows_per_s"], 0), "route_ms": summary(r["route_ms"]),
                  "share_of_play_time": summary(r["share_of_play_time"], 5), "ply_ms": summary(r["ply_ms"]),
                  "rows": r["rows"], "games": r["games"]}
    e, h = out["export"]["rows_per_s"], out["host"]["rows_per_s"]
    out["export_over_host"] = round(e["median"] / h["median"], 2)
    out["ranges_overlap"] = not (e["min"] > h["max"] or h["min"] > e["max"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
