#!/usr/bin/env python3
"""Augmented training batches out of a replay ring on the GPU: the kernel route against the plain-torch route, in
ONE process, warm.

A ring of `--capacity` rows (default 500 000, the reference's buffer size) is filled by a seeded generator - stones,
turn signs, visit distributions, masks and targets with the value ranges self-play leaves; no self-play is needed
to measure a gather.  What one policy update reads is a sample of `--sample` ring rows (default 12 500 = 500 000 x
the reference's replay ratio 0.025) drawn on the device, then `--epochs` (2) passes over it in batches of `--batch`
samples under a fresh permutation each, every batch gathered, cast and symmetry-augmented; a repetition is
`--updates` (10) of those, so that a timed window is not a handful of launches:

  kernel   `ReplayBatches` with route="kernel": one az_replay_dev_batch (k_replay_batch) per batch
  torch    the same iteration with route="torch": indexing, cast, flips / transposes, concatenation

The two routes alternate, `--reps` times each, and each repetition is timed by a host clock from an idle device to a
device synchronise.  Every batch is dropped as soon as the next one is made, as a training loop does.

  ms                     one repetition: updates x (sample + epochs x batches)
  batches_per_s, rows_per_s   batches, and augmented rows (S x samples), per second of the route
  bytes_read_per_sample, bytes_written_per_sample   what k_replay_batch moves per sample, from the shapes (no counter)

One JSON line on stdout (kept under profiles/); progress on stderr.

    python tools/measure_batch.py [--othello] [--batch N] [--capacity N] [--sample N] [--epochs N] [--updates N] [--reps N]

`--trace-only` runs the kernel route `--reps` times and exits: the program to put behind `rocprofv3 --kernel-trace
--stats --` for the kernel's device time; it prints the calls and samples, and `--kernel-stats CSV --samples N
--calls N` turns that run's kernel_stats.csv into microseconds per call, bytes per second and the share of the HBM
rate `--hbm-bytes-per-s` (default 8e12, the MI355X's peak).  There is no fall-back: without a GPU it fails.
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

GEOMETRY = {"Connect4": (7, 42, 2), "Othello": (65, 64, 4)}             # actions, cells, symmetries


def log(msg):
    sys.stderr.write("[batch] %s\n" % msg)
    sys.stderr.flush()


def bytes_per_sample(game):
    """Bytes k_replay_batch reads from the ring (and the index arrays) and writes to the batch for one sample."""
    A, cells, S = GEOMETRY[game]
    small = 1 + 2 + 2 + 12 + 12                                          # winner, steps, aux, root_wdl, future_root_wdl
    read = 3 * cells + 4 * A + A + small + 8 + 8                         # + idx and order entries
    write = S * (4 * 3 * cells + 4 * A + A + small)
    return read, write


def kernel_stats(path, game, samples, calls, hbm):
    for rec in csv.DictReader(open(path)):
        if "k_replay_batch" in rec["Name"]:
            n_calls, total_ns = int(rec["Calls"]), float(rec["TotalDurationNs"])
            rd, wr = bytes_per_sample(game)
            # the trace holds the warm-up's calls too: scale the samples by the calls it counted
            moved = samples * (n_calls / calls) * (rd + wr) if calls else samples * (rd + wr)
            rate = moved / (total_ns * 1e-9)
            return {"tool": "measure_batch", "kernel": "k_replay_batch", "game": game, "calls": n_calls,
                    "total_us": round(total_ns / 1e3, 2), "avg_us": round(total_ns / 1e3 / n_calls, 2),
                    "min_us": round(float(rec["MinNs"]) / 1e3, 2), "max_us": round(float(rec["MaxNs"]) / 1e3, 2),
                    "bytes_read_per_sample": rd, "bytes_written_per_sample": wr, "bytes_per_s": round(rate),
                    "hbm_bytes_per_s": hbm, "share_of_hbm_rate": round(rate / hbm, 4),
                    "hbm_bound_us_per_call": round(moved / n_calls / hbm * 1e6, 3)}
    raise SystemExit("no k_replay_batch in %s" % path)


def summary(v, digits=3):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "all": [round(x, digits) for x in v]}


def fill_ring(torch, RP, game, capacity, dev, seed):
    """A full ring with the value ranges self-play leaves, from a seeded device generator."""
    A, cells, _S = GEOMETRY[game]
    buf = RP.SampledReplayTensors(game, capacity, dev)
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    z = dict(device=dev, generator=gen)
    cell = torch.randint(0, 3, tuple(buf.state.shape[:1]) + tuple(buf.state.shape[2:]), **z)    # empty / own / opponent
    buf.state[:, 0] = (cell == 1).to(torch.int8)
    buf.state[:, 1] = (cell == 2).to(torch.int8)
    buf.state[:, 2] = (torch.randint(0, 2, (capacity, 1, 1), **z) * 2 - 1).to(torch.int8)
    del cell
    p = torch.rand((capacity, A), **z)
    buf.valid_mask.copy_(torch.rand((capacity, A), **z) < 0.6)
    p = p * buf.valid_mask
    buf.prob.copy_(p / p.sum(1, keepdim=True).clamp_min(1e-9))
    del p
    buf.winner.copy_(torch.randint(-1, 2, (capacity, 1), **z))
    buf.steps_to_end.copy_(torch.randint(0, 61, (capacity, 1), **z))
    buf.aux_target.copy_(torch.randint(-64, 65, (capacity, 1), **z))
    for t in (buf.root_wdl, buf.future_root_wdl):
        w = torch.rand((capacity, 3), **z)
        t.copy_(w / w.sum(1, keepdim=True))
    buf._ptr = capacity
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--othello", action="store_true")
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--capacity", type=int, default=500000)
    ap.add_argument("--sample", type=int, default=12500)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--samples", type=int, default=0)
    ap.add_argument("--calls", type=int, default=0)
    ap.add_argument("--hbm-bytes-per-s", type=float, default=8.0e12)
    args = ap.parse_args()
    game = "Othello" if args.othello else "Connect4"
    if args.kernel_stats:
        print(json.dumps(kernel_stats(args.kernel_stats, game, args.samples, args.calls, args.hbm_bytes_per_s)), flush=True)
        return
    assert args.reps >= 3, "at least three repetitions per route"
    assert 0 < args.sample <= args.capacity and args.batch > 0 and args.epochs > 0 and args.updates > 0

    import torch
    from src import abi, replay as RP
    assert torch.cuda.is_available(), "measure_batch needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    t0 = time.perf_counter()
    buf = fill_ring(torch, RP, game, args.capacity, dev, 1234 + args.seed)
    torch.cuda.synchronize()
    log("%s ring of %d rows filled in %.2f s" % (game, args.capacity, time.perf_counter() - t0))
    # the sample size the learner would draw from this ring is the reference's rule; the tool pins it to --sample
    ratio = args.sample / args.capacity
    S = GEOMETRY[game][2]

    def repetition(route, call):
        """`--updates` policy updates' reads: per update a sample, then the epochs' batches.  Returns (batches, samples)."""
        n_batches = n_samples = 0
        for u in range(args.updates):
            key = call * args.updates + u
            idx = torch.empty(args.sample, dtype=torch.int64, device=dev)
            abi.check(abi.lib().az_replay_dev_sample_indices(args.seed, key, len(buf), idx.data_ptr(), args.sample, abi._stream()))
            loader = RP.ReplayBatches(buf, idx, args.batch, route=route, shuffle=True, seed=key)
            for _ in range(args.epochs):
                for batch in loader:
                    n_batches += 1
                    n_samples += batch[0].shape[0] // S
                    del batch
        return n_batches, n_samples

    for k, route in enumerate(("kernel", "torch", "kernel", "torch")):  # every shape and code object once, the allocator warm
        repetition(route, k)
        torch.cuda.synchronize()

    if args.trace_only:
        calls = samples = 0
        for rep in range(args.reps):
            b, s = repetition("kernel", 100 + rep)
            calls += b
            samples += s
        torch.cuda.synchronize()
        print(json.dumps({"tool": "measure_batch", "trace_only": True, "game": game, "batch": args.batch,
                          "kernel_calls_after_warm_up": calls, "samples_after_warm_up": samples,
                          "note": "the warm-up made two more repetitions of the kernel route"}), flush=True)
        return

    res = {k: dict(ms=[], batches=[], samples=[]) for k in ("kernel", "torch")}
    for rep in range(args.reps):
        for route in ("kernel", "torch"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            b, s = repetition(route, 100 + rep)                           # both routes read the same sample
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            res[route]["ms"].append(el * 1e3); res[route]["batches"].append(b); res[route]["samples"].append(s)
            log("rep %d %-6s: %d batches, %d samples in %.3f ms" % (rep, route, b, s, el * 1e3))
    rd, wr = bytes_per_sample(game)
    out = {"tool": "measure_batch", "game": game, "batch": args.batch, "capacity": args.capacity, "sample": args.sample,
           "replay_ratio": ratio, "epochs": args.epochs, "updates_per_repetition": args.updates, "repetitions": args.reps, "symmetries": S,
           "bytes_read_per_sample": rd, "bytes_written_per_sample": wr}
    for k, r in res.items():
        ms = r["ms"]
        out[k] = {"ms": summary(ms), "batches_per_repetition": r["batches"][0], "samples_per_repetition": r["samples"][0],
                  "batches_per_s": round(r["batches"][0] / (statistics.median(ms) * 1e-3)),
                  "rows_per_s": round(S * r["samples"][0] / (statistics.median(ms) * 1e-3))}
    k_ms, t_ms = out["kernel"]["ms"], out["torch"]["ms"]
    out["torch_over_kernel"] = round(t_ms["median"] / k_ms["median"], 2)
    out["torch_spread_ms"] = round(t_ms["max"] - t_ms["min"], 3)
    out["kernel_median_below_torch_median_by_more_than_torch_spread"] = bool(t_ms["median"] - k_ms["median"] > t_ms["max"] - t_ms["min"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
