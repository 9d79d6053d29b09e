#!/usr/bin/env python3
"""Gradient clipping and the AdamW step on the GPU: `ClipAdamW` (src/optim.py, three launches) against what the
reference runs after `backward()`, in ONE process, warm.

Networks: az_net's reference-shaped Connect4 and Othello modules with the reference's parameter groups (five for
Connect4, six for Othello) and its schedulers.  Routes, alternating, `--reps` windows each:

    a   clip_grad_norm_(parameters, 5); torch.optim.AdamW(...).step()        the reference's configuration
    b   the same with AdamW(fused=True)
    c   adopt(net.opt).clip_step(5)                                          ClipAdamW, kernel route

Two kinds of window per network:

    clip_step   `--iters` (50) times clip + step on fixed seeded gradients (norm below 5, so that route a's in-place
                clipping leaves them as they are).  Per iteration: the host's time to enqueue (clock stopped before the
                synchronise), the span between two device events round the window, and the whole window up to the
                synchronise.  Where the host enqueues slower than the device works, the last two are the host's time too.
    batch       one `train_step` call of `--step-batches` (10) batches of `--step-rows` (1024) rows, kernel loss route,
                config (b) of the tests: forward, losses, backward, clip, step; the final no-grad forward and the one
                host read are part of the window.

One JSON line on stdout (kept under profiles/); progress on stderr.  The claim the line answers per network and kind of
window: `c_median_below_a_median_by_more_than_a_spread`; the same against b is reported beside it.

    python tools/measure_optim.py [--iters N] [--reps N] [--step-rows N] [--step-batches N]

There is no fall-back: without a GPU it fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
for p in (PKG, ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from measure_loss import CONFIG_B, make_batch, summary     # noqa: E402  (the same seeded batches as the loss measurement)

ROUTES = ("a", "b", "c")
WHAT = {"a": "clip_grad_norm_ + AdamW", "b": "clip_grad_norm_ + AdamW(fused=True)", "c": "ClipAdamW.clip_step"}


def log(msg):
    sys.stderr.write("[optim] %s\n" % msg)
    sys.stderr.flush()


def compare(res, key):
    """res[route][key] are summaries; c against a (the claim) and against b."""
    out = {}
    for other in ("a", "b"):
        c, o = res["c"][key], res[other][key]
        out["%s_over_c" % other] = round(o["median"] / c["median"], 2)
        out["%s_spread" % other] = round(o["max"] - o["min"], 3)
        out["c_median_below_%s_median_by_more_than_%s_spread" % (other, other)] = bool(o["median"] - c["median"] > o["max"] - o["min"])
    return out


def build(torch, az_net, optim, game, route, dev):
    from torch.optim.lr_scheduler import LinearLR, SequentialLR
    torch.manual_seed(7)
    net = (az_net.Connect4Net if game == "Connect4" else az_net.OthelloNet)(device=dev)
    net.opt = torch.optim.AdamW(optim.reference_param_groups(net, 1e-3), lr=1e-3, weight_decay=1e-2, **({"fused": True} if route == "b" else {}))
    warm = LinearLR(net.opt, start_factor=0.001, total_iters=100)
    train = LinearLR(net.opt, start_factor=1, end_factor=0.1, total_iters=1000)
    net.scheduler = SequentialLR(net.opt, schedulers=[warm, train], milestones=[100])
    if route == "c":
        optim.adopt(net.opt)
        assert net.opt.route == "kernel"
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-rows", type=int, default=1024)
    ap.add_argument("--step-batches", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert args.reps >= 3, "at least three repetitions per route"
    assert args.iters > 0 and args.step_rows > 0 and args.step_batches > 0

    import torch
    from src import az_net, optim, train_loss as TL
    assert torch.cuda.is_available(), "measure_optim needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def clip_and_step(net, route):
        if route == "c":
            return net.opt.clip_step(5)
        norm = torch.nn.utils.clip_grad_norm_(net.parameters(), 5)
        net.opt.step()
        return norm

    out = {"tool": "measure_optim", "routes": WHAT, "iterations_per_window": args.iters, "repetitions": args.reps,
           "step_rows": args.step_rows, "batches_per_window": args.step_batches, "config": CONFIG_B, "networks": []}
    for game in ("Connect4", "Othello"):
        nets = {r: build(torch, az_net, optim, game, r, dev) for r in ROUTES}
        params = list(nets["a"].parameters())
        res = {"game": game, "module": "az_net.%sNet" % game, "tensors": len(params), "elements": sum(p.numel() for p in params),
               "groups": len(nets["a"].opt.param_groups)}
        scale = 2.0 / (res["elements"] ** 0.5)                            # norm about 2
        gen = torch.Generator(device=dev)
        for r in ROUTES:
            gen.manual_seed(99 + args.seed)
            for p in nets[r].parameters():
                p.grad = torch.randn(p.shape, device=dev, generator=gen) * scale

        # ---- clip + step alone
        ms = {r: {"enqueue_us": [], "events_us": [], "window_us": []} for r in ROUTES}
        for r in ROUTES * 2:                                              # every code object once, the allocator warm
            for _ in range(args.iters):
                clip_and_step(nets[r], r)
            torch.cuda.synchronize()
        for rep in range(args.reps):
            for r in ROUTES:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                for _ in range(args.iters):
                    clip_and_step(nets[r], r)
                e1.record()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                ms[r]["enqueue_us"].append((t1 - t0) * 1e6 / args.iters)
                ms[r]["events_us"].append(e0.elapsed_time(e1) * 1e3 / args.iters)
                ms[r]["window_us"].append((t2 - t0) * 1e6 / args.iters)
            log("%s clip+step rep %d: %s" % (game, rep, "  ".join("%s %.1f us" % (r, ms[r]["window_us"][-1]) for r in ROUTES)))
        res["clip_step"] = {r: {k: summary(v, 1) for k, v in ms[r].items()} for r in ROUTES}
        res["clip_step"].update(compare(res["clip_step"], "window_us"))

        # ---- a whole train_step batch
        batch, _ = make_batch(torch, game, args.step_rows, dev, 4321 + args.seed)
        loader = [batch] * args.step_batches
        for r in ROUTES:
            nets[r] = build(torch, az_net, optim, game, r, dev)
            TL.train_step(nets[r], loader, lambda b: b, n_epochs=1, route="kernel", **CONFIG_B)
            torch.cuda.synchronize()
        ms = {r: [] for r in ROUTES}
        for rep in range(args.reps):
            for r in ROUTES:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                TL.train_step(nets[r], loader, lambda b: b, n_epochs=1, route="kernel", **CONFIG_B)
                torch.cuda.synchronize()
                ms[r].append((time.perf_counter() - t0) * 1e3 / args.step_batches)
            log("%s train_step rep %d: %s" % (game, rep, "  ".join("%s %.3f ms/batch" % (r, ms[r][-1]) for r in ROUTES)))
        res["batch"] = {r: {"ms_per_batch": summary(ms[r])} for r in ROUTES}
        res["batch"].update(compare(res["batch"], "ms_per_batch"))
        out["networks"].append(res)
        del nets
    out["all_c_median_below_a_median_by_more_than_a_spread"] = all(
        n[k]["c_median_below_a_median_by_more_than_a_spread"] for n in out["networks"] for k in ("clip_step", "batch"))
    out["all_c_median_below_b_median_by_more_than_b_spread"] = all(
        n[k]["c_median_below_b_median_by_more_than_b_spread"] for n in out["networks"] for k in ("clip_step", "batch"))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
