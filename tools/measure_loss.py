#!/usr/bin/env python3
"""The training losses and their gradients on the GPU: the kernel route of `training_loss` (src/train_loss.py)
against its plain-torch route, in ONE process, warm.

A batch of N augmented rows is made by a seeded generator with the value ranges self-play leaves (stones, turn
signs, visit distributions with end-state rows, masks, targets), the three head outputs likewise (logits masked at
-1e9 before the log-softmax).  A timed window is `--iters` (50) times

    training_loss(...)  ->  (policy + value + aux).backward()      # gradients arrive at the three head outputs

under config (b) of the tests (value_decay 0.98, distillation 0.3 at temperature 2, psw_beta 0.3, entropy 0.01,
td 0.25 over 5 steps: every term on), so that a window is not a handful of launches.  The two routes alternate,
`--reps` times each, and each window is timed by a host clock from an idle device to a device synchronise.
Shapes: Connect4 at N = 1024 and 8192, Othello at N = 2048.

It also times one full `train_step` batch - forward of az_net's reference-shaped Connect4 module, the losses,
backward, clipping, AdamW - on each route at `--step-rows` (1024) rows, so that the share of a training batch the
losses take is on record.

One JSON line on stdout (kept under profiles/); progress on stderr.  The claim the line answers per shape:
`kernel_median_below_torch_median_by_more_than_torch_spread`, and `all_shapes` for all of them together.

    python tools/measure_loss.py [--iters N] [--reps N] [--step-rows N] [--step-batches N]

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
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

GEOMETRY = {"Connect4": (7, 6, 7, 42.0), "Othello": (65, 8, 8, 64.0)}     # actions, rows, columns, aux offset
CONFIG_B = dict(value_decay=0.98, distill_alpha=0.3, distill_temp=2.0, psw_beta=0.3, entropy_lambda=0.01, td_alpha=0.25, td_steps=5)
SHAPES = (("Connect4", 1024), ("Connect4", 8192), ("Othello", 2048))


def log(msg):
    sys.stderr.write("[loss] %s\n" % msg)
    sys.stderr.flush()


def summary(v, digits=3):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits),
            "all": [round(x, digits) for x in v]}


def compare(res):
    k_ms, t_ms = res["kernel"]["ms"], res["torch"]["ms"]
    res["torch_over_kernel"] = round(t_ms["median"] / k_ms["median"], 2)
    res["torch_spread_ms"] = round(t_ms["max"] - t_ms["min"], 3)
    res["kernel_median_below_torch_median_by_more_than_torch_spread"] = bool(
        t_ms["median"] - k_ms["median"] > t_ms["max"] - t_ms["min"])
    return res


def make_batch(torch, game, n, dev, seed):
    """A batch as `ReplayBatches` yields it, and head outputs for it, from a seeded device generator."""
    A, R, Cc, _ = GEOMETRY[game]
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    z = dict(device=dev, generator=gen)
    cell = torch.randint(0, 3, (n, R, Cc), **z)
    turn = (torch.randint(0, 2, (n, 1, 1), **z) * 2 - 1).float().expand(n, R, Cc)
    state = torch.stack([(cell == 1).float(), (cell == 2).float(), turn], 1).contiguous()
    end = torch.rand((n, 1), **z) < 0.04                                  # end states: no policy target, mask all ones
    mask = (torch.rand((n, A), **z) < 0.6) | end
    mask[:, 0] |= ~mask.any(1)
    p = torch.rand((n, A), **z) * mask * ~end
    prob = p / p.sum(1, keepdim=True).clamp_min(1e-9)
    winner = torch.randint(-1, 2, (n, 1), **z).to(torch.int8)
    steps_to_end = torch.where(end, 0, torch.randint(1, 43, (n, 1), **z)).to(torch.int16)
    aux_target = torch.randint(-42, 43, (n, 1), **z).to(torch.int16)
    wdl = []
    for keep in (~end, (steps_to_end > 5) & ~end):
        w = torch.rand((n, 3), **z)
        wdl.append((w / w.sum(1, keepdim=True) * keep).contiguous())
    batch = (state, prob.contiguous(), winner, steps_to_end, aux_target, wdl[0], mask.contiguous(), wdl[1])
    logits = (torch.randn((n, A), **z) * 1.5).masked_fill(~mask, -1e9)
    heads = (torch.log_softmax(logits, 1), torch.log_softmax(torch.randn((n, 3), **z), 1), torch.rand((n,), **z))
    return batch, heads


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
    from src import az_net, train_loss as TL
    assert torch.cuda.is_available(), "measure_loss needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = TL.LossConfig(**CONFIG_B)

    def window(route, batch, heads, offset):
        for _ in range(args.iters):
            for h in heads:
                h.grad = None
            TL.training_loss(*heads, batch, offset, cfg, route=route).total.backward()

    out = {"tool": "measure_loss", "config": CONFIG_B, "iterations_per_window": args.iters, "repetitions": args.reps, "shapes": []}
    for game, n in SHAPES:
        batch, heads = make_batch(torch, game, n, dev, 1234 + args.seed)
        heads = [h.detach().requires_grad_(True) for h in heads]
        offset = GEOMETRY[game][3]
        for route in ("kernel", "torch", "kernel", "torch"):             # every code object once, the allocator warm
            window(route, batch, heads, offset)
            torch.cuda.synchronize()
        ms = {"kernel": [], "torch": []}
        for rep in range(args.reps):
            for route in ("kernel", "torch"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                window(route, batch, heads, offset)
                torch.cuda.synchronize()
                ms[route].append((time.perf_counter() - t0) * 1e3)
            log("%s N=%d rep %d: kernel %.3f ms, torch %.3f ms" % (game, n, rep, ms["kernel"][-1], ms["torch"][-1]))
        res = {"game": game, "rows": n}
        for route, v in ms.items():
            res[route] = {"ms": summary(v), "us_per_loss_and_backward": round(statistics.median(v) * 1e3 / args.iters, 2)}
        out["shapes"].append(compare(res))
    out["all_shapes_kernel_median_below_torch_median_by_more_than_torch_spread"] = all(
        s["kernel_median_below_torch_median_by_more_than_torch_spread"] for s in out["shapes"])

    # one full train_step batch on each route: the reference-shaped Connect4 module, AdamW, clipping
    batch, _ = make_batch(torch, "Connect4", args.step_rows, dev, 4321 + args.seed)
    loader = [batch] * args.step_batches
    nets = {}
    for route in ("kernel", "torch"):
        torch.manual_seed(7)
        net = az_net.Connect4Net(device=dev)
        net.opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-2)
        net.scheduler = torch.optim.lr_scheduler.LambdaLR(net.opt, lambda _: 1.0)
        nets[route] = net
        TL.train_step(net, loader, lambda b: b, n_epochs=1, route=route, **CONFIG_B)
        torch.cuda.synchronize()
    ms = {"kernel": [], "torch": []}
    for rep in range(args.reps):
        for route in ("kernel", "torch"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            TL.train_step(nets[route], loader, lambda b: b, n_epochs=1, route=route, **CONFIG_B)
            torch.cuda.synchronize()
            ms[route].append((time.perf_counter() - t0) * 1e3)
        log("train_step rep %d: kernel %.3f ms, torch %.3f ms" % (rep, ms["kernel"][-1], ms["torch"][-1]))
    step = {"game": "Connect4", "rows": args.step_rows, "batches_per_window": args.step_batches, "module": "az_net.Connect4Net",
            "window": "one train_step call: the batches, the final no-grad forward and the one host read"}
    for route, v in ms.items():
        step[route] = {"ms": summary(v), "ms_per_batch": round(statistics.median(v) / args.step_batches, 3)}
    compare(step)
    same = next(s for s in out["shapes"] if s["game"] == "Connect4" and s["rows"] == 1024)
    if args.step_rows == 1024:
        for route in ("kernel", "torch"):
            step[route]["loss_share_of_batch"] = round(same[route]["us_per_loss_and_backward"] * 1e-3 / step[route]["ms_per_batch"], 3)
    out["train_step"] = step
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
