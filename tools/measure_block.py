#!/usr/bin/env python3
"""The residual block's training forward and backward on the GPU: the kernel route of `residual_block`
(src/train_block.py) against its plain-torch route, in ONE process, warm.  The protocol of tools/measure_loss.py:
the routes alternate, `--reps` (7) windows each, every window timed by a host clock from an idle device to a device
synchronise.

(a) the block alone: a window is `--iters` (50) times  y = residual_block(x, ...); y.backward(dy)  with gradients to
    all five tensors, seeded inputs (random normal x, Kaiming-scaled W, keep at p = 0.2), at N = 1024 and N = 8192;
(b) a training batch: a window is one `train_step` call of `--step-batches` (10) batches of `--step-rows` (1024) rows on
    az_net.Connect4Net, with `adopt_blocks` ("kernel") and without ("torch"); both use the kernel loss route;
(c) once, outside the windows: HIP-event time of the three UNADOPTED blocks' forward and backward inside a training
    batch of `--step-rows` rows (forward hooks and gradient hooks on the blocks record events), next to the event time
    of the whole forward + loss + backward: the share of a batch the blocks are today.  The backward interval of a
    block runs from the arrival of its output's gradient to the arrival of its input's gradient; torch accumulates the
    parameter gradients inside it.

One JSON line on stdout (kept under profiles/); progress on stderr.  The claim the line answers for (a) per shape and
for (b): `kernel_median_below_torch_median_by_more_than_torch_spread`.

    python tools/measure_block.py [--iters N] [--reps N] [--step-rows N] [--step-batches N]

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

from measure_loss import CONFIG_B, compare, make_batch, summary      # noqa: E402

SHAPES = (1024, 8192)
KEEP_P = 0.2


def log(msg):
    sys.stderr.write("[block] %s\n" % msg)
    sys.stderr.flush()


def block_inputs(torch, n, dev, seed):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    z = dict(device=dev, generator=gen)
    x = torch.randn((n, 64, 6, 7), **z)
    gamma = 1 + 0.3 * torch.randn((64,), **z)
    beta = 0.2 * torch.randn((64,), **z)
    W = torch.randn((64, 64, 3, 3), **z) * (2.0 / 576) ** 0.5
    b = 0.1 * torch.randn((64,), **z)
    keep = (torch.rand((n, 64), **z) >= KEEP_P).float() / (1 - KEEP_P)
    dy = torch.randn((n, 64, 6, 7), **z)
    return [t.requires_grad_(True) for t in (x, gamma, beta, W, b)], keep, dy


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
    from src import az_net, train_block as TB, train_loss as TL
    assert torch.cuda.is_available(), "measure_block needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {"tool": "measure_block", "iterations_per_window": args.iters, "repetitions": args.reps, "keep_p": KEEP_P, "shapes": []}

    # ---- (a) the block alone
    for n in SHAPES:
        tensors, keep, dy = block_inputs(torch, n, dev, 1234 + args.seed)

        def window(route):
            for _ in range(args.iters):
                for t in tensors:
                    t.grad = None
                TB.residual_block(*tensors, keep=keep, route=route).backward(dy)
        for route in ("kernel", "torch", "kernel", "torch"):             # every code object once, the allocator warm
            timed(lambda: window(route))
        ms = {"kernel": [], "torch": []}
        for rep in range(args.reps):
            for route in ("kernel", "torch"):
                ms[route].append(timed(lambda: window(route)))
            log("block N=%d rep %d: kernel %.3f ms, torch %.3f ms" % (n, rep, ms["kernel"][-1], ms["torch"][-1]))
        res = {"rows": n}
        for route, v in ms.items():
            res[route] = {"ms": summary(v), "us_per_forward_and_backward": round(statistics.median(v) * 1e3 / args.iters, 2)}
        out["shapes"].append(compare(res))
    out["all_shapes_kernel_median_below_torch_median_by_more_than_torch_spread"] = all(
        s["kernel_median_below_torch_median_by_more_than_torch_spread"] for s in out["shapes"])

    # ---- (b) one train_step call with and without adopt_blocks
    batch, _ = make_batch(torch, "Connect4", args.step_rows, dev, 4321 + args.seed)
    loader = [batch] * args.step_batches
    nets = {}
    for route in ("kernel", "torch"):
        torch.manual_seed(7)
        net = az_net.Connect4Net(device=dev)
        net.opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-2)
        net.scheduler = torch.optim.lr_scheduler.LambdaLR(net.opt, lambda _: 1.0)
        if route == "kernel":
            TB.adopt_blocks(net, route="kernel")
        nets[route] = net
        for _ in range(2):
            TL.train_step(net, loader, lambda b: b, n_epochs=1, route="kernel", **CONFIG_B)
        torch.cuda.synchronize()
    ms = {"kernel": [], "torch": []}
    for rep in range(args.reps):
        for route in ("kernel", "torch"):
            ms[route].append(timed(lambda: TL.train_step(nets[route], loader, lambda b: b, n_epochs=1, route="kernel", **CONFIG_B)))
        log("train_step rep %d: adopted %.3f ms, unadopted %.3f ms" % (rep, ms["kernel"][-1], ms["torch"][-1]))
    step = {"game": "Connect4", "rows": args.step_rows, "batches_per_window": args.step_batches, "module": "az_net.Connect4Net",
            "loss_route": "kernel", "kernel": None, "torch": None,
            "window": "one train_step call: the batches, the final no-grad forward and the one host read; "
                      "'kernel' is the module after adopt_blocks, 'torch' the module as it is"}
    for route, v in ms.items():
        step[route] = {"ms": summary(v), "ms_per_batch": round(statistics.median(v) / args.step_batches, 3)}
    out["train_step"] = compare(step)

    # ---- (c) the three unadopted blocks inside a training batch, by HIP events
    net = nets["torch"]
    blocks = [m for m in net.hidden.children() if TB._is_block(m)]
    cfg = TL.LossConfig(**CONFIG_B)
    marks = []

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def pre(mod, inputs):
        i = blocks.index(mod)
        marks.append(("fwd_begin", i, event()))
        if inputs[0].requires_grad:
            inputs[0].register_hook(lambda g, i=i: marks.append(("bwd_end", i, event())) and None)

    def post(mod, inputs, output):
        i = blocks.index(mod)
        marks.append(("fwd_end", i, event()))
        output.register_hook(lambda g, i=i: marks.append(("bwd_begin", i, event())) and None)
    handles = [h for m in blocks for h in (m.register_forward_pre_hook(pre), m.register_forward_hook(post))]
    shares = []
    net.train()
    for rep in range(5):
        del marks[:]
        net.opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        begin = event()
        heads = net(batch[0], batch[6])
        TL.training_loss(*heads, batch, net.aux_target_offset, cfg, route="kernel").total.backward()
        end = event()
        torch.cuda.synchronize()
        at = {(k, i): e for k, i, e in marks}
        fwd = sum(at["fwd_begin", i].elapsed_time(at["fwd_end", i]) for i in range(len(blocks)))
        bwd = sum(at["bwd_begin", i].elapsed_time(at["bwd_end", i]) for i in range(len(blocks)))
        shares.append((fwd, bwd, begin.elapsed_time(end)))
    for h in handles:
        h.remove()
    fwd, bwd, whole = (statistics.median(s[k] for s in shares[1:]) for k in range(3))
    out["blocks_in_a_batch"] = {"rows": args.step_rows, "blocks": len(blocks), "route": "torch (unadopted)", "samples": len(shares) - 1,
                                "forward_ms": round(fwd, 3), "backward_ms": round(bwd, 3),
                                "forward_loss_backward_ms": round(whole, 3), "share": round((fwd + bwd) / whole, 3),
                                "clock": "HIP events on the stream; the optimiser step is outside the interval"}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
