#!/usr/bin/env python3
"""The native learner (src/learner.py: az_learn_dev_epoch) against the Python route it restates - `adopt_all` +
`train_step(route="kernel")` + `ClipAdamW` - on the GPU, in ONE process, warm.  The protocol of tools/measure_heads.py: the
routes alternate, `--reps` (7) windows each, every window timed by a host clock from an idle device to a device
synchronise.

(a) a training window at dropout 0: one `train_step` call over a `ReplayBatches` of `--step-batches` (10) batches of
    `--step-rows` (1024) rows (after augmentation) drawn from a ring of synthetic Connect4 rows - the batches, the final
    no-grad forward and the one host read.  "native" is `NativeLearner.train_step`, "python" is `train_loss.train_step` on
    az_net.Connect4Net with all four pieces adopted and `net.opt` a `ClipAdamW`; both gather their batches with
    az_replay_dev_batch;
(b) the same with the reference's dropout attributes at 0.2 on both modules (blocks, attention, both heads);
(c) the dropout inputs alone, at N = 1024 and 8192: a window is `--iters` (50) times k_learn_keep (az_learn_dev_keep)
    against the torch draws it replaces - `draw_keep` for the three blocks and the two heads, `draw_keep_bits` for the
    attention block;
(d) the HOST time of enqueueing a window of (a)'s batches one by one, from an idle device to the return of the last call,
    the device not waited for: `NativeLearner.step` against zero_grad, forward, loss, backward and `clip_step` per batch.

One JSON line on stdout (kept under profiles/); progress on stderr.  The claim per row:
`native_median_below_python_median_by_more_than_python_spread`.

    python tools/measure_learner.py [--iters N] [--reps N] [--step-rows N] [--step-batches N]

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

from measure_loss import CONFIG_B, make_batch, summary      # noqa: E402

KEEP_SHAPES = (1024, 8192)
CLAIM = "native_median_below_python_median_by_more_than_python_spread"


def log(msg):
    sys.stderr.write("[learner] %s\n" % msg)
    sys.stderr.flush()


def compare(res, digits=3):
    n_ms, p_ms = res["native"]["ms"], res["python"]["ms"]
    res["python_over_native"] = round(p_ms["median"] / n_ms["median"], 2)
    res["python_spread_ms"] = round(p_ms["max"] - p_ms["min"], digits)
    res[CLAIM] = bool(p_ms["median"] - n_ms["median"] > p_ms["max"] - p_ms["min"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--step-rows", type=int, default=1024)
    ap.add_argument("--step-batches", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    assert args.reps >= 3, "at least three repetitions per route"
    assert args.iters > 0 and args.step_rows > 0 and args.step_rows % 2 == 0 and args.step_batches > 0

    import torch
    from src import az_net, learner as LN, optim as O, replay as RP, train_attn as TA, train_heads as TH, train_loss as TL
    assert torch.cuda.is_available(), "measure_learner needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    cfg = TL.LossConfig(**CONFIG_B)

    def timed(fn, wait=True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if wait:
            torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return ms

    def fresh_net(p):
        torch.manual_seed(7)
        net = az_net.Connect4Net(device=dev).train()
        with torch.no_grad():                   # the reference zeroes the heads' output weights: move them off zero
            for lin in (net.policy_head.out, net.dual_head.value_out, net.dual_head.aux_out):
                lin.weight.normal_(0, 0.05)
        if p > 0:
            layers = list(net.hidden.children())
            for block in layers[2:-1]:
                block.dropout = torch.nn.Dropout2d(p)
            layers[-1].attn.dropout_p = p
            net.policy_head.dropout = torch.nn.Dropout(p)
            net.dual_head.pool_drop = torch.nn.Dropout(p)
        net.opt = torch.optim.AdamW(O.reference_param_groups(net, 1e-4), lr=1e-4, weight_decay=1e-2)
        net.scheduler = torch.optim.lr_scheduler.LambdaLR(net.opt, lambda _: 1.0)
        return net

    # a ring of synthetic rows and one sample of it: --step-batches batches of --step-rows rows after augmentation
    cap = 8192
    rows, _ = make_batch(torch, "Connect4", cap, dev, 4321 + args.seed)
    ring = RP.ReplayTensors("Connect4", cap, device=dev)
    for name, t in zip(RP.ReplayTensors.TENSORS, rows):
        getattr(ring, name).copy_(t.to(getattr(ring, name).dtype).reshape(getattr(ring, name).shape))
    ring._ptr = cap
    gen = torch.Generator().manual_seed(99 + args.seed)
    per = args.step_rows // 2
    idx = torch.randint(0, cap, (per * args.step_batches,), generator=gen)
    batches = ring.batches(idx, per, order=torch.randperm(idx.numel(), generator=gen))
    assert len(batches) == args.step_batches

    out = {"tool": "measure_learner", "repetitions": args.reps, "rows": args.step_rows, "batches_per_window": args.step_batches,
           "module": "az_net.Connect4Net, the reference's parameter groups", "loss_config": "b", "claim": CLAIM}

    # ---- (a), (b): a train_step window; (d): the host side of its batches
    for key, p in (("train_step_dropout_0", 0.0), ("train_step_dropout_0.2", 0.2)):
        python_net = fresh_net(p)
        TH.adopt_all(python_net, route="kernel")
        O.adopt(python_net.opt)
        native_net = fresh_net(p)
        learner = LN.NativeLearner(native_net, args.step_rows, seed=args.seed)
        windows = {"native": lambda: learner.train_step(batches, n_epochs=1, **CONFIG_B),
                   "python": lambda: TL.train_step(python_net, batches, RP.augmented, n_epochs=1, route="kernel", **CONFIG_B)}
        for route in ("native", "python", "native", "python"):           # every code object once, the allocator warm
            timed(windows[route])
        ms = {r: [] for r in windows}
        for rep in range(args.reps):
            for route in ("native", "python"):
                ms[route].append(timed(windows[route]))
            log("%s rep %d: native %.3f ms, python %.3f ms" % (key, rep, ms["native"][-1], ms["python"][-1]))
        res = {r: {"ms": summary(v), "ms_per_batch": round(statistics.median(v) / args.step_batches, 3)} for r, v in ms.items()}
        res["window"] = "one train_step call: the batches, the final no-grad forward and the one host read"
        out[key] = compare(res)

        if p == 0.0:
            held = list(batches)

            def python_batches():
                for b in held:
                    python_net.opt.zero_grad(set_to_none=True)
                    log_p, value, steps = python_net(b[0], action_mask=b[6])
                    TL.training_loss(log_p, value, steps, b, python_net.aux_target_offset, cfg, "kernel").total.backward()
                    python_net.opt.clip_step(5)

            def native_batches():
                for b in held:
                    learner.step(b, cfg)
            python_net.train()
            host = {"native": native_batches, "python": python_batches}
            for route in ("native", "python"):
                timed(host[route])
            ms = {r: [] for r in host}
            for rep in range(args.reps):
                for route in ("native", "python"):
                    ms[route].append(timed(host[route], wait=False))
                log("host rep %d: native %.3f ms, python %.3f ms" % (rep, ms["native"][-1], ms["python"][-1]))
            res = {r: {"ms": summary(v), "us_per_batch": round(statistics.median(v) * 1e3 / len(held), 1)} for r, v in ms.items()}
            res["window"] = "host time of enqueueing the window's batches one by one; the device is not waited for"
            out["host_enqueue"] = compare(res)
        learner.close()

    # ---- (c) the dropout inputs alone
    out["keeps"] = []
    p = 0.2
    for n in KEEP_SHAPES:
        learner = LN.NativeLearner(fresh_net(p), n, seed=args.seed)

        def native_keeps():
            for i in range(args.iters):
                learner.draw_keeps(n, i)

        def torch_keeps():
            for _ in range(args.iters):
                for _ in range(3):
                    TH.draw_keep((n, 64), p, dev)
                TA.draw_keep_bits(n, p, dev)
                TH.draw_keep((n, 7, 64), p, dev)
                TH.draw_keep((n, 64), p, dev)
        fns = {"native": native_keeps, "python": torch_keeps}
        for route in ("native", "python", "native", "python"):
            timed(fns[route])
        ms = {r: [] for r in fns}
        for rep in range(args.reps):
            for route in ("native", "python"):
                ms[route].append(timed(fns[route]))
            log("keeps N=%d rep %d: native %.3f ms, torch %.3f ms" % (n, rep, ms["native"][-1], ms["python"][-1]))
        res = {"rows": n, "rate": p, "iterations_per_window": args.iters}
        for route, v in ms.items():
            res[route] = {"ms": summary(v), "us_per_batch": round(statistics.median(v) * 1e3 / args.iters, 2)}
        out["keeps"].append(compare(res))
        learner.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
