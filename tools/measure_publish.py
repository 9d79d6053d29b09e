#!/usr/bin/env python3
"""Trained weights into a live evaluator: `publish` (src/publish.py: az_learn_publish / az_nn_model_publish, ONE launch into
the twin's existing buffers) against the only route there was before it, `FastConnect4Net.from_module(net)` +
`native_model()` on the same module (a new twin: about a hundred torch operations, new buffers, four device reads, a new
az_nn_model) - on the GPU, in ONE process, warm.  The protocol of tools/measure_learner.py: the routes alternate, `--reps`
(9) windows each after two warm-up rounds, every window starts from an idle device.

Per window three figures, reported separately:
    host_ms     host clock from the call to its return (both routes wait for the device inside: publish once, for the
                three head biases; the rebuild four times, in `.item()`)
    total_ms    host clock from the call to an idle device (a device synchronise after the return)
    device_ms   between two events on the stream, recorded right before and right after the call: what the device spends
                from its first operation to its last, gaps between the rebuild's small kernels included

Routes: "publish_learner" (`NativeLearner.publish`, az_learn_publish), "publish_module" (`FastConnect4Net.publish_from` of
the module: the Python walk over the state dict, then az_nn_model_publish), "rebuild" (from_module + native_model; the old
twin is dropped outside the window).  The module's parameters change between windows (one optimiser-sized in-place
update), as they would after a training step.

One JSON line on stdout (kept under profiles/); progress on stderr.  The claim per publish route:
`publish_median_below_rebuild_median_by_more_than_rebuild_spread`, for host_ms and for device_ms.  No threshold gates
anything: the figures say what they say.

    python tools/measure_publish.py [--reps N] [--game connect4|othello]

`--game othello`: `FusedSearch.publish_weights()` ("publish_weights": the preconditions, az_nn_model_publish_othello, the
version tuple) and `FastOthelloNet.publish_from()` ("publish_twin") against "rebuild" (`FastOthelloNet(net)` +
`native_model()`: eleven weight packings, a dozen BatchNorm folds, two 512 x 512 transposes, three device reads, a new
az_nn_model), at 1 and 3 residual blocks, in this one process; between windows the parameters AND the BatchNorms' running
statistics move.  One JSON line with an entry per depth.

There is no fall-back: without a GPU it fails.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
for p in (PKG, ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from measure_loss import summary      # noqa: E402

CLAIM = "publish_median_below_rebuild_median_by_more_than_rebuild_spread"


def log(msg):
    sys.stderr.write("[publish] %s\n" % msg)
    sys.stderr.flush()


def windows(torch, routes, reps, move, tag):
    """Two warm-up rounds, then `reps` windows per route, the routes alternating -> {route: {figure: [ms]}}"""
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def window(fn):
        move()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        start.record()
        fn()
        stop.record()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t0) * 1e3, start.elapsed_time(stop)

    for _ in range(2):                      # every code object once, the allocator warm
        for name in routes:
            window(routes[name])
    ms = {name: {"host_ms": [], "total_ms": [], "device_ms": []} for name in routes}
    for rep in range(reps):
        for name in routes:
            host, total, device = window(routes[name])
            for key, v in (("host_ms", host), ("total_ms", total), ("device_ms", device)):
                ms[name][key].append(v)
        log("%s rep %d: " % (tag, rep) + ", ".join("%s host %.3f device %.3f" % (n, ms[n]["host_ms"][-1], ms[n]["device_ms"][-1]) for n in routes))
    return ms


def main_othello(args):
    import torch
    from src import MCTS_cpp, az_net
    from src.fast_othello import FastOthelloNet
    assert torch.cuda.is_available(), "measure_publish needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    out = {"tool": "measure_publish", "game": "othello", "repetitions": args.reps, "claim": CLAIM,
           "window": "parameters and running statistics change, the device idles, then one call; host_ms to the call's return, "
                     "total_ms to an idle device, device_ms between events around the call"}
    for n_blocks in (1, 3):
        torch.manual_seed(7)
        net = az_net.OthelloNet(num_res_blocks=n_blocks, device=dev)
        with torch.no_grad():               # trained-looking BatchNorm statistics, the zeroed output layers off zero
            for m in net.modules():
                if isinstance(m, torch.nn.BatchNorm2d):
                    m.running_mean.normal_(0.0, 0.2); m.running_var.uniform_(0.5, 1.5)
                    m.weight.uniform_(0.7, 1.3); m.bias.normal_(0.0, 0.1)
            for m in (net.policy_head.board_out, net.policy_head.pass_fc, net.dual_head.value_out[-1], net.dual_head.aux_out[-1]):
                m.weight.normal_(0.0, 0.05); m.bias.normal_(0.0, 0.05)
        wrapper = MCTS_cpp.BatchedMCTS(8, 1.4, 800, 0.0, 16, noise_epsilon=0.0, use_symmetry=False, game_name="Othello",
                                       score_utility_factor=0.15, score_scale=8.0)
        fs = wrapper._fused_runner(net, True)
        assert fs.publish_weights() == "rebuilt" and isinstance(fs.fast, FastOthelloNet) and fs.fast.native_model() is not None
        assert fs.publish_weights() == "published"
        kept = {}

        def rebuild():
            kept["fast"] = FastOthelloNet(net)
            kept["model"] = kept["fast"].native_model()

        def move():
            with torch.no_grad():           # the weights and the running statistics move, as after a training step
                for p in net.parameters():
                    p.mul_(1.0 - 1e-6)
                for m in net.modules():
                    if isinstance(m, torch.nn.BatchNorm2d):
                        m.running_var.mul_(1.0 + 1e-6)
            kept.clear()

        routes = {"publish_weights": fs.publish_weights, "publish_twin": fs.fast.publish_from, "rebuild": rebuild}
        ms = windows(torch, routes, args.reps, move, "%d blocks" % n_blocks)
        entry = {name: {key: summary(v) for key, v in ms[name].items()} for name in routes}
        for name in ("publish_weights", "publish_twin"):
            for key in ("host_ms", "device_ms"):
                r, p = entry["rebuild"][key], entry[name][key]
                entry[name]["rebuild_over_publish_" + key] = round(r["median"] / p["median"], 2)
                entry[name][CLAIM + "_" + key] = bool(r["median"] - p["median"] > r["max"] - r["min"])
        out["blocks_%d" % n_blocks] = entry
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--game", choices=("connect4", "othello"), default="connect4")
    args = ap.parse_args()
    assert args.reps >= 3, "at least three repetitions per route"
    if args.game == "othello":
        return main_othello(args)

    import torch
    from src import az_net, learner as LN, optim as O
    from src.fast_net import FastConnect4Net
    assert torch.cuda.is_available(), "measure_publish needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    torch.manual_seed(7)
    net = az_net.Connect4Net(device=dev).train()
    with torch.no_grad():                   # the reference zeroes the heads' output weights: move them off zero
        for lin in (net.policy_head.out, net.dual_head.value_out, net.dual_head.aux_out):
            lin.weight.normal_(0, 0.05)
    net.opt = torch.optim.AdamW(O.reference_param_groups(net, 1e-4), lr=1e-4, weight_decay=1e-2)
    net.scheduler = torch.optim.lr_scheduler.LambdaLR(net.opt, lambda _: 1.0)
    learner = LN.NativeLearner(net, 64)
    fast = FastConnect4Net.from_module(net)
    assert fast.native_model() is not None
    kept = {}

    def rebuild():
        kept["fast"] = FastConnect4Net.from_module(net)
        kept["model"] = kept["fast"].native_model()

    routes = {"publish_learner": lambda: learner.publish(fast), "publish_module": lambda: fast.publish_from(net), "rebuild": rebuild}

    def move():
        with torch.no_grad():               # the weights move, as after a training step
            for p in net.parameters():
                p.mul_(1.0 - 1e-6)
        kept.clear()

    ms = windows(torch, routes, args.reps, move, "connect4")
    out = {"tool": "measure_publish", "repetitions": args.reps, "module": "az_net.Connect4Net, 3 blocks", "claim": CLAIM,
           "window": "the weights change, the device idles, then one call; host_ms to the call's return, total_ms to an idle device, "
                     "device_ms between events around the call"}
    for name in routes:
        out[name] = {key: summary(v) for key, v in ms[name].items()}
    for name in ("publish_learner", "publish_module"):
        for key in ("host_ms", "device_ms"):
            r, p = out["rebuild"][key], out[name][key]
            out[name]["rebuild_over_publish_" + key] = round(r["median"] / p["median"], 2)
            out[name][CLAIM + "_" + key] = bool(r["median"] - p["median"] > r["max"] - r["min"])
    learner.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
