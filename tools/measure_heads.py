#!/usr/bin/env python3
"""The Connect4 heads' training forward and backward on the GPU: the kernel route of `heads` (src/train_heads.py) against
the unadopted modules, in ONE process, warm.  The protocol of tools/measure_stem.py: the routes alternate, `--reps` (7)
windows each, every window timed by a host clock from an idle device to a device synchronise.

(a) the heads alone: a window is `--iters` (50) times  out = heads(tokens, legal); backward(out, upstream)  with gradients
    to the tokens and the eighteen parameters, seeded tokens, a Bernoulli(0.7) mask, at N = 1024 and N = 8192.  "torch" is
    az_net.Connect4Net's own `policy_head` and `dual_head`; "kernel" is `heads(route="kernel")` on the same parameters;
(b) a training batch: a window is one `train_step` call of `--step-batches` (10) batches of `--step-rows` (1024) rows on
    az_net.Connect4Net with `adopt_blocks`, `adopt_attention` and `adopt_stem`, against the same plus `adopt_heads`; both
    use the kernel loss route;
(c) once, outside the windows: HIP-event time of the UNADOPTED heads' forward and backward inside a training batch of
    `--step-rows` rows of the stem-blocks-and-attention module - from the tokens `hidden` returns to the three outputs,
    and from the first output gradient the loss hands back to the last of the tokens' gradient and the eighteen parameter
    gradients - next to the event time of the whole forward + loss + backward: the share of a batch the heads are today.

One JSON line on stdout (kept under profiles/); progress on stderr.  The claim the line answers per row of (a) and for
(b): `kernel_median_below_torch_median_by_more_than_torch_spread`.

    python tools/measure_heads.py [--iters N] [--reps N] [--step-rows N] [--step-batches N]

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


def log(msg):
    sys.stderr.write("[heads] %s\n" % msg)
    sys.stderr.flush()


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
    from src import az_net, train_attn as TA, train_block as TB, train_heads as TH, train_loss as TL, train_stem as TS
    assert torch.cuda.is_available(), "measure_heads needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def fresh_net():
        torch.manual_seed(7)
        net = az_net.Connect4Net(device=dev).train()
        with torch.no_grad():                   # the reference zeroes the heads' output weights: move them off zero
            for lin in (net.policy_head.out, net.dual_head.value_out, net.dual_head.aux_out):
                lin.weight.normal_(0, 0.05)
        return net

    out = {"tool": "measure_heads", "iterations_per_window": args.iters, "repetitions": args.reps, "shapes": []}

    # ---- (a) the heads alone
    net = fresh_net()
    params = [TH._resolve(net, path) for _, path, _ in TH.PARAMS]

    def torch_heads(tokens, legal):
        return (net.policy_head(tokens, legal),) + tuple(net.dual_head(tokens))

    def kernel_heads(tokens, legal):
        return TH.heads(tokens, legal, *params, eps=net.policy_head.norm.eps, route="kernel")
    fns = {"kernel": kernel_heads, "torch": torch_heads}
    for n in SHAPES:
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234 + args.seed)
        tokens = (1.5 * torch.randn((n, 42, 64), device=dev, generator=gen)).requires_grad_(True)
        legal = torch.rand((n, 7), device=dev, generator=gen) < 0.7
        legal[:, 3] = True                      # no entirely illegal row
        ups = [torch.randn(shape, device=dev, generator=gen) for shape in ((n, 7), (n, 3), (n,))]
        ups[0] = ups[0] * legal                 # as the loss hands it back: nothing on illegal moves

        def window(route):
            for _ in range(args.iters):
                tokens.grad = None
                for t in params:
                    t.grad = None
                torch.autograd.backward(list(fns[route](tokens, legal)), ups)
        for route in ("kernel", "torch", "kernel", "torch"):             # every code object once, the allocator warm
            timed(lambda: window(route))
        ms = {"kernel": [], "torch": []}
        for rep in range(args.reps):
            for route in ("kernel", "torch"):
                ms[route].append(timed(lambda: window(route)))
            log("heads N=%d rep %d: kernel %.3f ms, torch %.3f ms" % (n, rep, ms["kernel"][-1], ms["torch"][-1]))
        res = {"rows": n}
        for route, v in ms.items():
            res[route] = {"ms": summary(v), "us_per_forward_and_backward": round(statistics.median(v) * 1e3 / args.iters, 2)}
        out["shapes"].append(compare(res))
    out["all_shapes_kernel_median_below_torch_median_by_more_than_torch_spread"] = all(
        s["kernel_median_below_torch_median_by_more_than_torch_spread"] for s in out["shapes"])

    # ---- (b) one train_step call: stem, blocks and attention adopted, and the heads too
    batch, _ = make_batch(torch, "Connect4", args.step_rows, dev, 4321 + args.seed)
    loader = [batch] * args.step_batches
    routes = ("stem_blocks_and_attention", "all_four")
    nets = {}
    for route in routes:
        net = fresh_net()
        net.opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-2)
        net.scheduler = torch.optim.lr_scheduler.LambdaLR(net.opt, lambda _: 1.0)
        TB.adopt_blocks(net, route="kernel")
        TA.adopt_attention(net, route="kernel")
        TS.adopt_stem(net, route="kernel")
        if route == "all_four":
            TH.adopt_heads(net, route="kernel")
        nets[route] = net
        for _ in range(2):
            TL.train_step(net, loader, lambda b: b, n_epochs=1, route="kernel", **CONFIG_B)
        torch.cuda.synchronize()
    ms = {r: [] for r in routes}
    for rep in range(args.reps):
        for route in routes:
            ms[route].append(timed(lambda: TL.train_step(nets[route], loader, lambda b: b, n_epochs=1, route="kernel", **CONFIG_B)))
        log("train_step rep %d: " % rep + ", ".join("%s %.3f ms" % (r, ms[r][-1]) for r in routes))
    per = {r: {"ms": summary(v), "ms_per_batch": round(statistics.median(v) / args.step_batches, 3)} for r, v in ms.items()}
    out["train_step"] = {"game": "Connect4", "rows": args.step_rows, "batches_per_window": args.step_batches,
                         "module": "az_net.Connect4Net", "loss_route": "kernel", "routes": per,
                         "window": "one train_step call: the batches, the final no-grad forward and the one host read",
                         "against_stem_blocks_and_attention": compare({"kernel": dict(per["all_four"]),
                                                                       "torch": dict(per["stem_blocks_and_attention"])})}

    # ---- (c) the unadopted heads inside a training batch of the stem-blocks-and-attention module, by HIP events
    net = nets["stem_blocks_and_attention"]
    cfg = TL.LossConfig(**CONFIG_B)
    marks = {}

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def ends(_):
        marks.setdefault("bwd_ends", []).append(event())

    def begins(_):
        if "bwd_begin" not in marks:
            marks["bwd_begin"] = event()

    def post(mod, inputs, output):
        marks["fwd_begin"] = event()
        output.register_hook(ends)
    handles = [net.hidden.register_forward_hook(post)]
    for w in list(net.policy_head.parameters()) + list(net.dual_head.parameters()):
        handles.append(w.register_hook(ends))
    shares = []
    net.train()
    for rep in range(5):
        marks.clear()
        net.opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        begin = event()
        heads = net(batch[0], batch[6])
        marks["fwd_end"] = event()
        for o in heads:
            o.register_hook(begins)
        TL.training_loss(*heads, batch, net.aux_target_offset, cfg, route="kernel").total.backward()
        end = event()
        torch.cuda.synchronize()
        assert len(marks["bwd_ends"]) >= 19, "the tokens and every parameter of the heads got a gradient"
        shares.append((marks["fwd_begin"].elapsed_time(marks["fwd_end"]),
                       max(marks["bwd_begin"].elapsed_time(e) for e in marks["bwd_ends"]), begin.elapsed_time(end)))
    for h in handles:
        h.remove()
    fwd, bwd, whole = (statistics.median(s[k] for s in shares[1:]) for k in range(3))
    out["heads_in_a_batch"] = {"rows": args.step_rows, "route": "torch (heads unadopted; stem, blocks and attention adopted)",
                               "samples": len(shares) - 1, "forward_ms": round(fwd, 3), "backward_ms": round(bwd, 3),
                               "forward_loss_backward_ms": round(whole, 3), "share": round((fwd + bwd) / whole, 3),
                               "interval": "from the tokens to the three outputs; backward from the first output gradient to the last of "
                                           "the tokens' gradient and the eighteen parameter gradients",
                               "clock": "HIP events on the stream; the optimiser step is outside the interval"}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
