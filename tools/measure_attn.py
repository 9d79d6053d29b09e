#!/usr/bin/env python3
"""The gated attention block's training forward and backward on the GPU: the kernel route of `gated_attention`
(src/train_attn.py, through `adopt_attention`) against the unadopted module, in ONE process, warm.  The protocol of
tools/measure_block.py: the routes alternate, `--reps` (7) windows each, every window timed by a host clock from an idle
device to a device synchronise.

(a) the block alone: a window is `--iters` (50) times  y = block(x); y.backward(dy)  with gradients to x and the six
    parameters, seeded inputs, at N = 1024 and N = 8192, at dropout p = 0 and p = 0.2.  "torch" is az_net's attention
    block itself in training mode, its `scaled_dot_product_attention` call given `dropout_p` (the one argument the
    reference passes and the inference-side module leaves out); "kernel" is a twin with the same parameters after
    `adopt_attention`, which draws its mask words with torch ops inside the window;
(b) a training batch: a window is one `train_step` call of `--step-batches` (10) batches of `--step-rows` (1024) rows on
    az_net.Connect4Net: unadopted, with `adopt_blocks`, with `adopt_blocks` and `adopt_attention`; all use the kernel
    loss route.  Two comparisons: both adopted against unadopted, and both adopted against blocks only;
(c) once, outside the windows: HIP-event time of the UNADOPTED attention block's forward and backward inside a training
    batch of `--step-rows` rows (hooks record events), next to the event time of the whole forward + loss + backward:
    the share of a batch the block is today.

One JSON line on stdout (kept under profiles/); progress on stderr.  The claim the line answers per row of (a) and per
comparison of (b): `kernel_median_below_torch_median_by_more_than_torch_spread`.

    python tools/measure_attn.py [--iters N] [--reps N] [--step-rows N] [--step-batches N]

There is no fall-back: without a GPU it fails.
"""
import argparse
import json
import os
import statistics
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
for p in (PKG, ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from measure_loss import CONFIG_B, compare, make_batch, summary      # noqa: E402

SHAPES = (1024, 8192)
DROPOUT = (0.0, 0.2)


def log(msg):
    sys.stderr.write("[attn] %s\n" % msg)
    sys.stderr.flush()


def with_sdpa_dropout(torch, attn):
    """az_net._GatedAttention.forward with `dropout_p` handed to scaled_dot_product_attention in training mode, as the
    reference's module does; everything else is the module's own code path, op for op."""
    F = torch.nn.functional

    def forward(self, x):
        b, t, dim = x.shape
        h = self.prenorm(x)
        q, k, v = self.qkv_proj(h).view(b, t, 3, self.heads, self.hd).unbind(2)
        gate = self.gate_proj(h)
        q = self.q_norm(q).transpose(1, 2)
        k = self.k_norm(k).transpose(1, 2)
        a = F.scaled_dot_product_attention(q, k, v.transpose(1, 2), dropout_p=self.dropout_p if self.training else 0.0)
        a = a * gate.transpose(1, 2).unsqueeze(-1).sigmoid()
        return self.o_proj(a.transpose(1, 2).reshape(b, t, dim)) + x
    attn.forward = types.MethodType(forward, attn)


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
    from src import az_net, train_attn as TA, train_block as TB, train_loss as TL
    assert torch.cuda.is_available(), "measure_attn needs a GPU"
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    out = {"tool": "measure_attn", "iterations_per_window": args.iters, "repetitions": args.reps, "shapes": []}

    # ---- (a) the block alone
    blocks = {}
    for route in ("kernel", "torch"):
        torch.manual_seed(7)
        net = az_net.Connect4Net(device=dev).train()
        with torch.no_grad():
            for w in (net.hidden[-1].attn.prenorm.weight, net.hidden[-1].attn.q_norm.weight, net.hidden[-1].attn.k_norm.weight):
                w.add_(0.3 * torch.randn_like(w))
        if route == "kernel":
            TA.adopt_attention(net, route="kernel")
        else:
            with_sdpa_dropout(torch, net.hidden[-1].attn)
        blocks[route] = net.hidden[-1]
    for n in SHAPES:
        gen = torch.Generator(device=dev)
        gen.manual_seed(1234 + args.seed)
        x = torch.randn((n, 64, 6, 7), device=dev, generator=gen).requires_grad_(True)
        dy = torch.randn((n, 42, 64), device=dev, generator=gen)
        for p in DROPOUT:
            for b in blocks.values():
                b.attn.dropout_p = p

            def window(route):
                block = blocks[route]
                for _ in range(args.iters):
                    x.grad = None
                    for t in block.parameters():
                        t.grad = None
                    block(x).backward(dy)
            for route in ("kernel", "torch", "kernel", "torch"):             # every code object once, the allocator warm
                timed(lambda: window(route))
            ms = {"kernel": [], "torch": []}
            for rep in range(args.reps):
                for route in ("kernel", "torch"):
                    ms[route].append(timed(lambda: window(route)))
                log("block N=%d p=%.1f rep %d: kernel %.3f ms, torch %.3f ms" % (n, p, rep, ms["kernel"][-1], ms["torch"][-1]))
            res = {"rows": n, "dropout_p": p}
            for route, v in ms.items():
                res[route] = {"ms": summary(v), "us_per_forward_and_backward": round(statistics.median(v) * 1e3 / args.iters, 2)}
            out["shapes"].append(compare(res))
    out["all_shapes_kernel_median_below_torch_median_by_more_than_torch_spread"] = all(
        s["kernel_median_below_torch_median_by_more_than_torch_spread"] for s in out["shapes"])

    # ---- (b) one train_step call: unadopted, blocks adopted, blocks and attention adopted
    batch, _ = make_batch(torch, "Connect4", args.step_rows, dev, 4321 + args.seed)
    loader = [batch] * args.step_batches
    routes = ("unadopted", "blocks", "blocks_and_attention")
    nets = {}
    for route in routes:
        torch.manual_seed(7)
        net = az_net.Connect4Net(device=dev)
        net.opt = torch.optim.AdamW(net.parameters(), lr=1e-4, weight_decay=1e-2)
        net.scheduler = torch.optim.lr_scheduler.LambdaLR(net.opt, lambda _: 1.0)
        if route != "unadopted":
            TB.adopt_blocks(net, route="kernel")
        if route == "blocks_and_attention":
            TA.adopt_attention(net, route="kernel")
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
                         "against_unadopted": compare({"kernel": dict(per["blocks_and_attention"]), "torch": dict(per["unadopted"])}),
                         "against_blocks_only": compare({"kernel": dict(per["blocks_and_attention"]), "torch": dict(per["blocks"])})}

    # ---- (c) the unadopted attention block inside a training batch, by HIP events
    net = nets["unadopted"]
    block = net.hidden[-1]
    cfg = TL.LossConfig(**CONFIG_B)
    marks = {}

    def event():
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        return e

    def pre(mod, inputs):
        marks["fwd_begin"] = event()
        if inputs[0].requires_grad:
            inputs[0].register_hook(lambda g: marks.__setitem__("bwd_end", event()))

    def post(mod, inputs, output):
        marks["fwd_end"] = event()
        output.register_hook(lambda g: marks.__setitem__("bwd_begin", event()))
    handles = [block.register_forward_pre_hook(pre), block.register_forward_hook(post)]
    shares = []
    net.train()
    for rep in range(5):
        marks.clear()
        net.opt.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        begin = event()
        heads = net(batch[0], batch[6])
        TL.training_loss(*heads, batch, net.aux_target_offset, cfg, route="kernel").total.backward()
        end = event()
        torch.cuda.synchronize()
        shares.append((marks["fwd_begin"].elapsed_time(marks["fwd_end"]), marks["bwd_begin"].elapsed_time(marks["bwd_end"]),
                       begin.elapsed_time(end)))
    for h in handles:
        h.remove()
    fwd, bwd, whole = (statistics.median(s[k] for s in shares[1:]) for k in range(3))
    out["attention_in_a_batch"] = {"rows": args.step_rows, "route": "torch (unadopted)", "samples": len(shares) - 1,
                                   "forward_ms": round(fwd, 3), "backward_ms": round(bwd, 3),
                                   "forward_loss_backward_ms": round(whole, 3), "share": round((fwd + bwd) / whole, 3),
                                   "clock": "HIP events on the stream; the optimiser step is outside the interval"}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
