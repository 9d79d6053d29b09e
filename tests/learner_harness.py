"""What the native learner's tests (test_learner_cpu.py, test_learner_gpu.py) share: the built package with `src.learner` and
`src.replay` next to the training pieces, the seeded Connect4 module with or without the reference's dropout attributes,
the optimiser state of a module as numpy, and a replay ring filled from fixture G16.  A plain module: no fixture and no
pytest setting lives here."""
import importlib

import numpy as np

import train_gpu_harness as H
import train_loss_ref as TR
from test_train_loss_cpu import golden_batch

KNOBS = dict(TR.CONFIGS["b"])
MODULES = ("az_net", "optim", "train_attn", "train_block", "train_heads", "train_loss", "train_stem")


def load_env():
    env = H.load_env(MODULES)
    env["LN"] = importlib.import_module("src.learner")
    env["RP"] = importlib.import_module("src.replay")
    return env


def module(env, device="cuda", dropout=(0.0, 0.0, 0.0, 0.0)):
    """`H.module(..., stem_bias=True)` in float32; `dropout` = (blocks, attention, policy head, pool) puts the reference's
    attributes on it: `dropout` (Dropout2d) on every residual block, `attn.dropout_p`, `policy_head.dropout`,
    `dual_head.pool_drop`."""
    torch = env["torch"]
    net = H.module(env, torch.float32, device, stem_bias=True)
    p_block, p_attn, p_policy, p_pool = dropout
    if p_block:
        for b in list(net.hidden.children())[2:-1]:
            b.dropout = torch.nn.Dropout2d(p_block)
    if p_attn:
        list(net.hidden.children())[-1].attn.dropout_p = p_attn
    if p_policy:
        net.policy_head.dropout = torch.nn.Dropout(p_policy)
    if p_pool:
        net.dual_head.pool_drop = torch.nn.Dropout(p_pool)
    return net


def python_twin(env, dropout=(0.0, 0.0, 0.0, 0.0)):
    """The module on the Python route: all four pieces adopted, `net.opt` a ClipAdamW."""
    net = module(env, "cuda", dropout)
    assert env["TH"].adopt_all(net) == (3, 1, 1, 1)
    env["O"].adopt(net.opt)
    return net


def python_batch(env, net, batch, config, max_norm=5):
    """One batch as `train_step` runs it on the Python route -> (the TrainingLoss, the gradient norm)."""
    net.train()
    net.opt.zero_grad(set_to_none=True)
    log_p, value, steps = net(batch[0], action_mask=batch[6])
    loss = env["TL"].training_loss(log_p, value, steps, batch, net.aux_target_offset, config, "kernel")
    loss.total.backward()
    return loss, net.opt.clip_step(max_norm)


def trained_state(net):
    """name -> numpy: every parameter and, per parameter of the optimiser in its order, exp_avg, exp_avg_sq and step."""
    out = {"p." + k: v.detach().cpu().numpy() for k, v in net.named_parameters()}
    flat = [p for g in net.opt.param_groups for p in g["params"]]
    for i, p in enumerate(flat):
        s = net.opt.state[p]
        out["m.%d" % i], out["v.%d" % i] = s["exp_avg"].cpu().numpy(), s["exp_avg_sq"].cpu().numpy()
        out["t.%d" % i] = np.asarray(float(s["step"]))
    return out


def first_difference(a, b):
    """The first name whose bytes differ between two `trained_state`s, or None."""
    assert list(a) == list(b)
    for k in a:
        if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes():
            return k
    return None


def ring(env, rows=200):
    """A SampledReplayTensors ring of `rows` rows on the GPU filled from fixture G16's Connect4 rows (repeated as needed)."""
    torch, RP = env["torch"], env["RP"]
    g = golden_batch("c4")
    take = np.arange(rows) % len(g[0])
    buf = RP.SampledReplayTensors("Connect4", rows, device="cuda")
    names = ("state", "prob", "winner", "steps_to_end", "aux_target", "root_wdl", "valid_mask", "future_root_wdl")
    for name, x in zip(names, g):
        dst = getattr(buf, name)
        dst.copy_(torch.from_numpy(np.ascontiguousarray(x[take])).to(dst.dtype).reshape(dst.shape))
    buf._ptr = rows
    return buf
