"""The Connect4 heads' training forward and backward: the column policy head and the WDL value + moves-left head as one
function of the tokens - the last network piece of the training side.

The reference's `CNN` ends with `policy_head` (`ColumnPolicyHead`: an RMS norm, a row gate whose softmax pools the six
rows of each column, a 64 x 64 layer with SiLU and dropout, one logit per column, the legal-move mask and a log-softmax)
and `dual_head` (`DualHead`: the mean token, a residual 64 x 64 layer with dropout, another 64 x 64 layer between RMS
norms, WDL log-probabilities and a sigmoid moves-left fraction).  Here:

    heads          the two as ONE autograd node: tokens [N, 42, 64] -> (log_p [N, 7], value [N, 3], steps [N]).
                   route="kernel" (the default for CUDA tensors) is az_train_dev_heads_fwd / az_train_dev_heads_bwd
                   (include/az_train.h, csrc/train_heads_kernels.hip): one launch forward, two backward, nothing waits for
                   the device; only the inputs are saved (the backward runs the forward again), nothing under
                   `torch.no_grad()`.  route="torch" is the header's formulas in plain torch with explicit dropout
                   factors: the only route on the CPU, the baseline on a GPU.
    adopt_heads    gives a module with the reference's names a forward that runs its embedding and `hidden` as they are
                   and then calls `heads` once with the two head modules' own parameters; `restore_heads` puts the class's
                   forward back.
    adopt_all      the four adoptions - residual blocks, attention block, stem, heads - in one call; `restore_all`.

Opt-in: az_net.py, train_loss.py, train_block.py, train_attn.py, train_stem.py and every existing caller behave as before.

Needs torch and src.abi only: a learner does not import the engine."""
import ctypes as C

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from src import train_route as R
from src.abi import TrainHeadsGradsC, TrainHeadsParamsC, _stream, check, lib

CHANNELS, ROWS, COLS, TOKENS, CLASSES = 64, 6, 7, 42, 3
# az_train_heads_params, in its order: (field, the reference's attribute path, shape)
PARAMS = (("policy_norm_weight", "policy_head.norm.weight", (CHANNELS,)),
          ("row_gate_weight", "policy_head.row_gate.weight", (1, CHANNELS)),
          ("row_gate_bias", "policy_head.row_gate.bias", (1,)),
          ("policy_fc_weight", "policy_head.fc.weight", (CHANNELS, CHANNELS)),
          ("policy_fc_bias", "policy_head.fc.bias", (CHANNELS,)),
          ("policy_out_weight", "policy_head.out.weight", (1, CHANNELS)),
          ("policy_out_bias", "policy_head.out.bias", (1,)),
          ("pool_norm_weight", "dual_head.pool_norm.weight", (CHANNELS,)),
          ("pool_fc_weight", "dual_head.pool_fc.weight", (CHANNELS, CHANNELS)),
          ("pool_fc_bias", "dual_head.pool_fc.bias", (CHANNELS,)),
          ("norm_weight", "dual_head.norm.weight", (CHANNELS,)),
          ("fc_weight", "dual_head.fc.weight", (CHANNELS, CHANNELS)),
          ("fc_bias", "dual_head.fc.bias", (CHANNELS,)),
          ("out_norm_weight", "dual_head.out_norm.weight", (CHANNELS,)),
          ("value_out_weight", "dual_head.value_out.weight", (CLASSES, CHANNELS)),
          ("value_out_bias", "dual_head.value_out.bias", (CLASSES,)),
          ("aux_out_weight", "dual_head.aux_out.weight", (1, CHANNELS)),
          ("aux_out_bias", "dual_head.aux_out.bias", (1,)))
NPARAM = len(PARAMS)


def _rms(v, w, eps):
    return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps) * w


def _torch_heads(tokens, legal, params, keep_policy, keep_pool, eps):
    (p_norm, gate_w, gate_b, p_fc_w, p_fc_b, out_w, out_b,
     pool_norm, pool_w, pool_b, norm, fc_w, fc_b, out_norm, val_w, val_b, aux_w, aux_b) = params
    n = tokens.shape[0]
    xn = _rms(tokens, p_norm, eps).reshape(n, ROWS, COLS, CHANNELS).transpose(1, 2)     # [N, 7, 6, 64]
    w = torch.softmax(F.linear(xn, gate_w, gate_b).squeeze(-1), dim=-1)                 # over the six rows
    colf = (w.unsqueeze(-1) * xn).sum(dim=2)
    a = F.silu(F.linear(colf, p_fc_w, p_fc_b))
    if keep_policy is not None:
        a = a * keep_policy
    logit = F.linear(a, out_w, out_b).squeeze(-1)
    if legal is not None:
        logit = logit.masked_fill(~legal, -1e9)
    log_p = F.log_softmax(logit, dim=-1)
    m = tokens.mean(dim=1)
    z = F.silu(F.linear(_rms(m, pool_norm, eps), pool_w, pool_b))
    if keep_pool is not None:
        z = z * keep_pool
    x1 = m + z
    h = _rms(F.silu(F.linear(_rms(x1, norm, eps), fc_w, fc_b)), out_norm, eps)
    return log_p, F.log_softmax(F.linear(h, val_w, val_b), dim=-1), torch.sigmoid(F.linear(h, aux_w, aux_b).squeeze(-1))


def _why_not_kernel(tokens, legal, params, keep_policy, keep_pool):
    """The reason the kernel route cannot take these tensors, or None."""
    if not isinstance(tokens, torch.Tensor) or tokens.dim() != 3 or tuple(tokens.shape[1:]) != (TOKENS, CHANNELS):
        return "route='kernel' takes tokens of shape [N, 42, 64], got %s" % (tuple(getattr(tokens, "shape", ())),)
    n = tokens.shape[0]
    if n == 0:
        return "route='kernel' needs at least one sample"
    named = [("tokens", (n, TOKENS, CHANNELS), tokens)] + [(name, shape, t) for (name, _, shape), t in zip(PARAMS, params)]
    if keep_policy is not None:
        named.append(("keep_policy", (n, COLS, CHANNELS), keep_policy))
    if keep_pool is not None:
        named.append(("keep_pool", (n, CHANNELS), keep_pool))
    return R.tensor_fault(named, tokens.device, any_strides=("tokens",)) or _legal_fault(tokens, legal) or R.cuda_fault(tokens)


def _legal_fault(tokens, legal):
    if legal is None:
        return None
    if not isinstance(legal, torch.Tensor) or tuple(legal.shape) != (tokens.shape[0], COLS) or legal.dtype != torch.bool:
        return "route='kernel' takes legal of shape [N, 7] and dtype bool"
    if legal.device != tokens.device or not legal.is_contiguous():
        return "route='kernel' needs a contiguous legal on the tokens' device"
    return None


def _launch_fwd(tokens, legal, params, keep_policy, keep_pool, eps):
    """(log_p, value, steps); one launch on the current stream."""
    n = tokens.shape[0]
    log_p = torch.empty((n, COLS), dtype=torch.float32, device=tokens.device)
    value = torch.empty((n, CLASSES), dtype=torch.float32, device=tokens.device)
    steps = torch.empty((n,), dtype=torch.float32, device=tokens.device)
    with torch.cuda.device(tokens.device):
        check(lib().az_train_dev_heads_fwd(C.byref(TrainHeadsParamsC(*(p.data_ptr() for p in params))), tokens.data_ptr(), R.ptr(legal),
                                           R.ptr(keep_policy), R.ptr(keep_pool), n, eps, log_p.data_ptr(), value.data_ptr(),
                                           steps.data_ptr(), _stream()))
    return log_p, value, steps


class _Heads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tokens, legal, keep_policy, keep_pool, eps, max_workgroups, *params):
        out = _launch_fwd(tokens, legal, params, keep_policy, keep_pool, eps)
        ctx.save_for_backward(tokens, legal, keep_policy, keep_pool, *params)
        ctx.knobs = (eps, max_workgroups)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_log_p, d_value, d_steps):
        tokens, legal, keep_policy, keep_pool, *params = ctx.saved_tensors
        eps, max_workgroups = ctx.knobs
        n = tokens.shape[0]
        # an output nobody used arrives as None: its gradient is zero
        ups = [torch.zeros(shape, dtype=torch.float32, device=tokens.device) if g is None else g.contiguous()
               for g, shape in ((d_log_p, (n, COLS)), (d_value, (n, CLASSES)), (d_steps, (n,)))]
        L = lib()
        work, size = R.workspace(L.az_train_heads_workspace_bytes, n, max_workgroups, tokens.device)
        d_tokens = torch.empty_like(tokens)
        d_params = [torch.empty_like(p) for p in params]
        grads = TrainHeadsGradsC(d_tokens.data_ptr(), *(g.data_ptr() for g in d_params), work.data_ptr(), size)
        with torch.cuda.device(tokens.device):
            check(L.az_train_dev_heads_bwd(C.byref(TrainHeadsParamsC(*(p.data_ptr() for p in params))), tokens.data_ptr(), R.ptr(legal),
                                           R.ptr(keep_policy), R.ptr(keep_pool), *(u.data_ptr() for u in ups), n, eps, max_workgroups,
                                           C.byref(grads), _stream()))
        return (d_tokens, None, None, None, None, None, *d_params)


def heads(tokens, legal, policy_norm_weight, row_gate_weight, row_gate_bias, policy_fc_weight, policy_fc_bias, policy_out_weight,
          policy_out_bias, pool_norm_weight, pool_fc_weight, pool_fc_bias, norm_weight, fc_weight, fc_bias, out_norm_weight,
          value_out_weight, value_out_bias, aux_out_weight, aux_out_bias, keep_policy=None, keep_pool=None, eps=1e-5, route=None,
          max_workgroups=0):
    """Both Connect4 heads on tokens [N, 42, 64] (token 7 * row + col) -> (log_p [N, 7], value [N, 3], steps [N]); the
    formulas are in include/az_train.h.  `legal` [N, 7] bool or None (all legal): an illegal column's logit is -1e9 before
    the log-softmax.  The eighteen parameters are the two head modules' own, in the order of az_train_heads_params (`PARAMS`
    names them).  `keep_policy` [N, 7, 64] and `keep_pool` [N, 64] are the two dropout factors, 0 or 1 / (1 - p) per
    element, None for all ones; they and `legal` get no gradient.

    route: None ("kernel" when the tokens are a CUDA tensor, else "torch"), "kernel" or "torch".  The kernel route takes
    float32 tensors on one CUDA device; tokens that are not contiguous are copied once.  Anything else it cannot take is a
    ValueError with the reason: there is no silent fallback.  Its backward is computed all at once (d_tokens and all
    eighteen gradients, not differentiable again); an upstream gradient that is not contiguous is made so, one that is
    None (an output nobody used) counts as zero.  `max_workgroups` caps the workgroups of the backward and with them the
    workspace (0: the kernels' default, see az_train.h).  Under `torch.no_grad()`, or when nothing needs a gradient,
    nothing is saved."""
    route = R.resolve(route, tokens)
    params = (policy_norm_weight, row_gate_weight, row_gate_bias, policy_fc_weight, policy_fc_bias, policy_out_weight, policy_out_bias,
              pool_norm_weight, pool_fc_weight, pool_fc_bias, norm_weight, fc_weight, fc_bias, out_norm_weight, value_out_weight,
              value_out_bias, aux_out_weight, aux_out_bias)
    if route == "torch":
        return _torch_heads(tokens, legal, params, keep_policy, keep_pool, eps)
    why = _why_not_kernel(tokens, legal, params, keep_policy, keep_pool)
    if why is not None:
        raise ValueError(why)
    R.check_knobs(max_workgroups, eps)
    if not tokens.is_contiguous():
        tokens = tokens.contiguous()
    if torch.is_grad_enabled() and any(t.requires_grad for t in (tokens,) + params):
        return _Heads.apply(tokens, legal, keep_policy, keep_pool, float(eps), int(max_workgroups), *params)
    return _launch_fwd(tokens.detach(), legal, tuple(p.detach() for p in params), keep_policy, keep_pool, float(eps))


def draw_keep(shape, p, device, generator=None):
    """A dropout factor tensor at rate p: independent Bernoulli(1 - p) / (1 - p) per element; p <= 0 gives None (all ones),
    p >= 1 all zeros."""
    p = float(p)
    if p <= 0.0:
        return None
    keep = torch.empty(shape, dtype=torch.float32, device=device)
    if p >= 1.0:
        return keep.zero_()
    return keep.bernoulli_(1.0 - p, generator=generator).div_(1.0 - p)


# ---------------------------------------------------------------------------------------- a module's heads

_EMBED_NAMES = ("_embed_state", "embed")        # the reference's spelling first: its forward goes through that one


def _resolve(net, path):
    obj = net
    for part in path.split("."):
        obj = getattr(obj, part, None)
        if obj is None:
            return None
    return obj


def _check(net):
    if not all(hasattr(net, k) for k in ("hidden", "policy_head", "dual_head")):
        raise ValueError("adopt_heads takes a module with the reference's names: `hidden`, `policy_head`, `dual_head`")
    if not any(callable(getattr(type(net), k, None)) for k in _EMBED_NAMES):
        raise ValueError("adopt_heads takes a module with an `embed` or `_embed_state` method")
    for name, path, shape in PARAMS:
        w = _resolve(net, path)
        if not isinstance(w, torch.Tensor) or tuple(w.shape) != shape:
            raise ValueError("adopt_heads takes the 64-wide Connect4 heads: %s is not %s" % (path, list(shape)))
    norms = (net.policy_head.norm, net.dual_head.pool_norm, net.dual_head.norm, net.dual_head.out_norm)
    eps = {getattr(m, "eps", None) for m in norms}
    if len(eps) != 1 or None in eps:
        raise ValueError("adopt_heads takes four norms with one explicit eps, got %s" % sorted(map(str, eps)))
    return eps.pop()


def _normalise_mask(action_mask, device):
    """The class's own normalisation of the legal-move mask (Connect4Net.forward, the reference's `_normalize_action_mask`)."""
    if action_mask is None:
        return None
    if not isinstance(action_mask, torch.Tensor):
        action_mask = torch.as_tensor(action_mask)       # a numpy array, as the class takes one
    if action_mask.ndim == 1:
        action_mask = action_mask.unsqueeze(0)
    return action_mask.to(device=device, dtype=torch.bool)


def _rate(module, name):
    return float(getattr(getattr(module, name, None), "p", 0.0) or 0.0)


def adopt_heads(net, route=None):
    """Gives a module with the reference's names - az_net.Connect4Net, or the reference's CNN - an instance-attribute
    `forward` that normalises the legal-move mask as the class does, runs the class's embedding method (`_embed_state`
    or `embed`) and `hidden` AS THEY ARE FOUND ON THE INSTANCE - so `adopt_stem`'s pass-through, `adopt_blocks` and
    `adopt_attention` keep working, in any order - and then calls `heads` ONCE with the parameters of `policy_head` and
    `dual_head`.  Returns 1.

    ValueError unless the eighteen parameters have the 64-wide Connect4 shapes and the four `RMSNorm`s share one explicit
    eps.  Independent of the other three adoptions.  Parameters, state dict, optimiser groups and `train_step` are
    untouched; `restore_heads(net)` puts the class's forward back.  Adopting twice replaces the route.

    In training mode `policy_head.dropout.p` and `dual_head.pool_drop.p` (the reference's attributes; absent counts as 0)
    draw factors of bernoulli(1 - p) / (1 - p) per element from torch's generator, [N, 7, 64] and [N, 64].  The
    DISTRIBUTION is torch's, the RANDOM STREAM is not: the same seed gives other masks than the unadopted module draws.

    Opt-in.  Measured on an MI355X (tools/measure_heads.py), two runs: the heads' forward + backward
    alone takes 167 us (388 in a disturbed second run) against 944 and 1073 for the unadopted modules at N = 1024, and 696
    and 693 against 2703 and 2696 at N = 8192.  A whole `train_step` batch of 1024 rows on the Connect4 module with stem,
    blocks, attention and heads adopted took 1.43 against 2.47 ms and 1.43 against 2.53 ms at the median, 42 % less than
    with the other three alone; the gap was beyond that route's own min-max spread in both runs.  The unadopted heads were
    1.36 ms, 50 %, of such a batch's forward + loss + backward."""
    R.check_route(route)
    eps = _check(net)
    embed_name = next(k for k in _EMBED_NAMES if callable(getattr(type(net), k, None)))

    def forward(x, action_mask=None):
        legal = _normalise_mask(action_mask, x.device)
        tokens = net.hidden(getattr(net, embed_name)(x))
        n = tokens.shape[0]
        if legal is not None and legal.shape[0] != n:
            legal = legal.expand(n, COLS)
        if legal is not None:
            legal = legal.contiguous()
        ph, dh = net.policy_head, net.dual_head
        keep_policy = draw_keep((n, COLS, CHANNELS), _rate(ph, "dropout"), tokens.device) if ph.training else None
        keep_pool = draw_keep((n, CHANNELS), _rate(dh, "pool_drop"), tokens.device) if dh.training else None
        return heads(tokens, legal, *(_resolve(net, path) for _, path, _ in PARAMS), keep_policy=keep_policy, keep_pool=keep_pool,
                     eps=eps, route=route)
    R.adopt(net, "_az_heads_adopted", forward)
    return 1


def restore_heads(net):
    """Undoes `adopt_heads`: the module runs its class's forward again.  Returns the number restored (0 or 1)."""
    return R.restore(net, "_az_heads_adopted")


def adopt_all(net, route=None):
    """`adopt_blocks`, `adopt_attention`, `adopt_stem` and `adopt_heads` on one module: with route="kernel" on a GPU the
    whole training batch - state, stem, blocks, attention, heads, and with `train_step(route="kernel")` the loss, the
    clipping and the AdamW step - runs as the project's kernels.  Returns the four counts (blocks, attention, stem, heads):
    (3, 1, 1, 1) on the reference's network.  A ValueError of any of the four leaves what was adopted before it undone."""
    from src import train_attn, train_block, train_stem
    done = []
    try:
        counts = []
        for adopt, restore in ((train_block.adopt_blocks, train_block.restore_blocks),
                               (train_attn.adopt_attention, train_attn.restore_attention),
                               (train_stem.adopt_stem, train_stem.restore_stem), (adopt_heads, restore_heads)):
            counts.append(adopt(net, route=route))
            done.append(restore)
    except ValueError:
        for restore in reversed(done):
            restore(net)
        raise
    return tuple(counts)


def restore_all(net):
    """Undoes `adopt_all` (or whichever of the four adoptions the module has): the counts restored, in `adopt_all`'s order."""
    from src import train_attn, train_block, train_stem
    return (train_block.restore_blocks(net), train_attn.restore_attention(net), train_stem.restore_stem(net), restore_heads(net))
