"""The Connect4 gated attention block's training forward and backward: the second network piece of the training side.

The reference's `AttentionBlock(64, 4, dropout)` wraps `GatedAttention`: an RMS pre-norm, the q/k/v and gate projections,
16-wide RMS norms on q and k, softmax attention over the 42 cells with dropout on the probabilities, a sigmoid gate per
head, the output projection and the skip connection; float32, the last layer of `net.hidden`.  Here:

    gated_attention   the block as ONE autograd node.  route="kernel" (the default for CUDA tensors) is
                      az_train_dev_attn_fwd / az_train_dev_attn_bwd (include/az_train.h, csrc/train_attn_kernels.hip):
                      one launch forward, two backward, nothing waits for the device; only the inputs are saved (the
                      backward runs the forward again), nothing under `torch.no_grad()`.  route="torch" is the header's
                      formula in plain torch with an explicit mask made from the bits: the only route on the CPU, the
                      baseline on a GPU.
    draw_keep_bits    the dropout mask of a batch as the kernels take it: one 64-bit word per (sample, head, query).
    adopt_attention   gives the attention block of a module with the reference's names (`net.hidden`) a forward that
                      calls `gated_attention` with the block's own parameters; `restore_attention` puts the original
                      forward back.

Opt-in: az_net.py, train_loss.py, train_block.py and every existing caller behave as before.

Needs torch and src.abi only: a learner does not import the engine."""
import ctypes as C

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from src import train_route as R
from src.abi import TrainAttnGradsC, TrainAttnParamsC, _stream, check, lib

CHANNELS, ROWS, COLS, HEADS, HEAD_DIM = 64, 6, 7, 4, 16
TOKENS = ROWS * COLS
PARAM_SHAPES = (("prenorm_weight", (CHANNELS,)), ("qkv_weight", (3 * CHANNELS, CHANNELS)), ("gate_weight", (HEADS, CHANNELS)),
                ("o_weight", (CHANNELS, CHANNELS)), ("q_norm_weight", (HEAD_DIM,)), ("k_norm_weight", (HEAD_DIM,)))


def _rms(v, w, eps):
    return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps) * w


def keep_mask(keep_bits, dtype=torch.float32):
    """[N, 4, 42] words -> [N, 4, 42, 42] of 0 and 1: bit j of word (n, a, i) is entry (n, a, i, j); bits 42 and above are ignored."""
    j = torch.arange(TOKENS, device=keep_bits.device)
    return ((keep_bits[..., None] >> j) & 1).to(dtype)


def _torch_attention(x, prenorm_weight, qkv_weight, gate_weight, o_weight, q_norm_weight, k_norm_weight, keep_bits, keep_scale, eps):
    n = x.shape[0]
    tok = x.flatten(2).transpose(1, 2)                              # [N, 42, 64]
    h = _rms(tok, prenorm_weight, eps)
    q, k, v = F.linear(h, qkv_weight).view(n, TOKENS, 3, HEADS, HEAD_DIM).unbind(2)
    gate = F.linear(h, gate_weight)                                 # [N, 42, 4]
    q = _rms(q, q_norm_weight, eps).transpose(1, 2)                 # [N, 4, 42, 16]
    k = _rms(k, k_norm_weight, eps).transpose(1, 2)
    p = torch.softmax((q @ k.transpose(-1, -2)) * HEAD_DIM ** -0.5, dim=-1)
    if keep_bits is not None:
        p = p * (keep_mask(keep_bits, p.dtype) * keep_scale)
    o = (p @ v.transpose(1, 2)) * torch.sigmoid(gate.transpose(1, 2).unsqueeze(-1))
    return F.linear(o.transpose(1, 2).reshape(n, TOKENS, CHANNELS), o_weight) + tok


def _why_not_kernel(x, params, keep_bits, keep_scale):
    """The reason the kernel route cannot take these tensors, or None."""
    if x.dim() != 4 or tuple(x.shape[1:]) != (CHANNELS, ROWS, COLS):
        return "route='kernel' takes x of shape [N, 64, 6, 7], got %s" % (tuple(x.shape),)
    if x.shape[0] == 0:
        return "route='kernel' needs at least one sample"
    named = [("x", x.shape, x)] + [(name, shape, t) for (name, shape), t in zip(PARAM_SHAPES, params)]
    return R.tensor_fault(named, x.device, any_strides=("x",)) or _mask_fault(x, keep_bits, keep_scale) or R.cuda_fault(x)


def _mask_fault(x, keep_bits, keep_scale):
    if keep_bits is None:
        return None if keep_scale == 1.0 else "route='kernel' needs keep_scale 1 without keep_bits"
    if tuple(keep_bits.shape) != (x.shape[0], HEADS, TOKENS) or keep_bits.dtype != torch.int64:
        return "route='kernel' takes keep_bits of shape [N, 4, 42] and dtype int64"
    if keep_bits.device != x.device or not keep_bits.is_contiguous():
        return "route='kernel' needs contiguous keep_bits on x's device"
    if not (keep_scale >= 1.0 and keep_scale != float("inf")):
        return "route='kernel' needs a finite keep_scale of at least 1"
    return None


def _token_major(x):
    """0 for a contiguous [N, 64, 6, 7], 1 for a channels-last one (its memory is [N, 42, 64]), None for anything else."""
    if x.is_contiguous():
        return 0
    if x.is_contiguous(memory_format=torch.channels_last):
        return 1
    return None


def _params(params):
    return TrainAttnParamsC(*(p.data_ptr() for p in params))


def _launch_fwd(x, params, keep_bits, keep_scale, eps):
    """y [N, 42, 64]; one launch on the current stream."""
    n = x.shape[0]
    y = torch.empty((n, TOKENS, CHANNELS), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(lib().az_train_dev_attn_fwd(C.byref(_params(params)), x.data_ptr(), _token_major(x),
                                          R.ptr(keep_bits), keep_scale, n, eps, y.data_ptr(), _stream()))
    return y


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, prenorm_weight, qkv_weight, gate_weight, o_weight, q_norm_weight, k_norm_weight, keep_bits, keep_scale, eps,
                max_workgroups):
        params = (prenorm_weight, qkv_weight, gate_weight, o_weight, q_norm_weight, k_norm_weight)
        y = _launch_fwd(x, params, keep_bits, keep_scale, eps)
        ctx.save_for_backward(x, *params, keep_bits)
        ctx.knobs = (keep_scale, eps, max_workgroups)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, *params, keep_bits = ctx.saved_tensors
        keep_scale, eps, max_workgroups = ctx.knobs
        dy = dy.contiguous()
        n = x.shape[0]
        L = lib()
        work, size = R.workspace(L.az_train_attn_workspace_bytes, n, max_workgroups, x.device)
        dx = torch.empty_like(x)                                    # x's strides: dx leaves in the layout x came in
        d_params = [torch.empty_like(p) for p in params]
        grads = TrainAttnGradsC(dx.data_ptr(), *(g.data_ptr() for g in d_params), work.data_ptr(), size)
        with torch.cuda.device(x.device):
            check(L.az_train_dev_attn_bwd(C.byref(_params(params)), x.data_ptr(), _token_major(x),
                                          R.ptr(keep_bits), keep_scale, dy.data_ptr(), n, eps,
                                          max_workgroups, C.byref(grads), _stream()))
        return (dx, *d_params, None, None, None, None)


def gated_attention(x, prenorm_weight, qkv_weight, gate_weight, o_weight, q_norm_weight, k_norm_weight, keep_bits=None,
                    keep_scale=1.0, eps=1e-5, route=None, max_workgroups=0):
    """The gated attention block on x [N, 64, 6, 7] (cell 7 * row + col is token t) -> y [N, 42, 64]; the formula is in
    include/az_train.h.  `keep_bits` [N, 4, 42] int64: bit j of word (n, a, i) keeps probability (a, i, j), kept ones are
    multiplied by `keep_scale`; None keeps all.  The mask gets no gradient.

    route: None ("kernel" when x is a CUDA tensor, else "torch"), "kernel" or "torch".  The kernel route takes float32
    tensors on one CUDA device; x may be contiguous or channels-last (its memory is then read as [N, 42, 64], and dx
    leaves the same way), any other stride pattern is copied once.  Anything else it cannot take is a ValueError with
    the reason: there is no silent fallback.  Its backward is computed all at once (all seven gradients, not
    differentiable again); an upstream gradient that is not contiguous is made so.  `max_workgroups` caps the workgroups
    of the backward and with them the workspace (0: the kernels' default, see az_train.h).  Under `torch.no_grad()`, or
    when no input needs a gradient, nothing is saved."""
    route = R.resolve(route, x)
    params = (prenorm_weight, qkv_weight, gate_weight, o_weight, q_norm_weight, k_norm_weight)
    keep_scale = float(keep_scale)
    if route == "torch":
        return _torch_attention(x, *params, keep_bits, keep_scale, eps)
    why = _why_not_kernel(x, params, keep_bits, keep_scale)
    if why is not None:
        raise ValueError(why)
    R.check_knobs(max_workgroups, eps)
    if _token_major(x) is None:
        x = x.contiguous()
    if torch.is_grad_enabled() and any(t.requires_grad for t in (x,) + params):
        return _Attention.apply(x, *params, keep_bits, keep_scale, float(eps), int(max_workgroups))
    return _launch_fwd(x.detach(), tuple(p.detach() for p in params), keep_bits, keep_scale, float(eps))


def draw_keep_bits(n, p, device, generator=None):
    """The dropout mask of n samples at rate p -> (int64 tensor [n, 4, 42], keep_scale): every bit 0 .. 41 of every word is
    an independent Bernoulli(1 - p), bits 42 and above are zero, keep_scale is 1 / (1 - p).  p = 0 gives (None, 1.0): no
    mask.  p >= 1 gives all-zero bits (and scale 1: nothing is kept to scale)."""
    p = float(p)
    if p <= 0.0:
        return None, 1.0
    if p >= 1.0:
        return torch.zeros((n, HEADS, TOKENS), dtype=torch.int64, device=device), 1.0
    # 0 / 1 as float32, packed 21 bits at a time: a sum below 2^21 is exact in float32 in any order, and the three passes over
    # N * 7056 floats are a third of what shifting int64 ones takes
    kept = torch.empty((n, HEADS, TOKENS, 2, TOKENS // 2), dtype=torch.float32, device=device).bernoulli_(1.0 - p, generator=generator)
    halves = (kept * torch.exp2(torch.arange(TOKENS // 2, dtype=torch.float32, device=kept.device))).sum(-1).to(torch.int64)
    return halves[..., 0] | (halves[..., 1] << (TOKENS // 2)), 1.0 / (1.0 - p)


# ---------------------------------------------------------------------------------------- a module's attention block

def _find(net):
    hidden = getattr(net, "hidden", None)
    if hidden is None:
        raise ValueError("adopt_attention takes a module with the reference's names: it has no `hidden`")
    names = ("prenorm", "qkv_proj", "gate_proj", "o_proj", "q_norm", "k_norm")
    for block in hidden.children():
        attn = getattr(block, "attn", None)
        if attn is not None and all(hasattr(attn, k) for k in names):
            return block
    raise ValueError("adopt_attention found no gated attention block in `hidden`")


def _check(attn):
    weights = (attn.prenorm.weight, attn.qkv_proj.weight, attn.gate_proj.weight, attn.o_proj.weight, attn.q_norm.weight, attn.k_norm.weight)
    for (name, shape), w in zip(PARAM_SHAPES, weights):
        if w is None or tuple(w.shape) != shape:
            raise ValueError("adopt_attention takes a 64-wide block of 4 heads of 16: %s is not %s" % (name, list(shape)))
    if any(getattr(m, "bias", None) is not None for m in (attn.qkv_proj, attn.gate_proj, attn.o_proj)):
        raise ValueError("adopt_attention takes projections without biases")
    eps = {m.eps for m in (attn.prenorm, attn.q_norm, attn.k_norm)}
    if len(eps) != 1 or None in eps:
        raise ValueError("adopt_attention takes three norms with one explicit eps, got %s" % sorted(map(str, eps)))
    return eps.pop()


def adopt_attention(net, route=None):
    """Gives the gated attention block of `net.hidden` - the child with an `attn` that has `prenorm`, `qkv_proj`,
    `gate_proj`, `o_proj`, `q_norm` and `k_norm`, as az_net.Connect4Net and the reference's CNN have it - a forward that
    calls `gated_attention` with the block's own parameters.  64 channels, 4 heads of 16, no biases and one eps for the
    three norms, or ValueError.  Returns 1.  The image may arrive contiguous or channels-last; neither is copied.
    Independent of `train_block.adopt_blocks`.  Parameters, state dict, optimiser groups and `train_step` are untouched;
    `restore_attention(net)` puts the original forward back.  Adopting twice replaces the route.

    In training mode with `attn.dropout_p > 0` (the reference's attribute; absent counts as 0) the mask is drawn by
    `draw_keep_bits` from torch's generator: independent Bernoulli(1 - p) per probability, kept ones times 1 / (1 - p), as
    the math form of scaled_dot_product_attention applies it.  The DISTRIBUTION is torch's, the RANDOM STREAM is not: the
    same seed gives other masks than the unadopted module draws.

    Opt-in.  Measured on an MI355X (tools/measure_attn.py), three runs: the block's forward + backward
    alone takes 319 us against the unadopted module's 1604 at N = 1024 and 1952 against 10259 at N = 8192 (392 against 1642
    and 2351 against 10447 with dropout 0.2, the mask words included).  A whole `train_step` batch of 1024 rows on the
    Connect4 module with blocks and attention adopted was 12 to 22 % shorter at the median than with the blocks alone; the
    gap was beyond the blocks-only route's own min-max spread in two runs and inside it in the third, a noisy one."""
    R.check_route(route)
    block = _find(net)
    _check(block.attn)

    def forward(x, block=block):
        attn = block.attn
        p = float(getattr(attn, "dropout_p", 0.0) or 0.0)
        bits, scale = draw_keep_bits(x.shape[0], p, x.device) if (attn.training and p > 0.0) else (None, 1.0)
        return gated_attention(x, attn.prenorm.weight, attn.qkv_proj.weight, attn.gate_proj.weight, attn.o_proj.weight,
                               attn.q_norm.weight, attn.k_norm.weight, bits, scale, attn.prenorm.eps, route)
    R.adopt(block, "_az_attn_adopted", forward)
    return 1


def restore_attention(net):
    """Undoes `adopt_attention`: the block runs its class's forward again.  Returns the number restored (0 or 1)."""
    return sum(R.restore(block, "_az_attn_adopted") for block in net.hidden.children())
