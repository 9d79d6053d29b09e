"""The Connect4 stem's training forward and backward: embedding, first convolution and SiLU as one function of the position.

The reference's `CNN` starts with `_embed_state` (piece embeddings times the two planes, plus the positional embedding of
the cell's mirror orbit), `hidden[0]` (Conv2d(32, 64, 3, padding=1)) and `hidden[1]` (SiLU).  Here:

    stem         the three as ONE autograd node.  route="kernel" (the default for CUDA tensors) is az_train_dev_stem_fwd /
                 az_train_dev_stem_bwd (include/az_train.h, csrc/train_stem_kernels.hip): two launches forward, three
                 backward, nothing waits for the device; the convolution is folded into a 3840-float table of the
                 parameters, which is all that is saved - the backward forms z again.  The output is a contiguous NCHW
                 tensor: the first residual block takes it without a copy.  route="torch" is literally the module's own
                 ops: the only route on the CPU, the baseline on a GPU.
    adopt_stem   gives a module with the reference's names a forward that reaches `stem` with the module's own parameters;
                 `restore_stem` puts everything back.

Opt-in: az_net.py, train_loss.py, train_block.py, train_attn.py and every existing caller behave as before.

Needs torch and src.abi only: a learner does not import the engine."""
import ctypes as C

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from src import train_route as R
from src.abi import TrainStemGradsC, TrainStemParamsC, _stream, check, lib

EMBED, CHANNELS, ROWS, COLS, CELLS, ORBITS = 32, 64, 6, 7, 42, 24
TABLE_BYTES = 15360             # AZ_TRAIN_STEM_TABLE_BYTES
# the orbit map the kernels have compiled in: 4 * row + min(col, 6 - col)
ORBIT_MAP = tuple(4 * (cell // COLS) + min(cell % COLS, COLS - 1 - cell % COLS) for cell in range(CELLS))
PARAM_SHAPES = (("piece_emb", (2, EMBED)), ("pos_emb", (ORBITS, EMBED)), ("conv_weight", (CHANNELS, EMBED, 3, 3)),
                ("conv_bias", (CHANNELS,)))


_ORBITS_ON = {}                 # device -> the orbit map as an index tensor there


def _torch_stem(state, piece_emb, pos_emb, conv_weight, conv_bias):
    if state.device not in _ORBITS_ON:
        _ORBITS_ON[state.device] = torch.tensor(ORBIT_MAP, device=state.device)
    b = state.size(0)
    own = state[:, 0].reshape(b, CELLS, 1)
    opp = state[:, 1].reshape(b, CELLS, 1)
    x = own * piece_emb[0] + opp * piece_emb[1] + F.embedding(_ORBITS_ON[state.device], pos_emb)
    return F.silu(F.conv2d(x.transpose(1, 2).reshape(b, EMBED, ROWS, COLS), conv_weight, conv_bias, padding=1))


def _why_not_kernel(state, params):
    """The reason the kernel route cannot take these tensors, or None."""
    if not isinstance(state, torch.Tensor) or state.dim() != 4 or tuple(state.shape[1:]) != (3, ROWS, COLS):
        return "route='kernel' takes a state of shape [N, 3, 6, 7], got %s" % (tuple(getattr(state, "shape", ())),)
    if state.shape[0] == 0:
        return "route='kernel' needs at least one sample"
    named = [("state", state.shape, state)] + [(name, shape, t) for (name, shape), t in zip(PARAM_SHAPES, params)]
    return R.tensor_fault(named, state.device) or R.cuda_fault(state)


def _params(params):
    return TrainStemParamsC(*(p.data_ptr() for p in params))


def _launch_fwd(state, params):
    """y and the table the fold left; two launches on the current stream."""
    n = state.shape[0]
    y = torch.empty((n, CHANNELS, ROWS, COLS), dtype=torch.float32, device=state.device)
    table = torch.empty(TABLE_BYTES, dtype=torch.uint8, device=state.device)
    with torch.cuda.device(state.device):
        check(lib().az_train_dev_stem_fwd(C.byref(_params(params)), state.data_ptr(), n, y.data_ptr(), table.data_ptr(), TABLE_BYTES,
                                          _stream()))
    return y, table


class _Stem(torch.autograd.Function):
    @staticmethod
    def forward(ctx, state, piece_emb, pos_emb, conv_weight, conv_bias, max_workgroups):
        y, table = _launch_fwd(state, (piece_emb, pos_emb, conv_weight, conv_bias))
        ctx.save_for_backward(state, piece_emb, pos_emb, conv_weight, conv_bias, table)
        ctx.max_workgroups = max_workgroups
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        state, *params, table = ctx.saved_tensors
        dy = dy.contiguous()
        n = state.shape[0]
        L = lib()
        work, size = R.workspace(L.az_train_stem_workspace_bytes, n, ctx.max_workgroups, state.device)
        out = [torch.empty_like(p) for p in params]
        grads = TrainStemGradsC(*(g.data_ptr() for g in out), work.data_ptr(), size)
        with torch.cuda.device(state.device):
            check(L.az_train_dev_stem_bwd(C.byref(_params(params)), state.data_ptr(), table.data_ptr(), dy.data_ptr(), n,
                                          ctx.max_workgroups, C.byref(grads), _stream()))
        return (None, *out, None)


def stem(state, piece_emb, pos_emb, conv_weight, conv_bias, route=None, max_workgroups=0):
    """`silu(conv3x3(t, conv_weight, conv_bias))` with zero padding, where
    `t[n, c, cell] = (state[n, 0, cell] * piece_emb[0, c] + state[n, 1, cell] * piece_emb[1, c]) + pos_emb[orbit(cell), c]`:
    state [N, 3, 6, 7] (planes 0 and 1 are multipliers of any value, plane 2 is not read; it gets no gradient), piece_emb
    [2, 32], pos_emb [24, 32], conv_weight [64, 32, 3, 3], conv_bias [64] -> [N, 64, 6, 7].

    route: None ("kernel" when the state is a CUDA tensor, else "torch"), "kernel" or "torch".  The torch route is the
    module's own ops (its output is channels-last, as the module's is).  The kernel route takes float32, contiguous
    tensors on one CUDA device and returns a contiguous tensor; anything else is a ValueError with the reason: there is no
    silent fallback.  Its backward is computed all at once (all four gradients, not differentiable again); an upstream
    gradient that is not contiguous is made so.  `max_workgroups` caps the workgroups of the backward and with them the
    workspace (0: the kernels' default, see az_train.h).  Under `torch.no_grad()`, or when no parameter needs a gradient,
    only the forward runs."""
    route = R.resolve(route, state)
    params = (piece_emb, pos_emb, conv_weight, conv_bias)
    if route == "torch":
        return _torch_stem(state, *params)
    why = _why_not_kernel(state, params)
    if why is not None:
        raise ValueError(why)
    R.check_knobs(max_workgroups)
    if torch.is_grad_enabled() and any(p.requires_grad for p in params):
        return _Stem.apply(state.detach(), *params, int(max_workgroups))
    return _launch_fwd(state.detach(), tuple(p.detach() for p in params))[0]


# ---------------------------------------------------------------------------------------- a module's stem

_EMBED_NAMES = ("embed", "_embed_state")


def _check(net):
    hidden = getattr(net, "hidden", None)
    if hidden is None or not all(hasattr(net, k) for k in ("piece_emb", "pos_emb", "orbit_map")):
        raise ValueError("adopt_stem takes a module with the reference's names: `hidden`, `piece_emb`, `pos_emb`, `orbit_map`")
    if not any(callable(getattr(type(net), k, None)) for k in _EMBED_NAMES):
        raise ValueError("adopt_stem takes a module with an `embed` or `_embed_state` method")
    layers = list(hidden.children())
    conv = layers[0] if layers else None
    if not (len(layers) >= 2 and isinstance(conv, torch.nn.Conv2d) and isinstance(layers[1], torch.nn.SiLU) and
            (conv.in_channels, conv.out_channels) == (EMBED, CHANNELS) and conv.kernel_size == (3, 3) and
            conv.padding == (1, 1) and conv.stride == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1 and
            conv.bias is not None and conv.padding_mode == "zeros"):
        raise ValueError("adopt_stem takes a `hidden` that starts with a 3 x 3, 32 -> 64, padding-1, biased convolution and a SiLU")
    for (name, shape), w in zip(PARAM_SHAPES[:2], (net.piece_emb.weight, net.pos_emb.weight)):
        if tuple(w.shape) != shape:
            raise ValueError("adopt_stem takes a %s of shape %s" % (name, list(shape)))
    if tuple(int(v) for v in net.orbit_map.reshape(-1).tolist()) != ORBIT_MAP:
        raise ValueError("adopt_stem takes the Connect4 orbit map 4 * row + min(col, 6 - col): this module's `orbit_map` differs")
    return conv, layers[1]


def adopt_stem(net, route=None):
    """Gives a module with the reference's names - az_net.Connect4Net, or the reference's CNN - a forward that reaches
    `stem(state, piece_emb.weight, pos_emb.weight, hidden[0].weight, hidden[0].bias, route)` in place of its embedding
    method, `hidden[0]` and `hidden[1]`.  Three instance attributes do it: the embedding method (`embed`, `_embed_state`,
    whichever the class has) hands the state through as it is, `hidden[0].forward` calls `stem`, `hidden[1].forward` is the
    identity.  So a DIRECT call of an adopted module's `embed` returns the state, not the embedded image.  Returns 1.

    ValueError for a `hidden` that does not start with a 3 x 3, 32 -> 64, padding-1, biased convolution and a SiLU, for
    embeddings of another shape, and for an `orbit_map` buffer that differs from the map the kernels have compiled in.
    Independent of `train_block.adopt_blocks` and `train_attn.adopt_attention`; with the blocks adopted too, the first
    block gets a contiguous image and copies nothing.  Parameters, state dict, optimiser groups and `train_step` are
    untouched; `restore_stem(net)` puts the class's methods back.  Adopting twice replaces the route.

    Opt-in.  Measured on an MI355X (tools/measure_stem.py), two runs: the stem's forward + backward
    alone takes 103 us against 310 and 326 for the unadopted module with the first block's layout copy at N = 1024, and 242
    and 194 against 978 and 976 at N = 8192.  A whole `train_step` batch of 1024 rows on the Connect4 module with blocks,
    attention and stem adopted took 2.66 against 3.01 ms and 2.97 against 3.33 ms at the median, about 11 % less than with
    blocks and attention alone; the gap was beyond that route's own min-max spread in both runs.  The unadopted stem was
    0.42 ms, 14 %, of such a batch's forward + loss + backward."""
    R.check_route(route)
    conv, act = _check(net)

    def forward(state):
        return stem(state, net.piece_emb.weight, net.pos_emb.weight, conv.weight, conv.bias, route)
    for name in _EMBED_NAMES:
        if callable(getattr(type(net), name, None)):
            net.__dict__[name] = _passthrough       # instance attributes: the class's methods stay underneath
    conv.forward = forward
    act.forward = _passthrough
    net._az_stem_adopted = True
    return 1


def _passthrough(x):
    return x


def restore_stem(net):
    """Undoes `adopt_stem`: the module runs its class's embedding method, convolution and SiLU again.  Returns the number
    restored (0 or 1)."""
    if not net.__dict__.pop("_az_stem_adopted", False):
        return 0
    for name in _EMBED_NAMES:
        net.__dict__.pop(name, None)
    layers = list(net.hidden.children())
    for layer in layers[:2]:
        layer.__dict__.pop("forward", None)
    return 1
