"""The Connect4 residual block's training forward and backward: the first network piece of the training side.

The reference's `ResidualBlock(64, 64)` is `x + dropout(silu(conv3x3(GroupNorm(1, 64)(x))))`, float32, 64 channels on
6 x 7 cells, and the Connect4 module uses it three times.  Here:

    residual_block   the block as ONE autograd node.  route="kernel" (the default for CUDA tensors) is
                     az_train_dev_block_fwd / az_train_dev_block_bwd (include/az_train.h, csrc/train_block_kernels.hip):
                     one launch forward, two backward, nothing waits for the device; z and two floats per sample are
                     saved, nothing under `torch.no_grad()`.  route="torch" is literally
                     `x + keep[:, :, None, None] * F.silu(F.conv2d(F.group_norm(x, 1, ...), ..., padding=1))`: the only
                     route on the CPU, the baseline on a GPU.
    adopt_blocks     gives every such block of a module with the reference's names (`net.hidden`) a forward that calls
                     `residual_block` with the block's own parameters; `restore_blocks` puts the original forwards back.

Opt-in: az_net.py, train_loss.py and every existing caller behave as before.

Needs torch and src.abi only: a learner does not import the engine."""
import ctypes as C

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from src import train_route as R
from src.abi import TrainBlockGradsC, TrainBlockParamsC, TrainBlockSavedC, _stream, check, lib

CHANNELS, ROWS, COLS = 64, 6, 7


def _torch_block(x, norm_weight, norm_bias, conv_weight, conv_bias, keep, eps):
    h = F.silu(F.conv2d(F.group_norm(x, 1, norm_weight, norm_bias, eps), conv_weight, conv_bias, padding=1))
    return x + h if keep is None else x + keep[:, :, None, None] * h


def _why_not_kernel(x, norm_weight, norm_bias, conv_weight, conv_bias, keep):
    """The reason the kernel route cannot take these tensors, or None."""
    if x.dim() != 4 or tuple(x.shape[1:]) != (CHANNELS, ROWS, COLS):
        return "route='kernel' takes x of shape [N, 64, 6, 7], got %s" % (tuple(x.shape),)
    if x.shape[0] == 0:
        return "route='kernel' needs at least one sample"
    named = [("x", x.shape, x), ("norm_weight", (CHANNELS,), norm_weight), ("norm_bias", (CHANNELS,), norm_bias),
             ("conv_weight", (CHANNELS, CHANNELS, 3, 3), conv_weight), ("conv_bias", (CHANNELS,), conv_bias)]
    if keep is not None:
        named.append(("keep", (x.shape[0], CHANNELS), keep))
    return R.tensor_fault(named, x.device) or R.cuda_fault(x)


def _params(norm_weight, norm_bias, conv_weight, conv_bias):
    return TrainBlockParamsC(norm_weight.data_ptr(), norm_bias.data_ptr(), conv_weight.data_ptr(), conv_bias.data_ptr())


def _launch_fwd(x, norm_weight, norm_bias, conv_weight, conv_bias, keep, eps, save):
    """y, and (z, stats) when `save`; one launch on the current stream."""
    n = x.shape[0]
    y = torch.empty_like(x)
    z = torch.empty_like(x) if save else None
    stats = torch.empty((n, 2), dtype=torch.float32, device=x.device) if save else None
    saved = TrainBlockSavedC(z.data_ptr(), stats.data_ptr()) if save else None
    with torch.cuda.device(x.device):
        check(lib().az_train_dev_block_fwd(C.byref(_params(norm_weight, norm_bias, conv_weight, conv_bias)), x.data_ptr(),
                                           R.ptr(keep), n, eps, y.data_ptr(),
                                           None if saved is None else C.byref(saved), _stream()))
    return y, z, stats


class _Block(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, norm_weight, norm_bias, conv_weight, conv_bias, keep, eps, max_workgroups):
        y, z, stats = _launch_fwd(x, norm_weight, norm_bias, conv_weight, conv_bias, keep, eps, True)
        ctx.save_for_backward(x, norm_weight, norm_bias, conv_weight, conv_bias, keep, z, stats)
        ctx.max_workgroups = max_workgroups
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, norm_weight, norm_bias, conv_weight, conv_bias, keep, z, stats = ctx.saved_tensors
        dy = dy.contiguous()
        n = x.shape[0]
        L = lib()
        work, size = R.workspace(L.az_train_block_workspace_bytes, n, ctx.max_workgroups, x.device)
        dx, d_nw, d_nb = torch.empty_like(x), torch.empty_like(norm_weight), torch.empty_like(norm_bias)
        d_cw, d_cb = torch.empty_like(conv_weight), torch.empty_like(conv_bias)
        saved = TrainBlockSavedC(z.data_ptr(), stats.data_ptr())
        grads = TrainBlockGradsC(dx.data_ptr(), d_nw.data_ptr(), d_nb.data_ptr(), d_cw.data_ptr(), d_cb.data_ptr(), work.data_ptr(), size)
        with torch.cuda.device(x.device):
            check(L.az_train_dev_block_bwd(C.byref(_params(norm_weight, norm_bias, conv_weight, conv_bias)), x.data_ptr(),
                                           R.ptr(keep), dy.data_ptr(), C.byref(saved), n,
                                           ctx.max_workgroups, C.byref(grads), _stream()))
        return dx, d_nw, d_nb, d_cw, d_cb, None, None, None


def residual_block(x, norm_weight, norm_bias, conv_weight, conv_bias, keep=None, eps=1e-5, route=None, max_workgroups=0):
    """`x + keep[:, :, None, None] * silu(conv3x3(group_norm(x, 1, norm_weight, norm_bias, eps), conv_weight, conv_bias))`
    with zero padding; `keep` [N, 64] is the factor Dropout2d applies per sample and channel (0 or 1 / (1 - p)), None
    for all ones; it gets no gradient.

    route: None ("kernel" when x is a CUDA tensor, else "torch"), "kernel" or "torch".  The kernel route takes float32,
    contiguous tensors on one CUDA device, x [N, 64, 6, 7]; anything else is a ValueError with the reason: there is no
    silent fallback.  Its backward is computed all at once (all five gradients, not differentiable again); an upstream
    gradient that is not contiguous is made so.  `max_workgroups` caps the workgroups of the backward and with them the
    workspace (0: the kernels' default, see az_train.h).  Under `torch.no_grad()`, or when no input needs a gradient,
    nothing is saved."""
    if R.resolve(route, x) == "torch":
        return _torch_block(x, norm_weight, norm_bias, conv_weight, conv_bias, keep, eps)
    why = _why_not_kernel(x, norm_weight, norm_bias, conv_weight, conv_bias, keep)
    if why is not None:
        raise ValueError(why)
    R.check_knobs(max_workgroups, eps)
    tensors = (x, norm_weight, norm_bias, conv_weight, conv_bias)
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        return _Block.apply(x, norm_weight, norm_bias, conv_weight, conv_bias, keep, float(eps), int(max_workgroups))
    return _launch_fwd(*(t.detach() for t in tensors), keep, float(eps), False)[0]


# ---------------------------------------------------------------------------------------- a module's blocks

def _is_block(m):
    conv, norm = getattr(m, "conv", None), getattr(m, "norm", None)
    return (isinstance(conv, torch.nn.Conv2d) and isinstance(norm, torch.nn.GroupNorm) and
            (conv.in_channels, conv.out_channels) == (CHANNELS, CHANNELS) and conv.kernel_size == (3, 3) and
            conv.padding == (1, 1) and conv.stride == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1 and
            conv.bias is not None and conv.padding_mode == "zeros" and
            norm.num_groups == 1 and norm.num_channels == CHANNELS and norm.affine and getattr(m, "resid", True))


def _keep(block, x):
    drop = getattr(block, "dropout", None)
    p = float(getattr(drop, "p", 0.0)) if drop is not None else 0.0
    if not (block.training and p > 0.0):
        return None
    if p >= 1.0:
        return torch.zeros((x.shape[0], CHANNELS), device=x.device, dtype=x.dtype)
    return torch.bernoulli(torch.full((x.shape[0], CHANNELS), 1 - p, device=x.device, dtype=x.dtype)) / (1 - p)


def adopt_blocks(net, route=None):
    """Gives every residual block of `net.hidden` - a child with a 3 x 3, 64 -> 64, padding-1 `conv` and a
    `GroupNorm(1, 64)` `norm`, as az_net.Connect4Net and the reference's CNN have them - a forward that calls
    `residual_block(x, norm.weight, norm.bias, conv.weight, conv.bias, keep, norm.eps, route)`.  Returns the number of
    blocks adopted.  On the kernel route an input that is not contiguous (the stem's output is channels-last) is copied
    once; the torch route gets it as it is.  Parameters, state dict, optimiser groups and `train_step` are untouched; `restore_blocks(net)` puts
    the original forwards back.  Adopting twice replaces the route.

    A block with a `dropout` module of p > 0 in training mode draws its factors per (sample, channel) from torch's
    generator: `bernoulli(1 - p) / (1 - p)`.  The DISTRIBUTION is Dropout2d's, the RANDOM STREAM is not: the same seed
    gives other masks than the unadopted module draws.

    Opt-in.  Measured on an MI355X (tools/measure_block.py): a block's forward + backward alone takes
    215 us against torch's 277 at N = 1024 and 1218 against 1646 at N = 8192.  A whole `train_step` batch of 1024 rows on
    the Connect4 module was 5 to 7 % shorter at the median in two runs (3.65 against 3.85 ms, 3.97 against 4.28 ms); the
    gap was beyond the unadopted route's own min-max spread in the first of them and inside it in the second, where one
    window ran long on both routes."""
    R.check_route(route)
    hidden = getattr(net, "hidden", None)
    if hidden is None:
        raise ValueError("adopt_blocks takes a module with the reference's names: it has no `hidden`")
    count = 0
    for block in hidden.children():
        if not _is_block(block):
            continue

        def forward(x, block=block):
            norm, conv = block.norm, block.conv
            if route == "kernel" or (route is None and x.is_cuda):
                x = x.contiguous()          # the stem hands the first block a channels-last image: one copy, here
            return residual_block(x, norm.weight, norm.bias, conv.weight, conv.bias, _keep(block, x), norm.eps, route)
        R.adopt(block, "_az_adopted", forward)
        count += 1
    if count == 0:
        raise ValueError("adopt_blocks found no 64-channel residual block in `hidden`")
    return count


def restore_blocks(net):
    """Undoes `adopt_blocks`: every adopted block runs its class's forward again.  Returns the number restored."""
    return sum(R.restore(block, "_az_adopted") for block in net.hidden.children())
