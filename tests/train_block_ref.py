"""The reference for the residual block's training forward and backward (az_train_dev_block_fwd / _bwd in
include/az_train.h, `residual_block` in src/train_block.py): the header's formulas restated in float64, channel-generic,
with the gradients from autograd; the float32 torch route on the CPU (the deviation torch itself has from float64,
which the GPU tests' bounds rest on); and the seeded inputs the CPU and the GPU tests share.  Everything is computed
once and cached; callers must not write into what they get."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from train_ref_common import FACTOR, FLOOR, bound, dev, deviations as plain_deviations      # noqa: F401  (the tests reach them through this module)

ROWS, COLS = 6, 7
EPS = 1e-5
QUANTITIES = ("y", "dx", "dgamma", "dbeta", "dW", "db")
GPU_N = (1, 2, 7, 65)
KEEP_P = 0.2
DEFAULT_CAP = 256           # workgroups of the backward when max_workgroups is 0 (csrc/train_block_kernels.hip)


def restatement(x, gamma, beta, W, b, keep, dy, eps=EPS):
    """The header's formulas in float64 -> dict of float64 arrays: QUANTITIES, and z, mean, rstd (what the forward saves)."""
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=k != "dy") for k, v in
         dict(x=x, gamma=gamma, beta=beta, W=W, b=b, dy=dy).items()}
    n, c = t["x"].shape[:2]
    kp = torch.ones((n, c), dtype=torch.float64) if keep is None else torch.tensor(np.asarray(keep, np.float64))
    flat = t["x"].reshape(n, -1)
    mean = flat.mean(1)
    var = ((flat - mean[:, None]) ** 2).mean(1)                         # biased
    rstd = 1.0 / torch.sqrt(var + eps)
    xn = (t["x"] - mean[:, None, None, None]) * rstd[:, None, None, None] * t["gamma"][None, :, None, None] + t["beta"][None, :, None, None]
    padded = F.pad(xn, (1, 1, 1, 1))                                     # zeros round the board
    z = t["b"][None, :, None, None].expand(n, -1, ROWS, COLS).clone()
    for ky in range(3):
        for kx in range(3):
            z = z + torch.einsum("oc,ncij->noij", t["W"][:, :, ky, kx], padded[:, :, ky:ky + ROWS, kx:kx + COLS])
    y = t["x"] + kp[:, :, None, None] * z * torch.sigmoid(z)
    y.backward(t["dy"])
    out = dict(y=y, dx=t["x"].grad, dgamma=t["gamma"].grad, dbeta=t["beta"].grad, dW=t["W"].grad, db=t["b"].grad,
               z=z, mean=mean, rstd=rstd)
    return {k: v.detach().numpy() for k, v in out.items()}


def torch_route(x, gamma, beta, W, b, keep, dy, eps=EPS, dtype=torch.float32, block=None):
    """`residual_block(route="torch")` (or `block`, a callable of the same signature) on the CPU in `dtype`."""
    if block is None:
        def block(x, g, be, W, b, keep, eps):
            h = F.silu(F.conv2d(F.group_norm(x, 1, g, be, eps), W, b, padding=1))
            return x + h if keep is None else x + keep[:, :, None, None] * h
    t = [torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for v in (x, gamma, beta, W, b)]
    kp = None if keep is None else torch.tensor(np.asarray(keep), dtype=dtype)
    y = block(*t, kp, eps)
    y.backward(torch.tensor(np.asarray(dy), dtype=dtype))
    names = ("dx", "dgamma", "dbeta", "dW", "db")
    return dict(y=y.detach().numpy(), **{k: v.grad.numpy() for k, v in zip(names, t)})


def deviations(got, ref, quantities=QUANTITIES):
    return plain_deviations(got, ref, quantities)


@functools.lru_cache(maxsize=None)
def inputs(n, channels=64, seed=23, keep_p=KEEP_P, zero_sample=True):
    """Seeded float32 inputs: x (its last sample all zero), gamma, beta off their defaults, a Kaiming-scaled W, b, dy and a
    keep with whole channels at 0 (every sample's channel 0 among them); keep_p = 0 gives keep None."""
    rng = np.random.default_rng(seed + 1000 * n + channels)
    x = rng.standard_normal((n, channels, ROWS, COLS)).astype(np.float32)
    if zero_sample:
        x[-1] = 0.0
    gamma = (1.0 + 0.3 * rng.standard_normal(channels)).astype(np.float32)
    beta = (0.2 * rng.standard_normal(channels)).astype(np.float32)
    W = (rng.standard_normal((channels, channels, 3, 3)) * np.sqrt(2.0 / (9 * channels))).astype(np.float32)
    b = (0.1 * rng.standard_normal(channels)).astype(np.float32)
    dy = rng.standard_normal((n, channels, ROWS, COLS)).astype(np.float32)
    keep = None
    if keep_p > 0:
        keep = ((rng.random((n, channels)) >= keep_p) / (1.0 - keep_p)).astype(np.float32)
        keep[:, 0] = 0.0
    return dict(x=x, gamma=gamma, beta=beta, W=W, b=b, keep=keep, dy=dy)


@functools.lru_cache(maxsize=None)
def padding_inputs(kx):
    """x non-zero only in columns 0 and 6, W non-zero only at the taps with this kx (0 or 2): a tap outside the board
    must contribute exactly nothing, and a row must not wrap into its neighbour.  x is small integers with column 6 the
    negative of column 0, so its mean is exactly 0 in any summation order, and beta is 0: xn is then exactly 0 in
    columns 1 to 5.  dy is non-zero only in the column whose kx-tap falls off the board (0 for kx = 0, 6 for kx = 2), so
    dW is exactly 0 at that tap (it reads outside the board) and at the opposite one (it reads a zero column) - unless
    the kernel wraps into the neighbouring row's column 6 or 0, which is not zero."""
    assert kx in (0, 2)
    d = {k: (None if v is None else v.copy()) for k, v in inputs(2, keep_p=0.0, zero_sample=False).items()}
    rng = np.random.default_rng(77 + kx)
    edge = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0], np.float32), size=d["x"].shape[:3])
    d["x"][:] = 0.0
    d["x"][:, :, :, 0], d["x"][:, :, :, 6] = edge, -edge
    d["beta"][:] = 0.0
    mask = np.zeros((1, 1, 3, 3), np.float32)
    mask[:, :, :, kx] = 1.0
    d["W"] = d["W"] * mask
    col = 0 if kx == 0 else 6
    keep_col = np.zeros((1, 1, 1, COLS), np.float32)
    keep_col[..., col] = 1.0
    d["dy"] = d["dy"] * keep_col
    return d


def _args(d):
    return (d["x"], d["gamma"], d["beta"], d["W"], d["b"], d["keep"], d["dy"])


@functools.lru_cache(maxsize=None)
def reference(n, keep_p=KEEP_P):
    return restatement(*_args(inputs(n, keep_p=keep_p)))


@functools.lru_cache(maxsize=None)
def torch_deviations(n, keep_p=KEEP_P):
    """float32 torch's own deviation from the restatement on `inputs(n)`, per quantity."""
    return deviations(torch_route(*_args(inputs(n, keep_p=keep_p))), reference(n, keep_p))


@functools.lru_cache(maxsize=None)
def padding_reference(kx):
    d = padding_inputs(kx)
    return restatement(*_args(d)), deviations(torch_route(*_args(d)), restatement(*_args(d)))
