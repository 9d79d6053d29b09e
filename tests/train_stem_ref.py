"""The reference for the Connect4 stem's training forward and backward (az_train_dev_stem_fwd / _bwd in
include/az_train.h, `stem` in src/train_stem.py): the header's DIRECT formulas - the embedded image t, the 288-term
convolution, dz, the five sums - restated in float64 numpy, with none of the kernels' factoring; the float32 torch route
on the CPU (the deviation torch itself has from float64, which the GPU tests' bounds rest on); and the seeded inputs the
CPU and the GPU tests share.  Everything is computed once and cached; callers must not write into what they get."""
import functools

import numpy as np

from train_ref_common import FACTOR, FLOOR, bound, dev, deviations as plain_deviations      # noqa: F401  (the tests reach them through this module)

ROWS, COLS, CELLS = 6, 7, 42
EMBED, CH, ORBITS = 32, 64, 24
PARAMS = ("E", "P", "W", "b")
QUANTITIES = ("y", "dW", "db", "dE", "dP")
GPU_N = (1, 2, 7, 65)
DEFAULT_CAP = 256           # workgroups of the backward when max_workgroups is 0 (csrc/train_stem_kernels.hip)
ORBIT = np.array([4 * (cell // COLS) + min(cell % COLS, COLS - 1 - cell % COLS) for cell in range(CELLS)])


def restatement(state, E, P, W, b, dy):
    """The header's direct formulas in float64 -> dict of float64 arrays: QUANTITIES, and t, z, dz, dt."""
    state, E, P, W, b, dy = (np.asarray(v, np.float64) for v in (state, E, P, W, b, dy))
    n = state.shape[0]
    own, opp = state[:, 0].reshape(n, CELLS), state[:, 1].reshape(n, CELLS)
    t = (own[:, None, :] * E[0][None, :, None] + opp[:, None, :] * E[1][None, :, None]) + P[ORBIT].T[None]     # [n, 32, 42]
    padded = np.zeros((n, EMBED, ROWS + 2, COLS + 2))
    padded[:, :, 1:-1, 1:-1] = t.reshape(n, EMBED, ROWS, COLS)
    z = np.broadcast_to(b[None, :, None, None], (n, CH, ROWS, COLS)).copy()
    for ky in range(3):
        for kx in range(3):
            z += np.einsum("oc,ncij->noij", W[:, :, ky, kx], padded[:, :, ky:ky + ROWS, kx:kx + COLS])
    s = 1.0 / (1.0 + np.exp(-z))
    y = z * s
    dz = dy * (s + z * s * (1.0 - s))
    dW = np.zeros_like(W)
    dtp = np.zeros_like(padded)
    for ky in range(3):
        for kx in range(3):
            dW[:, :, ky, kx] = np.einsum("noij,ncij->oc", dz, padded[:, :, ky:ky + ROWS, kx:kx + COLS])
            dtp[:, :, ky:ky + ROWS, kx:kx + COLS] += np.einsum("noij,oc->ncij", dz, W[:, :, ky, kx])
    dt = dtp[:, :, 1:-1, 1:-1].reshape(n, EMBED, CELLS)
    dE = np.stack([np.einsum("nk,nck->c", own, dt), np.einsum("nk,nck->c", opp, dt)])
    per_cell = dt.sum(0)                                                # [32, 42]
    dP = np.zeros_like(P)
    for cell in range(CELLS):
        dP[ORBIT[cell]] += per_cell[:, cell]
    return dict(y=y, dW=dW, db=dz.sum((0, 2, 3)), dE=dE, dP=dP, t=t.reshape(n, EMBED, ROWS, COLS), z=z, dz=dz, dt=dt)


def module_ops(state, E, P, W, b):
    """The module's own ops, hand-assembled: the embedding expression of az_net.Connect4Net.embed, the convolution, the
    SiLU.  Torch tensors in, y out."""
    import torch
    import torch.nn.functional as F
    n = state.size(0)
    own = state[:, 0].reshape(n, CELLS, 1)
    opp = state[:, 1].reshape(n, CELLS, 1)
    x = own * E[0] + opp * E[1] + F.embedding(torch.as_tensor(ORBIT), P)
    return F.silu(F.conv2d(x.transpose(1, 2).reshape(n, EMBED, ROWS, COLS), W, b, padding=1))


def torch_route(state, E, P, W, b, dy, dtype=None, fn=None):
    """`fn(state, E, P, W, b)` (default: `module_ops`) on the CPU in `dtype` (default float32) -> the five quantities."""
    import torch
    dtype = dtype or torch.float32
    t = [torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for v in (E, P, W, b)]
    y = (fn or module_ops)(torch.tensor(np.asarray(state), dtype=dtype), *t)
    y.backward(torch.tensor(np.asarray(dy), dtype=dtype))
    return dict(y=y.detach().numpy(), **{k: v.grad.numpy() for k, v in zip(("dE", "dP", "dW", "db"), t)})


def deviations(got, ref, quantities=QUANTITIES):
    return plain_deviations(got, ref, quantities)


@functools.lru_cache(maxsize=None)
def inputs(n, seed=0):
    """Seeded float32 inputs: 0/1 boards (no cell on both planes; the last sample of a batch of two or more is an empty
    board; plane 2 is the side-to-move plane, all ones or all zeros), orthogonal embeddings plus noise, a Kaiming-scaled
    W, a bias off zero and a seeded upstream gradient."""
    rng = np.random.default_rng(31 + 1000 * n + seed)
    stone = rng.integers(0, 3, size=(n, ROWS, COLS))                    # 0 empty, 1 own, 2 opponent
    state = np.zeros((n, 3, ROWS, COLS), np.float32)
    state[:, 0], state[:, 1] = stone == 1, stone == 2
    state[:, 2] = rng.integers(0, 2, size=(n, 1, 1))
    if n > 1:
        state[-1, :2] = 0.0

    def orthogonal(rows):
        q, _ = np.linalg.qr(rng.standard_normal((EMBED, EMBED)))
        return (q[:rows] + 0.05 * rng.standard_normal((rows, EMBED))).astype(np.float32)
    E, P = orthogonal(2), orthogonal(ORBITS)
    W = (rng.standard_normal((CH, EMBED, 3, 3)) * np.sqrt(2.0 / (9 * EMBED))).astype(np.float32)
    b = (0.1 * rng.standard_normal(CH)).astype(np.float32)
    dy = rng.standard_normal((n, CH, ROWS, COLS)).astype(np.float32)
    return dict(state=state, E=E, P=P, W=W, b=b, dy=dy)


def args(d):
    return (d["state"], d["E"], d["P"], d["W"], d["b"], d["dy"])


@functools.lru_cache(maxsize=None)
def multiplier_inputs():
    """`inputs(7)` with planes that are not 0/1: sample 0 holds 0.5 and -2 on both planes, and one cell of sample 1 has
    both planes at 1."""
    d = {k: v.copy() for k, v in inputs(7).items()}
    d["state"][0, 0] *= 0.5
    d["state"][0, 1] *= -2.0
    d["state"][0, 0, 2, 3], d["state"][0, 1, 2, 3] = -2.0, 0.5
    d["state"][1, 0, 0, 0] = d["state"][1, 1, 0, 0] = 1.0
    return d


@functools.lru_cache(maxsize=None)
def padding_inputs(which):
    """`inputs(2, 1)` with stones on columns 0 and 6 only - so a row that wraps into its neighbour shows - no empty sample,
    and the upstream gradient non-zero only on column 0 ("col0"), column 6 ("col6") or row 0 ("row0"): the weight gradient
    at the taps that would read outside the board from there (kx = 0, kx = 2, ky = 0) is exactly zero.  "plane1": the
    whole gradient, but no opponent stone anywhere: d_piece_emb[1] is exactly zero."""
    d = {k: v.copy() for k, v in inputs(2, 1).items()}
    rng = np.random.default_rng(5)
    stone = rng.integers(1, 3, size=(2, ROWS, 2))
    d["state"][:, :2] = 0.0
    for j, col in enumerate((0, COLS - 1)):
        d["state"][:, 0, :, col], d["state"][:, 1, :, col] = stone[:, :, j] == 1, stone[:, :, j] == 2
    keep = np.zeros((1, 1, ROWS, COLS), np.float32)
    if which == "col0":
        keep[..., 0] = 1.0
    elif which == "col6":
        keep[..., COLS - 1] = 1.0
    elif which == "row0":
        keep[..., 0, :] = 1.0
    else:
        assert which == "plane1"
        keep[:] = 1.0
        d["state"][:, 0] += d["state"][:, 1]
        d["state"][:, 1] = 0.0
    d["dy"] = d["dy"] * keep
    return d


def exact_zeros(which, got):
    """The part of the gradients that `padding_inputs(which)` makes exactly zero, and the rest of the same gradient."""
    if which == "col0":
        return got["dW"][:, :, :, 0], got["dW"][:, :, :, 1:]
    if which == "col6":
        return got["dW"][:, :, :, 2], got["dW"][:, :, :, :2]
    if which == "row0":
        return got["dW"][:, :, 0, :], got["dW"][:, :, 1:, :]
    return got["dE"][1], got["dE"][0]


@functools.lru_cache(maxsize=None)
def reference(n, seed=0):
    return restatement(*args(inputs(n, seed)))


@functools.lru_cache(maxsize=None)
def torch_deviations(n, seed=0):
    """float32 torch's own deviation from the restatement on `inputs(n, seed)`, per quantity."""
    return deviations(torch_route(*args(inputs(n, seed))), reference(n, seed))


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(restatement, float32 torch's deviations) of `multiplier_inputs()` ("multipliers") or `padding_inputs(name)`."""
    d = multiplier_inputs() if name == "multipliers" else padding_inputs(name)
    ref = restatement(*args(d))
    return ref, deviations(torch_route(*args(d)), ref)
