"""The reference for the gated attention block's training forward and backward (az_train_dev_attn_fwd / _bwd in
include/az_train.h, `gated_attention` in src/train_attn.py): the header's formulas restated in float64 with the gradients
from autograd; the float32 torch route on the CPU (the deviation torch itself has from float64, which the GPU tests'
bounds rest on); and the seeded inputs the CPU and the GPU tests share.  Everything is computed once and cached; callers
must not write into what they get."""
import functools

import numpy as np
import torch

from train_ref_common import FACTOR, FLOOR, bound, dev, deviations as plain_deviations      # noqa: F401  (the tests reach them through this module)

CH, HEADS, HD, ROWS, COLS, TOK = 64, 4, 16, 6, 7, 42
EPS = 1e-5
PARAMS = ("pre", "Wqkv", "Wg", "Wo", "qn", "kn")
QUANTITIES = ("y", "dx", "d_pre", "d_qkv", "d_gate", "d_o", "d_qn", "d_kn")
GPU_N = (1, 2, 7, 65)
KEEP_P = 0.2
DEFAULT_CAP = 256           # workgroups of the backward when max_workgroups is 0 (csrc/train_attn_kernels.hip)
LOW = (1 << TOK) - 1


def mask_of(bits, n):
    """[n, 4, 42] words (or None) -> float64 [n, 4, 42, 42]: entry (n, a, i, j) is bit j of word (n, a, i)."""
    if bits is None:
        return np.ones((n, HEADS, TOK, TOK))
    return ((np.asarray(bits).view(np.uint64)[..., None] >> np.arange(TOK, dtype=np.uint64)) & np.uint64(1)).astype(np.float64)


def restatement(x, pre, Wqkv, Wg, Wo, qn, kn, bits, keep_scale, dy, eps=EPS):
    """The header's formulas in float64, head by head -> dict of float64 arrays: QUANTITIES."""
    t = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in
         dict(x=x, pre=pre, Wqkv=Wqkv, Wg=Wg, Wo=Wo, qn=qn, kn=kn).items()}
    n = t["x"].shape[0]
    keep = torch.tensor(mask_of(bits, n)) * float(keep_scale)

    def rms(v, w):
        return v * (1.0 / torch.sqrt((v * v).mean(-1, keepdim=True) + eps)) * w

    tok = t["x"].reshape(n, CH, TOK).permute(0, 2, 1)                  # tok[t][c] = x[c][t]
    h = rms(tok, t["pre"])
    qkv = torch.einsum("oc,ntc->nto", t["Wqkv"], h)
    g = torch.einsum("ac,ntc->nta", t["Wg"], h)
    heads = []
    for a in range(HEADS):
        q, k, v = (qkv[:, :, third * CH + a * HD: third * CH + (a + 1) * HD] for third in range(3))
        qh, kh = rms(q, t["qn"]), rms(k, t["kn"])
        s = 0.25 * torch.einsum("nid,njd->nij", qh, kh)
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        p = e / e.sum(-1, keepdim=True) * keep[:, a]
        heads.append(torch.sigmoid(g[:, :, a:a + 1]) * torch.einsum("nij,njd->nid", p, v))
    y = torch.einsum("ck,nik->nic", t["Wo"], torch.cat(heads, -1)) + tok
    y.backward(torch.tensor(np.asarray(dy, np.float64)))
    out = dict(y=y, dx=t["x"].grad, d_pre=t["pre"].grad, d_qkv=t["Wqkv"].grad, d_gate=t["Wg"].grad, d_o=t["Wo"].grad,
               d_qn=t["qn"].grad, d_kn=t["kn"].grad)
    return {k: v.detach().numpy() for k, v in out.items()}


def _plain_block(x, pre, Wqkv, Wg, Wo, qn, kn, bits, keep_scale, eps):
    """The formula in torch ops of x's dtype (what `gated_attention(route="torch")` must equal)."""
    import torch.nn.functional as F
    n = x.shape[0]

    def rms(v, w):
        return v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps) * w

    tok = x.flatten(2).transpose(1, 2)
    h = rms(tok, pre)
    q, k, v = F.linear(h, Wqkv).view(n, TOK, 3, HEADS, HD).unbind(2)
    g = F.linear(h, Wg)
    q, k = rms(q, qn).transpose(1, 2), rms(k, kn).transpose(1, 2)
    p = torch.softmax((q @ k.transpose(-1, -2)) * 0.25, dim=-1)
    if bits is not None:
        p = p * (torch.tensor(mask_of(bits.numpy(), n)).to(p.dtype) * keep_scale)
    o = (p @ v.transpose(1, 2)) * torch.sigmoid(g.transpose(1, 2).unsqueeze(-1))
    return F.linear(o.transpose(1, 2).reshape(n, TOK, CH), Wo) + tok


def torch_route(x, pre, Wqkv, Wg, Wo, qn, kn, bits, keep_scale, dy, eps=EPS, dtype=torch.float32, block=None):
    """`gated_attention(route="torch")` (`block`, a callable of the same leading arguments) or the plain formula, on the CPU
    in `dtype`."""
    block = block or _plain_block
    t = [torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for v in (x, pre, Wqkv, Wg, Wo, qn, kn)]
    kb = None if bits is None else torch.tensor(np.asarray(bits, np.int64))
    y = block(*t, kb, float(keep_scale), eps)
    y.backward(torch.tensor(np.asarray(dy), dtype=dtype))
    return dict(y=y.detach().numpy(), **{k: v.grad.numpy() for k, v in zip(QUANTITIES[1:], t)})


def deviations(got, ref, quantities=QUANTITIES):
    return plain_deviations(got, ref, quantities)


@functools.lru_cache(maxsize=None)
def inputs(n, keep_p, qk_scale=1.0, seed=24):
    """Seeded float32 inputs: x [n, 64, 6, 7] (its last sample all zero when n > 1), every weight off its default, a seeded
    upstream gradient dy [n, 42, 64], and - for keep_p > 0 - mask words with bits 0 .. 41 Bernoulli(1 - keep_p), garbage in
    bits 42 .. 63 and the words of sample 0's head 1 all zero below bit 42.  `qk_scale` multiplies the two head norms'
    weights (6: logits reach +-160)."""
    rng = np.random.default_rng(seed + 1000 * n + int(100 * keep_p) + int(7 * qk_scale))
    x = rng.standard_normal((n, CH, ROWS, COLS)).astype(np.float32)
    if n > 1:
        x[-1] = 0.0
    pre = (1.0 + 0.3 * rng.standard_normal(CH)).astype(np.float32)
    Wqkv = (rng.standard_normal((3 * CH, CH)) * np.sqrt(2.0 / CH)).astype(np.float32)
    Wg = (rng.standard_normal((HEADS, CH)) * np.sqrt(2.0 / CH)).astype(np.float32)
    Wo = (rng.standard_normal((CH, CH)) * np.sqrt(2.0 / CH)).astype(np.float32)
    qn = ((1.0 + 0.3 * rng.standard_normal(HD)) * qk_scale).astype(np.float32)
    kn = ((1.0 + 0.3 * rng.standard_normal(HD)) * qk_scale).astype(np.float32)
    dy = rng.standard_normal((n, TOK, CH)).astype(np.float32)
    bits, keep_scale = None, 1.0
    if keep_p > 0:
        kept = rng.random((n, HEADS, TOK, TOK)) >= keep_p
        words = (kept.astype(np.uint64) << np.arange(TOK, dtype=np.uint64)).sum(-1, dtype=np.uint64)
        words[0, 1] = 0
        garbage = rng.integers(0, 1 << 22, size=words.shape, dtype=np.uint64) << np.uint64(TOK)
        bits = (words | garbage).view(np.int64)
        keep_scale = float(np.float32(1.0 / (1.0 - keep_p)))
    return dict(x=x, pre=pre, Wqkv=Wqkv, Wg=Wg, Wo=Wo, qn=qn, kn=kn, bits=bits, keep_scale=keep_scale, dy=dy)


def _args(d):
    return (d["x"], d["pre"], d["Wqkv"], d["Wg"], d["Wo"], d["qn"], d["kn"], d["bits"], d["keep_scale"], d["dy"])


@functools.lru_cache(maxsize=None)
def reference(n, keep_p, qk_scale=1.0):
    return restatement(*_args(inputs(n, keep_p, qk_scale)))


@functools.lru_cache(maxsize=None)
def torch_deviations(n, keep_p, qk_scale=1.0):
    """float32 torch's own deviation from the restatement on `inputs(n, keep_p, qk_scale)`, per quantity."""
    return deviations(torch_route(*_args(inputs(n, keep_p, qk_scale))), reference(n, keep_p, qk_scale))
