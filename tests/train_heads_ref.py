"""The reference for the Connect4 heads' training forward and backward (az_train_dev_heads_fwd / _bwd in
include/az_train.h, `heads` in src/train_heads.py): the header's forward formulas restated in float64 (torch autograd runs
their mirror image, and hands back the row-gate and logit gradients the two cancelling sums are measured against); the
float32 torch route on the CPU, written with the module's own ops (the deviation torch itself has from float64, which the
GPU tests' bounds rest on); and the seeded inputs the CPU and the GPU tests share.  Everything is computed once and
cached; callers must not write into what they get.

How a deviation is measured (`deviations`): the largest absolute difference from the restatement over the quantity's
largest magnitude, with two refinements.
  log_p      an illegal entry is about -1e9, where one float32 ulp is 64: over the whole tensor that magnitude would let any
             error on the legal entries pass.  So "log_p" is the legal entries alone, over the largest LEGAL magnitude, and
             "log_p_illegal" is the largest absolute difference on the illegal ones, held to 64 (`ILLEGAL_ABS`).
  d_row_gate_bias, d_policy_out_bias
             sums that cancel (a softmax ignores a shift; an all-legal row's d_logit adds to zero): float64 gives 1e-15
             and any float32 route gives rounding.  Their difference is divided by the float64 sum of the absolute values
             of their terms (sum |ds|, sum |d_logit|: `abs_ds`, `abs_dlogit` of the restatement), not by their own size."""
import functools

import numpy as np

from train_ref_common import FACTOR, FLOOR, bound, dev      # noqa: F401  (the tests reach them through this module)

ROWS, COLS, TOK, CH, CLASSES = 6, 7, 42, 64, 3
EPS = 1e-5
FIELDS = ("policy_norm_weight", "row_gate_weight", "row_gate_bias", "policy_fc_weight", "policy_fc_bias", "policy_out_weight",
          "policy_out_bias", "pool_norm_weight", "pool_fc_weight", "pool_fc_bias", "norm_weight", "fc_weight", "fc_bias",
          "out_norm_weight", "value_out_weight", "value_out_bias", "aux_out_weight", "aux_out_bias")
SHAPES = ((CH,), (1, CH), (1,), (CH, CH), (CH,), (1, CH), (1,), (CH,), (CH, CH), (CH,), (CH,), (CH, CH), (CH,), (CH,),
          (CLASSES, CH), (CLASSES,), (1, CH), (1,))
POLICY, DUAL = FIELDS[:7], FIELDS[7:]
GRADS = tuple("d_" + f for f in FIELDS)
OUTPUTS = ("log_p", "value", "steps")
UPSTREAM = ("d_log_p", "d_value", "d_steps")
QUANTITIES = OUTPUTS + ("d_tokens",) + GRADS
CANCELLING = {"d_row_gate_bias": "abs_ds", "d_policy_out_bias": "abs_dlogit"}
ILLEGAL_ABS = 64.0
GPU_N = (1, 2, 7, 65)
DEFAULT_CAP = 256           # workgroups of the backward when max_workgroups is 0 (csrc/train_heads_kernels.hip)
ROW_FLOATS = 13128          # a partial row: 13126 floats, padded
KEEP_P = 0.2
# inputs(n, case): 0 the standard mask, no keeps (what the reference's own heads with dropout 0 take: fixture G26);
# 1 the standard mask and p = 0.2 keeps; 2 null legal and null keeps; 3 case 1 with row_gate.weight x 20 and out.weight x 50
MASKED, KEPT, PLAIN, SATURATED = 0, 1, 2, 3


def restatement(d):
    """The header's formulas in float64 -> dict of float64 arrays: QUANTITIES, `abs_ds`, `abs_dlogit`, `row_score_max`, and `legal`."""
    import torch
    f64 = torch.float64
    tok = torch.tensor(d["tokens"], dtype=f64, requires_grad=True)
    p = {k: torch.tensor(d[k], dtype=f64, requires_grad=True) for k in FIELDS}
    n = tok.shape[0]
    legal = torch.ones((n, COLS), dtype=torch.bool) if d["legal"] is None else torch.tensor(d["legal"])
    keep_policy = torch.ones((n, COLS, CH), dtype=f64) if d["keep_policy"] is None else torch.tensor(d["keep_policy"], dtype=f64)
    keep_pool = torch.ones((n, CH), dtype=f64) if d["keep_pool"] is None else torch.tensor(d["keep_pool"], dtype=f64)

    def rms(v, w):
        return v * (1.0 / torch.sqrt((v * v).sum(-1, keepdim=True) / CH + EPS)) * w

    def sigmoid(z):
        return 1.0 / (1.0 + torch.exp(-z))

    def log_softmax(z):
        z = z - z.max(-1, keepdim=True).values
        return z - torch.log(torch.exp(z).sum(-1, keepdim=True))

    xn = rms(tok, p["policy_norm_weight"])                                              # [n, 42, 64]
    s = (xn * p["row_gate_weight"][0]).sum(-1) + p["row_gate_bias"][0]                  # [n, 42]
    s.retain_grad()
    grid = s.reshape(n, ROWS, COLS)
    e = torch.exp(grid - grid.max(1, keepdim=True).values)
    w = (e / e.sum(1, keepdim=True)).reshape(n, TOK)
    colf = (w[:, :, None] * xn).reshape(n, ROWS, COLS, CH).sum(1)                       # [n, 7, 64]
    u = colf @ p["policy_fc_weight"].T + p["policy_fc_bias"]
    a = u * sigmoid(u) * keep_policy
    raw = (a * p["policy_out_weight"][0]).sum(-1) + p["policy_out_bias"][0]             # [n, 7]
    raw.retain_grad()
    log_p = log_softmax(torch.where(legal, raw, torch.full_like(raw, -1e9)))
    m = tok.sum(1) / TOK
    z1 = rms(m, p["pool_norm_weight"]) @ p["pool_fc_weight"].T + p["pool_fc_bias"]
    x1 = m + keep_pool * z1 * sigmoid(z1)
    z2 = rms(x1, p["norm_weight"]) @ p["fc_weight"].T + p["fc_bias"]
    h = rms(z2 * sigmoid(z2), p["out_norm_weight"])
    value = log_softmax(h @ p["value_out_weight"].T + p["value_out_bias"])
    steps = sigmoid((h * p["aux_out_weight"][0]).sum(-1) + p["aux_out_bias"][0])
    up = [torch.tensor(d[k], dtype=f64) for k in UPSTREAM]
    torch.autograd.backward([log_p, value, steps], up)
    out = dict(log_p=log_p, value=value, steps=steps, d_tokens=tok.grad, **{"d_" + k: p[k].grad for k in FIELDS})
    out = {k: v.detach().numpy() for k, v in out.items()}
    out["abs_ds"] = float(s.grad.abs().sum())
    out["abs_dlogit"] = float(raw.grad.abs().sum())
    out["row_score_max"] = float(s.detach().max())
    out["legal"] = legal.numpy()
    return out


def module_ops(tokens, legal, params, keep_policy, keep_pool):
    """The two head modules' own ops (az_net._ColumnPolicy, az_net._ValueAux, the reference's heads), hand-assembled, with
    the dropout factors explicit.  Torch tensors in, the three outputs out."""
    import torch
    import torch.nn.functional as F
    (p_norm, gate_w, gate_b, p_fc_w, p_fc_b, out_w, out_b, pool_norm, pool_w, pool_b, norm, fc_w, fc_b, out_norm, val_w, val_b,
     aux_w, aux_b) = params
    n = tokens.shape[0]
    x = F.rms_norm(tokens, (CH,), p_norm, EPS).reshape(n, ROWS, COLS, CH).transpose(1, 2)
    w = torch.softmax(F.linear(x, gate_w, gate_b).squeeze(-1), dim=-1)
    col = F.silu(F.linear((w.unsqueeze(-1) * x).sum(dim=2), p_fc_w, p_fc_b))
    if keep_policy is not None:
        col = col * keep_policy
    logits = F.linear(col, out_w, out_b).squeeze(-1)
    if legal is not None:
        logits = logits.masked_fill(~legal, -1e9)
    m = tokens.mean(dim=1)
    z = F.silu(F.linear(F.rms_norm(m, (CH,), pool_norm, EPS), pool_w, pool_b))
    if keep_pool is not None:
        z = z * keep_pool
    h = F.rms_norm(F.silu(F.linear(F.rms_norm(m + z, (CH,), norm, EPS), fc_w, fc_b)), (CH,), out_norm, EPS)
    return F.log_softmax(logits, dim=-1), F.log_softmax(F.linear(h, val_w, val_b), dim=-1), torch.sigmoid(F.linear(h, aux_w, aux_b).squeeze(-1))


def torch_route(d, dtype=None, fn=None):
    """`fn(tokens, legal, params, keep_policy, keep_pool)` (default: `module_ops`) on the CPU in `dtype` (default float32)
    with autograd -> the QUANTITIES."""
    import torch
    dtype = dtype or torch.float32
    tok = torch.tensor(d["tokens"], dtype=dtype, requires_grad=True)
    params = [torch.tensor(d[k], dtype=dtype, requires_grad=True) for k in FIELDS]
    legal = None if d["legal"] is None else torch.tensor(d["legal"])
    keeps = [None if d[k] is None else torch.tensor(d[k], dtype=dtype) for k in ("keep_policy", "keep_pool")]
    outs = (fn or module_ops)(tok, legal, params, *keeps)
    torch.autograd.backward(list(outs), [torch.tensor(d[k], dtype=dtype) for k in UPSTREAM])
    got = dict(zip(OUTPUTS, (o.detach().numpy() for o in outs)), d_tokens=tok.grad.numpy())
    got.update({"d_" + k: t.grad.numpy() for k, t in zip(FIELDS, params)})
    return got


def deviations(got, ref, quantities=QUANTITIES):
    """Per quantity as the module's docstring says; `ref` is a restatement (it carries `legal`, `abs_ds`, `abs_dlogit`).
    With "log_p" among the quantities the result has "log_p_illegal" too: an absolute figure, to be held to ILLEGAL_ABS."""
    out = {}
    for q in quantities:
        g, r = np.asarray(got[q], np.float64), np.asarray(ref[q], np.float64)
        if q == "log_p":
            legal = ref["legal"]
            out[q] = dev(g[legal], r[legal]) if legal.any() else 0.0
            out["log_p_illegal"] = float(np.abs(g - r)[~legal].max()) if (~legal).any() else 0.0
        elif q in CANCELLING:
            out[q] = float(np.abs(g - r).max() / ref[CANCELLING[q]])
        else:
            out[q] = dev(g, r)
    return out


@functools.lru_cache(maxsize=None)
def inputs(n, case=MASKED):
    """Seeded float32 inputs.  Tokens about N(0, 1.5^2), the last sample's all zero when n >= 2.  Every parameter off its
    default (norm weights round 1, biases off 0, the three output weights - which the reference zeroes - too).  The
    standard mask: sample 0 all legal, sample 1 entirely illegal when n >= 3, the rest Bernoulli(0.7).  The upstream
    gradients are non-zero everywhere, on illegal entries too.  Keeps at p = 0.2: sample 0's column 2 all zero in
    keep_policy, sample n // 2 all zero in keep_pool.  The seed does not depend on the case: the four cases share tokens,
    parameters and gradients."""
    rng = np.random.default_rng(77 + 1000 * n)
    f32 = np.float32
    tokens = (1.5 * rng.standard_normal((n, TOK, CH))).astype(f32)
    if n >= 2:
        tokens[-1] = 0.0
    d = dict(tokens=tokens)
    for k, shape in zip(FIELDS, SHAPES):
        if k.endswith("norm_weight"):
            v = 1.0 + 0.1 * rng.standard_normal(shape)
        elif k.endswith("bias"):
            v = 0.1 * rng.standard_normal(shape)
        elif k in ("policy_out_weight", "value_out_weight", "aux_out_weight"):
            v = 0.1 * rng.standard_normal(shape)
        elif k == "row_gate_weight":
            v = 0.3 * rng.standard_normal(shape)        # row scores of a few units: times 20 they pass what exp takes in float32
        else:
            v = rng.standard_normal(shape) * np.sqrt(2.0 / CH)
        d[k] = v.astype(f32)
    legal = rng.random((n, COLS)) < 0.7
    legal[0] = True
    if n >= 3:
        legal[1] = False
    keep_policy = ((rng.random((n, COLS, CH)) >= KEEP_P) / (1.0 - KEEP_P)).astype(f32)
    keep_pool = ((rng.random((n, CH)) >= KEEP_P) / (1.0 - KEEP_P)).astype(f32)
    keep_policy[0, 2] = 0.0
    keep_pool[n // 2] = 0.0
    d["d_log_p"] = rng.standard_normal((n, COLS)).astype(f32)
    d["d_value"] = rng.standard_normal((n, CLASSES)).astype(f32)
    d["d_steps"] = rng.standard_normal((n,)).astype(f32)
    d["legal"] = None if case == PLAIN else legal
    d["keep_policy"], d["keep_pool"] = (keep_policy, keep_pool) if case in (KEPT, SATURATED) else (None, None)
    if case == SATURATED:
        d["row_gate_weight"] = d["row_gate_weight"] * f32(20.0)
        d["policy_out_weight"] = d["policy_out_weight"] * f32(50.0)
    assert case in (MASKED, KEPT, PLAIN, SATURATED)
    return d


@functools.lru_cache(maxsize=None)
def reference(n, case=MASKED):
    return restatement(inputs(n, case))


@functools.lru_cache(maxsize=None)
def torch_deviations(n, case=MASKED):
    """float32 torch's own deviation from the restatement on `inputs(n, case)`, per quantity (and "log_p_illegal")."""
    return deviations(torch_route(inputs(n, case)), reference(n, case))
