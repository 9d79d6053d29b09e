"""Float64 restatement of the training losses (include/az_train.h, section "Per sample"), next to othello_ref.py.

Every input is lifted to float64 before the first operation, the terms are written out element by element (no
library loss function), and the gradients come from autograd over those float64 operations.  This is what the
float32 routes of src/train_loss.py - the kernels and the plain-torch route - are measured against; it shares no
code with them.

    reference(heads, batch, offset, cfg, upstream=(1, 1, 1)) -> dict with
        policy, value, aux, entropy             float
        d_log_p, d_value, d_steps               float64 arrays: gradients of u_p policy + u_v value + u_a aux
        confusion [3, 3], policy_rows, td_rows  integers
        value_class, turn_sign, policy_mask     per row
"""
import numpy as np
import torch

CONFIGS = {
    "a": dict(value_decay=1.0, distill_alpha=0.0, distill_temp=1.0, psw_beta=0.0, entropy_lambda=0.0, td_alpha=0.0, td_steps=5),
    "b": dict(value_decay=0.98, distill_alpha=0.3, distill_temp=2.0, psw_beta=0.3, entropy_lambda=0.01, td_alpha=0.25, td_steps=5),
    "c": dict(value_decay=1.0, distill_alpha=0.5, distill_temp=1.0, psw_beta=0.3, entropy_lambda=0.01, td_alpha=0.5, td_steps=3),
    "d": dict(value_decay=0.95, distill_alpha=0.0, distill_temp=1.0, psw_beta=0.0, entropy_lambda=0.05, td_alpha=1.0, td_steps=40),
}
OFFSET = {"c4": 42.0, "ot": 64.0}
TENSORS = ("state", "prob", "winner", "steps_to_end", "aux_target", "root_wdl", "valid_mask", "future_root_wdl")


def _f64(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float64))


def _plogq(t, log_q):
    """sum over the last axis of t (log t - log_q), entries with t == 0 contributing exactly 0."""
    safe = torch.where(t > 0, t, torch.ones_like(t))
    return torch.where(t > 0, t * (safe.log() - log_q), torch.zeros_like(t)).sum(-1)


def _to_mover(wdl, sign):
    swap = (sign < 0).unsqueeze(1)
    return torch.cat([wdl[:, 0:1], torch.where(swap, wdl[:, 2:3], wdl[:, 1:2]), torch.where(swap, wdl[:, 1:2], wdl[:, 2:3])], 1)


def reference(log_p, value, steps, batch, offset, cfg, upstream=(1.0, 1.0, 1.0)):
    b = {t: np.asarray(x) for t, x in zip(TENSORS, batch)}
    N = b["prob"].shape[0]
    lp = _f64(log_p).requires_grad_(True)
    v = _f64(value).requires_grad_(True)
    s = _f64(np.asarray(steps).reshape(-1)).requires_grad_(True)
    prob = _f64(b["prob"])
    sign = torch.where(_f64(b["state"][:, 2, 0, 0]) >= 0, 1, -1)
    win = torch.as_tensor(b["winner"].reshape(-1).astype(np.int64))
    cls = torch.where(win == 0, 0, torch.where(win == sign, 1, 2))
    to_end = _f64(b["steps_to_end"].reshape(-1))
    mask = (prob.sum(1) > 0).double()
    onehot = torch.zeros(N, 3, dtype=torch.float64)
    onehot[torch.arange(N), cls] = 1.0

    # policy
    kl = _plogq(prob, lp)
    w = 1.0 + cfg["psw_beta"] * kl.detach() if cfg["psw_beta"] > 0 else torch.ones_like(kl)
    p = lp.exp()
    H = -torch.where(p > 0, p * lp, torch.zeros_like(p)).sum(1)
    policy = (mask * w * kl).sum() / N
    if cfg["entropy_lambda"] > 0:
        policy = policy - cfg["entropy_lambda"] * (mask * H).sum() / N

    # value
    z = onehot
    if cfg["value_decay"] < 1:
        d = (cfg["value_decay"] ** to_end).unsqueeze(1)
        z = d * onehot + (1 - d) / 3
    val = -(z * v).sum() / N
    if cfg["distill_alpha"] > 0:
        T = cfg["distill_temp"]
        rel = _to_mover(_f64(b["root_wdl"]), sign)
        tl = rel.clamp(min=1e-8).log() / T
        teacher = (tl - tl.logsumexp(1, keepdim=True)).exp()
        student = v / T - (v / T).logsumexp(1, keepdim=True)
        dist = ((rel.sum(1) > 0).double() * _plogq(teacher, student)).sum() / N * T * T
        val = (1 - cfg["distill_alpha"]) * val + cfg["distill_alpha"] * dist
    td_rows = 0
    if cfg["td_alpha"] > 0:
        rel = _to_mover(_f64(b["future_root_wdl"]), sign)
        mass = rel.sum(1)
        counted = (to_end > cfg["td_steps"]) & (mass > 0)
        td_rows = int(counted.sum())
        if td_rows > 0:
            t = rel / mass.clamp(min=1e-8).unsqueeze(1)
            if cfg["value_decay"] < 1:
                keep = cfg["value_decay"] ** cfg["td_steps"]
                t = keep * t + (1 - keep) / 3
            td = _plogq(t, v)[counted].sum() / td_rows
            val = (1 - cfg["td_alpha"]) * val + cfg["td_alpha"] * td

    # aux: smooth-L1 with beta 1
    diff = s - _f64(b["aux_target"].reshape(-1)) / offset
    aux = torch.where(diff.abs() < 1, 0.5 * diff * diff, diff.abs() - 0.5).sum() / N

    (upstream[0] * policy + upstream[1] * val + upstream[2] * aux).backward()
    pred = v.detach().argmax(1)
    conf = np.zeros((3, 3), np.int64)
    np.add.at(conf, (cls.numpy(), pred.numpy()), 1)
    zeros = lambda x: torch.zeros_like(x) if x.grad is None else x.grad
    return dict(policy=float(policy.detach()), value=float(val.detach()), aux=float(aux.detach()), entropy=float(H.detach().sum() / N),
                d_log_p=zeros(lp).numpy(), d_value=zeros(v).numpy(), d_steps=zeros(s).numpy(),
                confusion=conf, policy_rows=int(mask.sum()), td_rows=td_rows,
                value_class=cls.numpy(), turn_sign=sign.numpy(), policy_mask=mask.numpy())


def macro_f1(conf):
    """sklearn's f1_score(average='macro') from a confusion matrix: classes absent from both sides are left out."""
    conf = np.asarray(conf, np.float64).reshape(3, 3)
    scores = []
    for k in range(3):
        tp, fp, fn = conf[k, k], conf[:, k].sum() - conf[k, k], conf[k].sum() - conf[k, k]
        if tp + fp + fn > 0:
            scores.append(2 * tp / (2 * tp + fp + fn))
    return float(np.mean(scores)) if scores else 0.0


def seeded_heads(key, batch, seed):
    """Head outputs for a batch, float32: logits from a seeded generator, masked by valid_mask at -1e9, through
    float64 log-softmax; a value head whose argmax has no ties; steps in (0, 1)."""
    b = {t: np.asarray(x) for t, x in zip(TENSORS, batch)}
    N, A = b["prob"].shape
    rng = np.random.default_rng([seed, 0 if key == "c4" else 1, N])
    logits = rng.normal(0.0, 1.5, (N, A))
    logits = np.where(b["valid_mask"].astype(bool), logits, -1e9)
    log_p = torch.log_softmax(torch.from_numpy(logits), 1).numpy().astype(np.float32)
    value = torch.log_softmax(torch.from_numpy(rng.normal(0.0, 1.0, (N, 3))), 1).numpy().astype(np.float32)
    top = np.sort(value, 1)
    assert (top[:, 2] > top[:, 1]).all(), "a tie in the argmax of value"
    # a few rows beyond the smooth-L1 knee, so that both branches are exercised
    steps = rng.uniform(0.0, 1.0, N).astype(np.float32)
    steps[::7] += np.float32(2.5)
    return log_p, value, steps
