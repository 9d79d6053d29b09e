#!/usr/bin/env python3
"""Generate tests/golden/g18_training_loss.npz: what the REAL reference's loss code returns on the two batches of
fixture G16 for seeded head outputs, under four settings of its knobs.

Run in the build container only (needs the reference checkout and scikit-learn; CPU, no GPU, no compiled piece):

    python tests/golden/make_golden_loss.py            # AZ_REFERENCE=<checkout> if it is not /root/reference

`Base` (src/environments/NetworkBase.py) is imported unmodified from the checkout by file path and subclassed by a
probe that owns nothing but a dummy parameter, an SGD over it with learning rate 0 (so that `_optimize_batch` can
run as it stands) and a `forward` that hands back the seeded head outputs.  Per game (G16's 128 Connect4 and 192
Othello rows: end states, both turn signs, td rows, must-pass rows) and per config the script calls the
reference's own methods:

    _prepare_training_batch(batch, identity)     -> value_class, turn_sign, policy_mask
    _optimize_batch(model, batch_data, ...)      -> the three losses; autograd's gradients of their sum sit in the
                                                    head tensors' .grad afterwards
    _td_consistency_loss(...)                    -> only to count: the TD rows are recounted from its mask rule
    _final_train_metrics(batch_data, log_p)      -> entropy and sklearn's macro F1

Head outputs (recorded too): `seeded_heads` of tests/train_loss_ref.py - logits masked by the batch's valid_mask
at -1e9 before the log-softmax, a value head without argmax ties (asserted there).  Everything is float32, as the
reference computes it.  The four configs are `CONFIGS` of tests/train_loss_ref.py; the script asserts the TD row
counts 70 / 160, 90 / 168 and 0 / 64 that the tests rely on, and that config (d) on Connect4 takes the reference's
`None` branch.  Also recorded: sklearn's macro F1 for a few hand-made confusion matrices, one with an empty class.

Nothing from the reference is copied: the committed output is data.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AZ_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))
from train_loss_ref import CONFIGS, OFFSET, TENSORS, seeded_heads      # noqa: E402

TD_ROWS = {("b", "c4"): 70, ("b", "ot"): 160, ("c", "c4"): 90, ("c", "ot"): 168, ("d", "c4"): 0, ("d", "ot"): 64}
F1_CASES = np.array([
    [[5, 1, 0], [2, 7, 1], [0, 3, 9]],
    [[4, 0, 0], [0, 6, 0], [0, 0, 0]],          # class 2 neither true nor predicted: left out of the mean
    [[3, 0, 2], [1, 5, 0], [0, 0, 0]],          # class 2 predicted but never true: counts with 0
    [[0, 0, 0], [0, 9, 0], [0, 0, 0]],
    [[0, 4, 0], [0, 0, 4], [4, 0, 0]],          # nothing right
], np.int64)


def load_by_path(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    from sklearn.metrics import f1_score
    Base = load_by_path("ref_network_base", "src", "environments", "NetworkBase.py").Base

    class Probe(Base):
        def __init__(self, offset, heads):
            super().__init__()
            self.aux_target_offset = offset
            self.dummy = torch.nn.Parameter(torch.zeros(1))
            self.opt = torch.optim.SGD([self.dummy], lr=0.0)
            self.heads = heads

        def forward(self, state, action_mask=None):
            return self.heads

    g = np.load(os.path.join(HERE, "g16_training_batch.npz"))
    out = {}
    for key in ("c4", "ot"):
        batch = tuple(torch.from_numpy(g[f"{key}_{t}"]) for t in TENSORS)
        log_p, value, steps = seeded_heads(key, [x.numpy() for x in batch], 18)
        out[f"{key}_log_p"], out[f"{key}_value"], out[f"{key}_steps"] = log_p, value, steps
        for name, cfg in CONFIGS.items():
            heads = tuple(torch.from_numpy(x.copy()).requires_grad_(True) for x in (log_p, value, steps))
            probe = Probe(int(OFFSET[key]), heads)
            data = probe._prepare_training_batch(batch, lambda b: b)
            use_soft = cfg["value_decay"] < 1.0 or cfg["distill_alpha"] > 0
            p_loss, v_loss, aux_loss, last_log_p, _ = probe._optimize_batch(
                probe, data, use_soft, cfg["value_decay"], cfg["distill_alpha"], cfg["distill_temp"], cfg["psw_beta"],
                cfg["entropy_lambda"], cfg["td_alpha"], cfg["td_steps"])
            rel = Base._root_wdl_to_relative(data["future_root_wdl"], data["turn_sign"])
            td_rows = int(((data["steps_to_end"].view(-1) > cfg["td_steps"]) & (rel.sum(1) > 0)).sum()) if cfg["td_alpha"] > 0 else 0
            if cfg["td_alpha"] > 0:
                assert td_rows == TD_ROWS[(name, key)], (name, key, td_rows)
                td = Base._td_consistency_loss(heads[1].detach(), data, cfg["td_steps"], cfg["value_decay"])
                assert (td is None) == (td_rows == 0)
            entropy, f1 = probe._final_train_metrics(data, last_log_p.detach())
            k = f"{key}_{name}_"
            out[k + "losses"] = np.array([p_loss.item(), v_loss.item(), aux_loss.item()], np.float32)
            out[k + "d_log_p"], out[k + "d_value"], out[k + "d_steps"] = (h.grad.numpy().copy() for h in heads)
            out[k + "entropy"] = np.array([entropy], np.float32)
            out[k + "f1"] = np.array([f1], np.float64)
            out[k + "td_rows"] = np.array([td_rows], np.int64)
            if name == "a":
                out[f"{key}_value_class"] = data["value_class"].numpy().copy()
                out[f"{key}_turn_sign"] = data["turn_sign"].numpy().copy()
                out[f"{key}_policy_mask"] = data["policy_mask"].numpy().copy()
            print(k, out[k + "losses"], entropy, f1, td_rows)
    out["f1_cases"] = F1_CASES
    scores = []
    for conf in F1_CASES:
        true = np.repeat(np.arange(3), conf.sum(1))
        pred = np.concatenate([np.repeat(np.arange(3), row) for row in conf])
        scores.append(f1_score(true, pred, average="macro"))
    out["f1_scores"] = np.array(scores, np.float64)
    path = os.path.join(HERE, "g18_training_loss.npz")
    np.savez_compressed(path, **out)
    print(f"g18_training_loss.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
