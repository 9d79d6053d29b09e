#!/usr/bin/env python3
"""Generate tests/golden/g26_heads.npz: what the REAL reference's Connect4 heads return, forward and backward.

Run in the build container only (needs the reference checkout; CPU, no GPU, no compiled piece):

    python tests/golden/make_golden_heads.py            # AZ_REFERENCE=<checkout> if it is not /root/reference

`ColumnPolicyHead` and `DualHead` (src/environments/Connect4/Network.py) are imported unmodified from the checkout (their
module and NetworkBase alone, not the packages' compiled environments) and built as `ColumnPolicyHead(64, 0.0)` and
`DualHead(64, 3, 0.0)` in float32 on the CPU, in training mode.  Inputs: `inputs(3, 0)` of tests/train_heads_ref.py - three
seeded token grids (the last one all zero), the standard mask (sample 0 all legal, sample 1 entirely illegal), all eighteen
parameters off their defaults and seeded upstream gradients that are non-zero on illegal entries too.  The modules' own
forwards run, autograd runs them backward.  Stored: the inputs, the parameters, the three outputs, d_tokens and the
eighteen gradients - the quantities the tests hold.

Nothing from the reference is copied: the committed output is data.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AZ_REFERENCE", "/root/reference")
sys.path[:0] = [REF, os.path.dirname(HERE)]
from train_heads_ref import DUAL, FIELDS, MASKED, OUTPUTS, POLICY, UPSTREAM, inputs      # noqa: E402

# the reference's attribute of each field of az_train_heads_params, in its order
POLICY_ATTRS = ("norm.weight", "row_gate.weight", "row_gate.bias", "fc.weight", "fc.bias", "out.weight", "out.bias")
DUAL_ATTRS = ("pool_norm.weight", "pool_fc.weight", "pool_fc.bias", "norm.weight", "fc.weight", "fc.bias", "out_norm.weight",
              "value_out.weight", "value_out.bias", "aux_out.weight", "aux_out.bias")


def attr(module, path):
    for part in path.split("."):
        module = getattr(module, part)
    return module


def main():
    # the packages as bare namespaces: their __init__ files pull in the reference's compiled environments, which the
    # network does not need
    for name in ("src", "src.environments", "src.environments.Connect4"):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, *name.split("."))]
        sys.modules[name] = pkg
    from src.environments.Connect4.Network import ColumnPolicyHead, DualHead
    d = inputs(3, MASKED)
    assert d["legal"][0].all() and not d["legal"][1].any() and not d["tokens"][-1].any() and d["keep_policy"] is None
    policy, dual = ColumnPolicyHead(64, 0.0).float().train(), DualHead(64, 3, 0.0).float().train()
    weights = {k: attr(policy, a) for k, a in zip(POLICY, POLICY_ATTRS)}
    weights.update({k: attr(dual, a) for k, a in zip(DUAL, DUAL_ATTRS)})
    with torch.no_grad():
        for k in FIELDS:
            weights[k].copy_(torch.from_numpy(d[k]))
    tokens = torch.from_numpy(d["tokens"].copy()).requires_grad_(True)
    log_p = policy(tokens, torch.from_numpy(d["legal"]))
    value, steps = dual(tokens)
    torch.autograd.backward([log_p, value, steps], [torch.from_numpy(d[k]) for k in UPSTREAM])
    out = dict(tokens=d["tokens"], legal=d["legal"], **{k: d[k] for k in FIELDS + UPSTREAM},
               **dict(zip(OUTPUTS, (t.detach().numpy() for t in (log_p, value, steps)))), d_tokens=tokens.grad.numpy(),
               **{"d_" + k: weights[k].grad.numpy() for k in FIELDS})
    path = os.path.join(HERE, "g26_heads.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
