#!/usr/bin/env python3
"""Generate tests/golden/g24_gated_attention.npz: what the REAL reference's `AttentionBlock` returns, forward and backward.

Run in the build container only (needs the reference checkout; CPU, no GPU, no compiled piece):

    python tests/golden/make_golden_attn.py            # AZ_REFERENCE=<checkout> if it is not /root/reference

`AttentionBlock` (src/environments/Connect4/Network.py) is imported unmodified from the checkout (its module alone, not the
packages' compiled environments) and built as `AttentionBlock(64, 4, 0.0)` in float32, in training mode.  Inputs:
`inputs(3, 0)` of tests/train_attn_ref.py - a seeded x[3, 64, 6, 7] whose last sample is all zero, every weight off its
default and a seeded upstream gradient.  Stored: the inputs, the parameters, `y` and the seven autograd gradients - the
eight quantities the tests hold - plus the norms' eps.

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
from train_attn_ref import PARAMS, inputs      # noqa: E402


def main():
    # the packages as bare namespaces: their __init__ files pull in the reference's compiled environments, which a
    # network block does not need
    for name in ("src", "src.environments", "src.environments.Connect4"):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, *name.split("."))]
        sys.modules[name] = pkg
    from src.environments.Connect4.Network import AttentionBlock as Block
    d = inputs(3, 0)
    assert not d["x"][-1].any() and d["x"][0].any() and d["bits"] is None
    block = Block(64, 4, 0.0).float().train()
    attn = block.attn
    weights = dict(pre=attn.prenorm.weight, Wqkv=attn.qkv_proj.weight, Wg=attn.gate_proj.weight, Wo=attn.o_proj.weight,
                   qn=attn.q_norm.weight, kn=attn.k_norm.weight)
    assert {attn.prenorm.eps, attn.q_norm.eps, attn.k_norm.eps} == {1e-5}
    with torch.no_grad():
        for k in PARAMS:
            weights[k].copy_(torch.from_numpy(d[k]))
    x = torch.from_numpy(d["x"].copy()).requires_grad_(True)
    y = block(x)
    y.backward(torch.from_numpy(d["dy"]))
    out = dict(x=d["x"], dy=d["dy"], eps=np.float64(attn.prenorm.eps), y=y.detach().numpy(), dx=x.grad.numpy(),
               **{k: d[k] for k in PARAMS},
               **{q: weights[k].grad.numpy() for q, k in zip(("d_pre", "d_qkv", "d_gate", "d_o", "d_qn", "d_kn"), PARAMS)})
    path = os.path.join(HERE, "g24_gated_attention.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
