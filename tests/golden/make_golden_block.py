#!/usr/bin/env python3
"""Generate tests/golden/g23_res_block.npz: what the REAL reference's `ResidualBlock` returns, forward and backward.

Run in the build container only (needs the reference checkout; CPU, no GPU, no compiled piece):

    python tests/golden/make_golden_block.py            # AZ_REFERENCE=<checkout> if it is not /root/reference

`ResidualBlock` (src/environments/Connect4/Network.py) is imported unmodified from the checkout (its module alone, not the
packages' compiled environments) and built as
`ResidualBlock(16, 16, dropout=0.0)` in float32.  Sixteen channels keep the file small; the restatement of
tests/train_block_ref.py is channel-generic, and the kernels are held to the restatement.  Inputs: `inputs(3, channels=16,
keep_p=0)` of tests/train_block_ref.py - a seeded x[3, 16, 6, 7] whose last sample is all zero, gamma and beta off their
defaults, a Kaiming-scaled conv weight, a bias and a seeded upstream gradient.  Stored: the inputs, the parameters, `y`
and the five autograd gradients (x, norm weight and bias, conv weight and bias): the six quantities the tests hold -
plus the GroupNorm's eps.

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
from train_block_ref import inputs      # noqa: E402


def main():
    # the packages as bare namespaces: their __init__ files pull in the reference's compiled environments, which a
    # network block does not need
    for name in ("src", "src.environments", "src.environments.Connect4"):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, *name.split("."))]
        sys.modules[name] = pkg
    from src.environments.Connect4.Network import ResidualBlock as Block
    d = inputs(3, channels=16, keep_p=0.0)
    assert not d["x"][-1].any() and d["x"][0].any() and d["keep"] is None
    block = Block(16, 16, dropout=0.0).float().train()
    with torch.no_grad():
        block.norm.weight.copy_(torch.from_numpy(d["gamma"]))
        block.norm.bias.copy_(torch.from_numpy(d["beta"]))
        block.conv.weight.copy_(torch.from_numpy(d["W"]))
        block.conv.bias.copy_(torch.from_numpy(d["b"]))
    x = torch.from_numpy(d["x"].copy()).requires_grad_(True)
    y = block(x)
    y.backward(torch.from_numpy(d["dy"]))
    out = dict(x=d["x"], gamma=d["gamma"], beta=d["beta"], W=d["W"], b=d["b"], dy=d["dy"], eps=np.float64(block.norm.eps),
               y=y.detach().numpy(), dx=x.grad.numpy(), dgamma=block.norm.weight.grad.numpy(), dbeta=block.norm.bias.grad.numpy(),
               dW=block.conv.weight.grad.numpy(), db=block.conv.bias.grad.numpy())
    path = os.path.join(HERE, "g23_res_block.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
