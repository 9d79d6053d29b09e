#!/usr/bin/env python3
"""Generate tests/golden/g25_stem.npz: what the REAL reference's Connect4 `CNN` returns for its stem, forward and backward.

Run in the build container only (needs the reference checkout; CPU, no GPU, no compiled piece):

    python tests/golden/make_golden_stem.py            # AZ_REFERENCE=<checkout> if it is not /root/reference

`CNN` (src/environments/Connect4/Network.py) is imported unmodified from the checkout (its module and NetworkBase alone,
not the packages' compiled environments) and built as `CNN(lr=1e-3, dropout=0.0)` in float32 on the CPU, in training
mode.  Inputs: `inputs(3, 0)` of tests/train_stem_ref.py - three seeded 0/1 boards, the last one empty, both embeddings,
the first convolution's weight and a NON-ZERO bias off their defaults, and a seeded upstream gradient.  The module's own
`_embed_state`, `hidden[0]` and `hidden[1]` run forward, autograd runs them backward.  Stored: the inputs, the four
parameters, `y` and the four gradients - the five quantities the tests hold - plus the module's `orbit_map`.

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
from train_stem_ref import PARAMS, inputs      # noqa: E402


def main():
    # the packages as bare namespaces: their __init__ files pull in the reference's compiled environments, which the
    # network does not need
    for name in ("src", "src.environments", "src.environments.Connect4"):
        pkg = types.ModuleType(name)
        pkg.__path__ = [os.path.join(REF, *name.split("."))]
        sys.modules[name] = pkg
    from src.environments.Connect4.Network import CNN
    d = inputs(3, 0)
    assert not d["state"][-1, :2].any() and d["state"][0, :2].any() and np.abs(d["b"]).max() > 0.05
    net = CNN(lr=1e-3, dropout=0.0, device="cpu").float().train()
    weights = dict(E=net.piece_emb.weight, P=net.pos_emb.weight, W=net.hidden[0].weight, b=net.hidden[0].bias)
    with torch.no_grad():
        for k in PARAMS:
            weights[k].copy_(torch.from_numpy(d[k]))
    y = net.hidden[1](net.hidden[0](net._embed_state(torch.from_numpy(d["state"].copy()))))
    y.backward(torch.from_numpy(d["dy"]))
    out = dict(state=d["state"], dy=d["dy"], orbit_map=net.orbit_map.numpy(), y=y.detach().numpy(),
               **{k: d[k] for k in PARAMS}, **{"d" + k: weights[k].grad.numpy() for k in PARAMS})
    path = os.path.join(HERE, "g25_stem.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
