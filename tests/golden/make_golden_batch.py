#!/usr/bin/env python3
"""Generate tests/golden/g16_training_batch.npz: what the REAL reference hands its training step for chosen rows of
the buffers of fixture G15, and the sizes its `sample` gives.

Run in the build container only (needs the reference checkout; CPU, no GPU, no compiled piece):

    python tests/golden/make_golden_batch.py            # AZ_REFERENCE=<checkout> if it is not /root/reference

Rows.  G15's Connect4 and Othello tensors are copied into the reference's own `ReplayBuffer` (`_ptr` set), the
rows `idx` are fetched with its `get` (src/ReplayBuffer.py:125-128) and passed through the game's own `augment`
(src/environments/Connect4/utils.py:50-67, src/environments/Othello/utils.py:65-91), all imported unmodified from
the checkout by file path.  The two utils.py import numba for helpers this script never calls, and numba is not
installed here: a stand-in module named `numba` whose `njit` hands the function back is registered first (the
stand-in is this script's own code).  Stored per game: `idx` and the eight arrays `augment` returned.

`idx` (64 rows of Connect4, 48 of Othello) is a seeded draw with chosen rows put in front, and the script asserts
that it holds: ring slots 0 and capacity - 1, a repeated index, end-state rows (prob all zero, mask all ones), rows
of both turn signs, a row with a non-zero future_root_wdl and, for Othello, a row whose mask has the pass bit set
(a position where the mover must pass - not an end state, whose mask is all ones).

Sizes.  `sample_cases`: (len, capacity, replay_ratio, batch_size, full_batches) -> (len(loader.dataset),
len(loader)) read off the reference's `sample` (ReplayBuffer.py:130-145) on a Connect4-shaped buffer with `_ptr`
set to `len`: both branches of the size rule (len <= 10000, len at and just over 10000 / ratio, far over), ratios
0.25 and 0.025, both `full_batches` values, a batch larger than the sample.  The reference's `state` / `prob`
start uninitialised: only the sizes are recorded.

Nothing from the reference is copied: the committed output is data.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AZ_REFERENCE", "/root/reference")
TENSORS = ("state", "prob", "winner", "steps_to_end", "aux_target", "root_wdl", "valid_mask", "future_root_wdl")
GAMES = {"c4": ("Connect4", (7, 6, 7), 64), "ot": ("Othello", (65, 8, 8), 48)}
SAMPLE_CASES = [(length, capacity, ratio, batch, full)
                for length, capacity, ratio in ((100, 389, 0.25), (10000, 10000, 0.25), (40000, 50000, 0.25), (40001, 50000, 0.25),
                                                (50000, 50000, 0.25), (12345, 500000, 0.025), (400000, 500000, 0.025),
                                                (400001, 500000, 0.025), (500000, 500000, 0.025))
                for batch in (512, 4096, 100)
                for full in (False, True)]


def load_by_path(name, *parts):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, *parts))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def numba_stand_in():
    def njit(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]
        return lambda f: f
    mod = types.ModuleType("numba")
    mod.njit = njit
    sys.modules.setdefault("numba", mod)


def choose_rows(key, g, n_rows, rng):
    cap = int(g[f"{key}_capacity"][0])
    prob, mask, fut, state = (g[f"{key}_{t}"] for t in ("prob", "valid_mask", "future_root_wdl", "state"))
    end = np.flatnonzero((prob == 0).all(1) & mask.all(1))
    turn = state[:, 2, 0, 0]
    with_future = np.flatnonzero((fut != 0).any(1))
    front = [0, cap - 1, int(end[0]), int(end[-1]), int(np.flatnonzero(turn > 0)[3]), int(np.flatnonzero(turn < 0)[3]),
             int(with_future[0]), int(with_future[len(with_future) // 2])]
    if key == "ot":
        must_pass = np.flatnonzero(mask[:, 64] & ~mask.all(1))
        front += [int(must_pass[0]), int(must_pass[-1])]
    front.append(front[4])                                             # a repeated index
    idx = np.array(front + rng.integers(0, cap, n_rows - len(front)).tolist(), np.int64)
    # what the tests rely on
    assert 0 in idx and cap - 1 in idx and len(np.unique(idx)) < len(idx)
    assert ((prob[idx] == 0).all(1) & mask[idx].all(1)).sum() >= 2
    assert (turn[idx] > 0).any() and (turn[idx] < 0).any()
    assert (fut[idx] != 0).any()
    if key == "ot":
        assert (mask[idx, 64] & ~mask[idx].all(1)).any()
    return idx


def main():
    numba_stand_in()
    ReplayBuffer = load_by_path("ref_replay_buffer", "src", "ReplayBuffer.py").ReplayBuffer
    g = np.load(os.path.join(HERE, "g15_replay_buffer.npz"))
    rng = np.random.default_rng(16)
    out = {}
    for key, (game, (A, R, Cc), n_rows) in GAMES.items():
        augment = load_by_path(f"ref_{key}_utils", "src", "environments", game, "utils.py").augment
        cap = int(g[f"{key}_capacity"][0])
        buf = ReplayBuffer(3, cap, A, R, Cc, device="cpu")
        for t in TENSORS:
            getattr(buf, t).copy_(torch.from_numpy(g[f"{key}_{t}"]))
        buf._ptr = int(g[f"{key}_ptr"][0])
        assert len(buf) == cap
        idx = choose_rows(key, g, n_rows, rng)
        batch = augment(buf.get(torch.from_numpy(idx)))
        assert len(batch) == len(TENSORS)
        out[f"{key}_idx"] = idx
        for t, x in zip(TENSORS, batch):
            out[f"{key}_{t}"] = x.numpy().copy()
    cases, sizes = [], []
    for length, capacity, ratio, batch, full in SAMPLE_CASES:
        buf = ReplayBuffer(3, capacity, 7, 6, 7, replay_ratio=ratio, device="cpu")
        buf._ptr = length
        np.random.seed(0)
        loader = buf.sample(batch, full_batches=full)
        cases.append((length, capacity, ratio, batch, int(full)))
        sizes.append((len(loader.dataset), len(loader)))
    out["sample_cases"] = np.array(cases, np.float64)                  # every entry is exact in a double
    out["sample_sizes"] = np.array(sizes, np.int64)
    path = os.path.join(HERE, "g16_training_batch.npz")
    np.savez_compressed(path, **out)
    print(f"g16_training_batch.npz  {os.path.getsize(path) / 1024:.1f} KiB")
    for c, s in zip(cases, sizes):
        print(c, "->", s)


if __name__ == "__main__":
    main()
