#!/usr/bin/env python3
"""Generate tests/golden/g15_replay_buffer.npz: what the REAL reference's replay buffer holds after the games
of fixtures G11, G10 (Connect4) and G12 (Othello) were stored into it.

Run in the build container only (needs the reference checkout; CPU, no GPU, no compiled piece):

    python tests/golden/make_golden_replay.py            # AZ_REFERENCE=<checkout> if it is not /root/reference

The `play_data` tuples of every game are rebuilt from the fixture's g{i}_* arrays (one tuple per row: state,
prob, winner, steps_to_end, aux target, root WDL, valid mask and - where the fixture has it - the td-step
column), the games of a fixture are ordered by (length, index) - their (finishing ply, slot) order, since all
start together without refill - and every tuple goes through the reference's own `ReplayBuffer.store`
(src/ReplayBuffer.py:92-123, imported unmodified from the checkout), as server.py:300-302 does.

  Connect4  g11 then g10 into ONE buffer of 389 rows: 145 + 363 rows, so the ring wraps, g10 starts at a
            non-zero _ptr, and every slot has been written (the reference leaves `state` and `prob`
            uninitialised)
  Othello   g12 into a buffer of 307 rows (490 rows stored)

Neither capacity is a multiple of a game's row count.  Nothing from the reference is copied: the committed
output is data - the eight tensors, `_ptr` and the capacity per game.
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("AZ_REFERENCE", "/root/reference")
CAPACITY = {"c4": 389, "ot": 307}
TENSORS = ("state", "prob", "winner", "steps_to_end", "aux_target", "root_wdl", "valid_mask", "future_root_wdl")
COLUMNS = ("state", "prob", "z", "steps", "aux", "root_wdl", "mask", "fut")


def reference_buffer_class():
    spec = importlib.util.spec_from_file_location("ref_replay_buffer", os.path.join(REF, "src", "ReplayBuffer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.ReplayBuffer


def games_of(name):
    """[(length, index, play_data)] of a self-play fixture, in (length, index) order."""
    g = np.load(os.path.join(HERE, name + ".npz"))
    cols = [c for c in COLUMNS if f"g0_{c}" in g.files]
    games = []
    i = 0
    while f"g{i}_state" in g.files:
        arrs = [g[f"g{i}_{c}"] for c in cols]
        n = len(arrs[0])
        play = tuple(tuple(a[t] for a in arrs) for t in range(n))
        games.append((n - 1, i, play))
        i += 1
    return sorted(games, key=lambda t: (t[0], t[1]))


def main():
    ReplayBuffer = reference_buffer_class()
    out = {}
    for key, names, (A, R, Cc) in (("c4", ("g11_selfplay_plain_search", "g10_selfplay_numpy_rng"), (7, 6, 7)),
                                   ("ot", ("g12_selfplay_othello",), (65, 8, 8))):
        buf = ReplayBuffer(3, CAPACITY[key], A, R, Cc, device="cpu")
        rows = 0
        for name in names:
            for _length, _index, play in games_of(name):
                for data in play:
                    buf.store(*data)
                rows += len(play)
        assert rows > CAPACITY[key] and buf._ptr == rows
        for t in TENSORS:
            out[f"{key}_{t}"] = getattr(buf, t).numpy().copy()
        out[f"{key}_ptr"] = np.array([buf._ptr], np.int64)
        out[f"{key}_capacity"] = np.array([buf.current_capacity], np.int64)
    path = os.path.join(HERE, "g15_replay_buffer.npz")
    np.savez_compressed(path, **out)
    print(f"g15_replay_buffer.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
