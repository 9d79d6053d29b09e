#!/usr/bin/env python3
"""Generate tests/golden/g17_eval_match.npz from the REAL reference, compiled into oracle/_ref.

Run in the build container only (needs the reference checkout):

    make -C oracle ref && OMP_NUM_THREADS=1 python tests/golden/make_golden_match.py

What was done: the reference's own `TrainPipeline._batched_eval_games` (src/pipeline.py:264-335, with
`_sample_actions`, pipeline.py:337-351) is called UNBOUND on a namespace object that carries the attributes the
function reads (env, net, c_puct, dirichlet_alpha, env_name, vl_batch, use_symmetry, ...).  src/pipeline.py imports
`swanlab`, which is absent here: an empty stand-in module is placed in sys.modules first (as make_golden.py does for
numba); nothing of it is ever called.  The loop was NOT restated here - the restatement under test is
tests/match_harness.py.  The moves are recorded by wrapping `prune_roots` of the two search objects the function
builds (the function itself returns the winners only): a call with the games' actions, once per ply and object.

As in make_golden.py nothing from the reference is copied: its compiled extensions are imported from
oracle/_ref/native, its unmodified Python from the reference checkout.  Settings: eval_noise_eps 0 and symmetry off (the
reference's two search objects share ONE thread-local mt19937, so a noisy match cannot be reproduced by two
separately seeded engines), numpy's generator seeded for the sampler, a temperature high enough that the games
differ, two different numpy hash evaluators (salt 0 and a non-zero salt).  The committed file holds data only:
winners, every move, the salts and the settings.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("AZ_REFERENCE", "/root/reference")
assert os.environ.get("OMP_NUM_THREADS") == "1", "run with OMP_NUM_THREADS=1"

sys.path[:0] = [os.path.join(ROOT, "oracle", "_ref", "native"), REF, os.path.join(ROOT, "tests")]
for absent in ("numba", "swanlab"):
    if absent not in sys.modules:
        sys.modules[absent] = types.ModuleType(absent)
sys.modules["numba"].njit = lambda *a, **k: (lambda f: f)

from src.pipeline import TrainPipeline              # noqa: E402  (reference python, unmodified)
from src import MCTS_cpp as ref_wrapper             # noqa: E402  (reference python, unmodified)
from src.env_cpp.connect4 import Env as C4Env       # noqa: E402  (compiled reference)
from src.env_cpp.othello import Env as OtEnv        # noqa: E402  (compiled reference)

import match_harness as MH                          # noqa: E402


def _project_module(name, path):
    """A module of THIS project by file path (its package is called `src` too, like the reference's)."""
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


HASH = _project_module("az_hash_eval", os.path.join(ROOT, "alphazero-al_amd", "src", "hash_eval.py"))

SALT = 0x5A17C0DE1234ABCD
CASES = {
    # name: (game, n_games, n_playout, vl_batch, eval_temp, numpy seed, c_puct)
    "c4_k1": ("Connect4", 6, 30, 1, 1.0, 17, 1.4),
    "c4_k4": ("Connect4", 6, 30, 4, 1.0, 18, 1.4),
    "ot_k4": ("Othello", 4, 20, 4, 1.0, 19, 1.4),
}


def play(game, n_games, n_playout, vl_batch, eval_temp, np_seed, c_puct):
    if game == "Connect4":
        env, nets = C4Env(), (HASH.NumpyHashEvaluator(0), HASH.NumpyHashEvaluator(SALT))
    else:
        env, nets = OtEnv(), (MH.OthelloNumpyHashEvaluator(0), MH.OthelloNumpyHashEvaluator(SALT))
    ns = types.SimpleNamespace(env=env, net=nets[0], c_puct=c_puct, dirichlet_alpha=0.3, env_name=game, use_symmetry=False,
                               vl_batch=vl_batch, _sample_actions=TrainPipeline._sample_actions)
    log = []
    real = ref_wrapper.BatchedMCTS.prune_roots

    def recording(self, actions):
        log.append((id(self), np.array(actions, np.int32).copy()))
        return real(self, actions)
    ref_wrapper.BatchedMCTS.prune_roots = recording
    try:
        np.random.seed(np_seed)
        winners = TrainPipeline._batched_eval_games(ns, nets[0], nets[1], n_games, n_playout, eval_noise_eps=0.0,
                                                    eval_temp=eval_temp)
    finally:
        ref_wrapper.BatchedMCTS.prune_roots = real
    # two calls per ply (pipeline.py:326-327), the same actions in both
    assert len(log) % 2 == 0
    plies = []
    for a, b in zip(log[0::2], log[1::2]):
        assert a[0] != b[0] and np.array_equal(a[1], b[1])
        plies.append(a[1])
    # the function keeps finished games in the batch and plays their arg-max: replay the moves on Envs to find
    # where every game ended, and store -1 from there on
    moves = np.array(plies, np.int32)
    envs = [type(env)() for _ in range(n_games)]
    length = np.zeros(n_games, np.int32)
    for p in range(len(moves)):
        for i, e in enumerate(envs):
            if e.done():
                moves[p, i] = -1
            else:
                e.step(int(moves[p, i]))
                length[i] += 1
    assert all(e.done() for e in envs) and [int(e.winPlayer()) for e in envs] == [int(w) for w in winners]
    return np.asarray(winners, np.int32), moves, length


def main():
    out = dict(salts=np.array([0, SALT], np.uint64))
    for name, (game, n_games, n_playout, vl_batch, eval_temp, np_seed, c_puct) in CASES.items():
        winners, moves, length = play(game, n_games, n_playout, vl_batch, eval_temp, np_seed, c_puct)
        out[name + "_winner"] = winners
        out[name + "_moves"] = moves
        out[name + "_length"] = length
        out[name + "_settings"] = np.array([n_games, n_playout, vl_batch, np_seed], np.int32)
        out[name + "_floats"] = np.array([eval_temp, c_puct, 500.0, 0.3, 0.0], np.float64)   # temp, c_init, c_base, alpha, eps
        print(name, "winners", winners.tolist(), "lengths", length.tolist(),
              "distinct games", len({tuple(moves[:, i]) for i in range(n_games)}))
    path = os.path.join(HERE, "g17_eval_match.npz")
    np.savez_compressed(path, **out)
    print("g17_eval_match.npz  %.1f KiB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
