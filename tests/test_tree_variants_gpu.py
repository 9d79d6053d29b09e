"""Every route through the tree kernels that K or an environment switch selects, held to the plain-C oracle bit for
bit (visit counts, symmetry ids, leaf signature, root statistics as uint32 bit patterns; tree_variant_child.py).

The other suites reach Connect4 with K in {1, 2, 3, 4, 5, 7, 8} and Othello with K in {1, 4} under the default
switches: k_select8x4 / k_select8 / k_select<Othello>, k_backprop_spread / k_backprop_batched.  Here:
  in process    K > 8 (Connect4: k_backprop<Connect4> and k_select8<true>) and Othello K > 4 (k_backprop<Othello>);
  child process AZ_SELECT_VARIANT=0 (k_select<Connect4>), =1 (k_select8 at K <= 4), AZ_BACKPROP_SPREAD=0
                (k_backprop_batched<Connect4>), AZ_BACKPROP_V1=1 (k_backprop at K <= 4, both games),
                AZ_TREES_PER_WAVE=2 (lane groups of a wavefront that hold no tree).
Sizes: the smallest with a last wavefront that is not full (13 and 20 trees), paths deeper than the 8 lanes of a
Connect4 group (200+ simulations on few trees), duplicate and terminal leaves (20-ply openings).
"""
import os
import subprocess
import sys

import pytest

from tree_variant_child import side_by_side

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
CHILD = os.path.join(ROOT, "tests", "tree_variant_child.py")
SWITCHES = ("AZ_SELECT_VARIANT", "AZ_BACKPROP_V1", "AZ_BACKPROP_SPREAD", "AZ_TREES_PER_WAVE")


@pytest.fixture(scope="module")
def mcts_cpp():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src import mcts_cpp as m
    return m


@pytest.mark.parametrize("K", [9, 12])
def test_connect4_k_above_8_vs_oracle(mcts_cpp, K):
    """K > 8: k_backprop<Connect4, true, *> after k_select8<true> (the recipe of
    test_hip_parity.test_vs_oracle_backup_lane_group_sizes, which stops at the 8 groups of k_backprop_spread)."""
    side_by_side(mcts_cpp, "connect4", 13, 400, K, 3)


def test_othello_k_above_4_vs_oracle(mcts_cpp):
    """K > 4: k_backprop<Othello> (k_backprop_batched holds four leaves per tree)."""
    side_by_side(mcts_cpp, "othello", 20, 80, 6, 3)


ENV_ROUTES = [
    ("connect4", {"AZ_SELECT_VARIANT": "0"}),
    ("connect4", {"AZ_SELECT_VARIANT": "1"}),
    ("connect4", {"AZ_BACKPROP_SPREAD": "0"}),
    ("connect4", {"AZ_BACKPROP_V1": "1"}),
    ("connect4", {"AZ_SELECT_VARIANT": "1", "AZ_BACKPROP_SPREAD": "0", "AZ_TREES_PER_WAVE": "2"}),
    ("othello", {"AZ_BACKPROP_V1": "1"}),
]


@pytest.mark.parametrize("game,switches", ENV_ROUTES, ids=lambda v: v if isinstance(v, str) else ",".join("%s=%s" % kv for kv in v.items()))
def test_env_selected_route_vs_oracle(mcts_cpp, game, switches):
    """The switches are read once per process: a fresh interpreter per route, one after another."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    size = ["13", "200", "4", "2"] if game == "connect4" else ["20", "80", "4", "2"]
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD, game] + size
    r = subprocess.run(cmd, env=env, timeout=120, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
