"""The kernels of nn_conv.hip against bytes recorded from the commit BEFORE their integer work was reduced (EXPERIMENTS.md
E18): tests/golden/g14_conv_block_bytes.npz was written by tools/record_conv_golden.py in a checkout of that commit, and
every entry point that include/az_nn.h declares for the file - az_nn_conv_block (c_in 64 with and without the residual,
c_in 32), az_nn_stem_conv_block_positions, az_nn_stem_embed, az_nn_stem_embed_positions - has to reproduce them: same
inputs (from the seed in the record, checked by digest), same output bytes.

    free grid            batch 1, 3, 4, 5        dead waves; a partial tile; exactly one tile; one full + one partial
                         batch 13, batch_dev 9   the NaN canary in rows 9.. is part of the compared bytes
                         stem forms, gather list 9 of 13, one index outside the rows
    AZ_NN_CONV_GRID=2    batch 13                two tiles per workgroup, both raw-buffer parities, the last tile partial
    AZ_NN_CONV_GRID=1    batch 13                four tiles in one workgroup

The variable is read once per process, so each capped group runs once in a child process (the tool itself, with a time
limit); the free group runs in this process unless the variable is set here."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_conv_golden as R  # noqa: E402

_groups = {}


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()


def _group(name):
    """the results of a case's group, computed once"""
    g = name.split("/")[0]
    if g not in _groups:
        in_process = g == "free" and "AZ_NN_CONV_GRID" not in os.environ
        _groups[g] = R.run_group(g) if in_process else R.run_group_in_child(g, timeout=300)
    return _groups[g]


def test_record_is_complete():
    with np.load(R.FIXTURE) as z:
        assert int(z["seed"]) == R.SEED
        for n in R.all_case_names():
            assert "in/" + n in z.files and "out/" + n in z.files, n
            batch = int(n.split("/")[2][1:].split("n")[0].split("g")[0])
            assert z["out/" + n].shape == ((batch, 42, 64) if batch <= R.WHOLE_UP_TO else (32,)), n


@pytest.mark.parametrize("name", R.all_case_names())
def test_bytes_of_the_parent_commit(built, name):
    ins, out = _group(name)[name]
    with np.load(R.FIXTURE) as z:
        assert np.array_equal(z["in/" + name], ins), "the generated inputs are not the recorded ones"
        want = z["out/" + name]
    if "n9" in name or "g9" in name:                     # rows past batch_dev: the canary, untouched
        assert (out[9:] == 0x7FC0).all(), name               # (bf16 NaN as torch.full writes it)
        assert (out[:9] != 0x7FC0).any(axis=(1, 2)).all(), name   # every listed row was written
    got = R.stored(out)
    assert got.shape == want.shape and np.array_equal(got, want), name
