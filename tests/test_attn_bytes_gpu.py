"""The attention / heads kernels (nn_attn.hip, nn_attn_heads.hip, nn_heads.hip) and the model object against bytes recorded
from the commit BEFORE their earlier forms were removed (EXPERIMENTS.md E20): tests/golden/g19_attn_bytes.npz was written
by tools/record_attn_golden.py in a checkout of that commit, where the default forms and the earlier ones (az_nn_debug bit
8) agreed on every case, and az_nn_attn_heads, az_nn_attn_block, az_nn_heads, az_nn_model_forward and
az_nn_model_forward_positions have to reproduce them: same inputs (from the seed in the record, checked by digest), same
output bytes, the NaN prefill of rows nobody writes included.  The cases are listed in the tool's docstring: one
workgroup with 0 to 34 samples per wavefront, free grids up to 4099 samples, compact lists with stray indices, zero and
1e18 rows, sharpened q-norm weights, eps below FLT_MIN (the rsqrtf() instantiation).

test_bytes_of_the_parent_commit runs every case of the record.  tests/test_value_tail_gpu.py, test_attn_loads_gpu.py and
test_attn_slots_gpu.py keep, under the names they had when they compared the two forms, the groups of cases that guard
one property of the kernels each; they call check() here."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_attn_golden as R  # noqa: E402


_runner = []


@pytest.fixture(scope="module")
def runner():
    """the tool's Runner (library, both weight sets on the device), made once for all the modules that import this"""
    if not _runner:
        sys.path.insert(0, ROOT)
        import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
        import __graft_entry__ as ge
        ge.build()
        _runner.append(R.Runner())
    return _runner[0]


def test_record_is_complete():
    with np.load(R.FIXTURE) as z:
        assert int(z["seed"]) == R.SEED and z["w2"].shape == (32,)
        assert sorted(z.files) == sorted(["seed", "w2"] + [p + n for n in R.all_case_names() for p in ("in/", "out/")])
        for n, c in R.CASES.items():
            B = len(R._model_inputs("planes")["mask"]) if c["kind"] == "planes" else c["B"]
            whole = (B, 42, 64) if c["entry"] == "block" else (B, 11)
            nbytes = int(np.prod(whole)) * (2 if c["entry"] == "block" else 4)
            assert z["out/" + n].shape == (whole if nbytes <= R.WHOLE_UP_TO else (32,)), n


def check(runner, name):
    """one case: the inputs are the recorded ones, the outputs have the recorded bytes; and what holds whatever the record
    says - a compact list writes its listed rows and no other, every other case but eps = 0 is finite"""
    c = R.CASES[name]
    ins, out = runner.run(name)
    with np.load(R.FIXTURE) as z:
        assert np.array_equal(z["w2"], runner.wdigest["w2", False]), "the drawn weights are not the recorded ones"
        assert np.array_equal(z["in/" + name], ins), "the generated inputs are not the recorded ones"
        want = z["out/" + name]
    finite = (out & 0x7F80) != 0x7F80 if out.dtype == np.uint16 else np.isfinite(out.view(np.float32))
    if c["live"] is not None:                               # compact: the listed rows, and only they, were written
        listed, strays = R.listed_rows(name)
        assert listed.sum() == c["live"] - strays
        assert finite[listed].all(), name
        assert (out[~listed] == 0x7FC00000).all(), name     # (f32 NaN as torch.full writes it)
    elif c["eps"] != 0.0:
        assert finite.all(), name
    got = R.stored(out)
    assert got.shape == want.shape and np.array_equal(got, want), name


@pytest.mark.parametrize("name", R.all_case_names())
def test_bytes_of_the_parent_commit(runner, name):
    check(runner, name)
