"""The deferred value tail of az_nn_attn_heads and the one-sigmoid gate tile of the attention body (nn_heads_core.h,
nn_attn_core.h): the cases of tests/golden/g19_attn_bytes.npz that guard them, byte for byte against the record of the
commit that still had the earlier forms (tests/test_attn_bytes_gpu.py, tools/record_attn_golden.py).  With the grid capped
to one workgroup (12 wavefronts) a few hundred samples reach the 16-slot flush of a wavefront."""
import pytest

from test_attn_bytes_gpu import check, runner  # noqa: F401  (runner: the fixture)

pytestmark = pytest.mark.gpu

SHARP = {False: "soft", True: "sharp"}


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("B", [1, 13, 192, 193, 401])
def test_attn_heads_one_workgroup(runner, B, sharp):
    """one workgroup: 0, 1-2, exactly 16, 16-17 and 33-34 samples per wavefront"""
    for mask in ("mask", "nomask"):
        check(runner, "heads/w1/plain/b%d/cap1/%s/%s" % (B, mask, SHARP[sharp]))


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("B", [777, 4099])
def test_attn_heads_uncapped(runner, B, sharp):
    for mask in ("mask", "nomask"):
        check(runner, "heads/w1/plain/b%d/cap0/%s/%s" % (B, mask, SHARP[sharp]))


@pytest.mark.parametrize("B,live,cap,stray", [(9, 5, 0, False), (401, 260, 1, False), (401, 260, 1, True), (9, 9, 0, True)])
def test_attn_heads_compact_list(runner, B, live, cap, stray):
    """batch_dev < B and shuffled scatter rows: listed rows as recorded, every other row still NaN; stray: some listed
    indices lie outside the batch (negative, B, far beyond) and are dropped, never written"""
    check(runner, "heads/w1/plain/b%dl%d%s/cap%d/mask/soft" % (B, live, "s" if stray else "", cap))


@pytest.mark.parametrize("sharp", [False, True])
def test_attn_block_gate_tile(runner, sharp):
    """az_nn_attn_block: the gate tile alone"""
    for B in (1, 3, 50):
        check(runner, "block/w1/plain/b%d/cap0/nomask/%s" % (B, SHARP[sharp]))


def test_heads_split_tail(runner):
    """az_nn_heads: the pair tail as policy_tail + value_tail"""
    for B in (1, 2, 3, 9):
        check(runner, "pair/w1/plain/b%d/cap0/mask/soft" % B)


def test_native_model_forward(runner):
    """az_nn_model_forward on about 3000 positions"""
    check(runner, "model/w1/planes/b0/cap0/mask/soft")
