"""Where the fused attention kernel's global loads sit (nn_attn_core.h, nn_attn_heads.hip): a sample's six row vectors
requested together, the residual rows one token tile ahead, the policy tail's row index and mask byte a sample ahead.
None of it may change a byte: the cases of tests/golden/g19_attn_bytes.npz that guard it, against the record of the commit
that still had the earlier load code (tests/test_attn_bytes_gpu.py, tools/record_attn_golden.py).  One workgroup is 12
wavefronts, each on every 12th sample."""
import pytest

from test_attn_bytes_gpu import check, runner  # noqa: F401  (runner: the fixture)

pytestmark = pytest.mark.gpu

SHARP = {False: "soft", True: "sharp"}


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("B", [1, 12, 13, 25, 193, 401])
def test_attn_heads_one_workgroup(runner, B, sharp):
    """one workgroup: a wavefront with no next sample (1); every wavefront exactly one sample (12); one wavefront with a
    next sample, eleven without (13); a half-empty pair after a full one (25); the 16-slot flush between two samples
    (193); many samples per wavefront (401)"""
    for mask in ("mask", "nomask"):
        check(runner, "heads/w1/plain/b%d/cap1/%s/%s" % (B, mask, SHARP[sharp]))


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("B", [777, 4099])
def test_attn_heads_uncapped(runner, B, sharp):
    for mask in ("mask", "nomask"):
        check(runner, "heads/w1/plain/b%d/cap0/%s/%s" % (B, mask, SHARP[sharp]))


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("B,live,cap,stray", [(9, 5, 0, False), (401, 260, 1, False), (401, 260, 1, True), (9, 9, 0, True),
                                              (9, 5, 0, True)])
def test_attn_heads_compact_list(runner, B, live, cap, stray, sharp):
    """The device-side count below `batch`, shuffled output rows, and NaN in every row of x at and past the count: a
    prefetch that went by the unclamped batch, or a tail that consumed a stray row, would carry the NaN into a listed
    row.  Listed rows have the recorded bytes and are finite, every other row keeps its NaN prefill.
    stray: some listed indices lie outside the batch (negative, B, far beyond) and are dropped, never dereferenced."""
    check(runner, "heads/w1/plain/b%dl%d%s/cap%d/mask/%s" % (B, live, "s" if stray else "", cap, SHARP[sharp]))


@pytest.mark.parametrize("sharp", [False, True])
def test_attn_block(runner, sharp):
    """az_nn_attn_block shares the attention body: the six row vectors requested together"""
    for B in (1, 3, 50):
        check(runner, "block/w1/plain/b%d/cap0/nomask/%s" % (B, SHARP[sharp]))


def test_native_model_forward_positions(runner):
    """az_nn_model_forward_positions on 3000 positions"""
    check(runner, "model/w1/positions/b3000/cap0/mask/soft")
