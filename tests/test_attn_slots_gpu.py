"""The fused attention kernel with fewer issue slots (nn_common.h rsq_normal / col_sum2 / col_max2 / sum16_dpp, used by
az_nn_attn_heads and az_nn_attn_block): bare reciprocal square roots, two column sums through one set of lane swaps, the
token means as DPP adds.  None of it may change a byte: the cases of tests/golden/g19_attn_bytes.npz that guard it, against
the record of the commit that still had rsqrtf() and the single reductions as a second form (tests/test_attn_bytes_gpu.py,
tools/record_attn_golden.py): random weights in the checkpoint's shapes, activations with rows of exact zeros (the
reciprocal square root's smallest argument, eps itself) and rows of magnitude 1e18 (squares near 1e36, their sums still
finite in f32).  Two tests need no record: an eps below FLT_MIN, which launches the rsqrtf() instantiation, against the
two launches (az_nn_attn_block, az_nn_heads) at the same eps, and the paired column reductions against the single ones."""
import ctypes as C
import os
import sys

import pytest

from test_attn_bytes_gpu import check, runner  # noqa: F401  (runner: the fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")


def _random_net(torch, az_net):
    """Connect4Net with every parameter drawn from one seeded CPU generator: matrices N(0, 1 / fan_in), norm weights
    1 + N(0, 0.25^2), everything else (biases, embeddings) N(0, 0.1^2)"""
    net = az_net.Connect4Net(device="cuda").eval()
    gen = torch.Generator().manual_seed(1500)
    with torch.no_grad():
        for name, p in net.named_parameters():
            v = torch.randn(p.shape, generator=gen)
            if p.dim() >= 2:
                v = v / float(p[0].numel()) ** 0.5
            elif "norm" in name and name.endswith("weight"):
                v = 1.0 + 0.25 * v
            else:
                v = 0.1 * v
            p.copy_(v.to(p.device))
    return net


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src import az_net
    from src.fast_net import FastConnect4Net, glue
    net = _random_net(torch, az_net)
    L = glue()
    return dict(torch=torch, L=L, fast=FastConnect4Net.from_module(net))


def _inputs(torch, B, seed):
    """x (B, 42, 64) bf16 and a mask with column 3 open"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((B, 42, 64), device="cuda", generator=gen) * 1.5
    mask = torch.rand((B, 7), device="cuda", generator=gen) > 0.25
    mask[:, 3] = True
    return x.to(torch.bfloat16).contiguous(), mask.to(torch.uint8).contiguous()


def _attn_heads(env, fast, x, m8, B, eps):
    torch, L = env["torch"], env["L"]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = [torch.full(shape, float("nan"), device="cuda") for shape in ((B, 7), (B, 3), (B,))]
    assert L.az_nn_attn_heads(x.data_ptr(), fast.pre_w.data_ptr(), fast.qkvg_w.data_ptr(), fast.qn_w.data_ptr(),
                              fast.kn_w.data_ptr(), fast.o_w.data_ptr(), C.byref(fast._heads_w), m8.data_ptr(),
                              *[t.data_ptr() for t in out], B, eps, None, None, s) == 0
    torch.cuda.synchronize()
    return out


def _attn_block(env, fast, x, B, eps):
    torch, L = env["torch"], env["L"]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    y = torch.full_like(x, float("nan"))
    assert L.az_nn_attn_block(x.data_ptr(), fast.pre_w.data_ptr(), fast.qkvg_w.data_ptr(), fast.qn_w.data_ptr(),
                              fast.kn_w.data_ptr(), fast.o_w.data_ptr(), y.data_ptr(), B, eps, None, s) == 0
    torch.cuda.synchronize()
    return y


SHARP = {False: "soft", True: "sharp"}


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 25])
def test_attn_heads(runner, B, sharp):
    """one sample; a full pair; a half-empty pair after a full one (3); 25: two wavefronts per workgroup with a second
    pair, uncapped and with everything in one workgroup"""
    for cap in (0, 1):
        for mask in ("mask", "nomask"):
            check(runner, "heads/w2/extreme/b%d/cap%d/%s/%s" % (B, cap, mask, SHARP[sharp]))


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 25])
def test_attn_block(runner, B, sharp):
    check(runner, "block/w2/extreme/b%d/cap0/nomask/%s" % (B, SHARP[sharp]))


@pytest.mark.parametrize("sharp", [False, True])
def test_attn_heads_flush_twice(runner, sharp):
    """one workgroup and 12 x 17 + 1 samples: every wavefront fills its 16 mean slots and flushes, then parks one more
    sample (the first wavefront two) and flushes a partial set"""
    check(runner, "heads/w2/extreme/b205/cap1/mask/" + SHARP[sharp])


@pytest.mark.parametrize("sharp", [False, True])
def test_attn_heads_compact_list(runner, sharp):
    """25 samples scattered into 40 output rows: the listed rows have the recorded bytes and are finite, the other 15 keep
    their NaN prefill; the samples past the device-side count are NaN and must not reach a listed row"""
    check(runner, "heads/w2/extreme/b40l25/cap0/mask/" + SHARP[sharp])


@pytest.mark.parametrize("eps", [0.0, 1e-40])
def test_eps_below_flt_min_runs_the_guarded_form(env, eps):
    """An eps below FLT_MIN is outside rsq_normal()'s range: the rsqrtf() instantiations are launched (their bytes are in
    tests/test_attn_bytes_gpu.py's record), and the results are those of the two launches (az_nn_attn_block, az_nn_heads)
    at the same eps.
    eps = 1e-40 (a denormal) is where the guard matters: every output is finite.  eps = 0 is no working setting of
    either form: the six padding tokens of a sample are rows of zeros, their statistic
    is 1 / sqrt(0 + 0) = inf and 0 x inf = NaN reaches every key - what is pinned is that the fused kernel and the two
    launches still agree, NaN for NaN.
    Bounds against the two launches where the values are finite: those of tests/test_attn_heads_gpu.py's _close (same
    rounding points, other f32 summation orders: a value next to a bf16 rounding boundary may round the other way, which
    moves an output by a few bf16 ulps of a logit) - maxima only, a mean over 25 samples says nothing about how rare such
    flips are."""
    torch, L = env["torch"], env["L"]
    fast = env["fast"]
    B = 25
    x, m8 = _inputs(torch, B, 1900)
    fused = _attn_heads(env, fast, x, m8, B, eps)
    y = _attn_block(env, fast, x, B, eps)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    two = [torch.full(shape, float("nan"), device="cuda") for shape in ((B, 7), (B, 3), (B,))]
    assert L.az_nn_heads(y.data_ptr(), C.byref(fast._heads_w), m8.data_ptr(), *[t.data_ptr() for t in two], B, eps,
                         None, None, s) == 0
    torch.cuda.synchronize()
    for name, a, b, bound in zip(("probs", "wdl", "moves_left"), fused, two, (5e-3, 5e-3, 0.05)):
        fin = torch.isfinite(a)
        assert torch.equal(fin, torch.isfinite(b)), name
        assert torch.equal(torch.isnan(a), torch.isnan(b)), name
        if eps > 0.0:
            assert fin.all(), name
        err = (a[fin] - b[fin]).abs().max().item() if fin.any() else 0.0
        print("eps = %g, fused against two launches:" % eps, name, "finite %d of %d, max |difference| %.3g"
              % (int(fin.sum().item()), a.numel(), err))
        assert err <= bound, (name, err)


def test_col_reduce2_equals_two_single_reductions(env):
    """col_sum2(a, b) against col_sum(a), col_sum(b) (and the max forms) on one wavefront: 64 lanes of random floats with
    +-inf among them, all 64 lanes of both outputs compared as uint32.  A column (lanes l, l + 16, l + 32, l + 48) with
    +inf and -inf sums to NaN in both forms."""
    torch, L = env["torch"], env["L"]
    gen = torch.Generator(device="cuda").manual_seed(2000)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for trial in range(8):
        ab = torch.randn((2, 64), device="cuda", generator=gen) * 10.0 ** (trial - 3)
        where = torch.randint(0, 64, (2, 6), device="cuda", generator=gen)
        for i in range(2):
            ab[i, where[i, :3]] = float("inf")
            ab[i, where[i, 3:]] = float("-inf")
        if trial == 0:
            ab[0] = torch.arange(64, device="cuda").float() + 1.0       # lane-numbered: a wrong partner shows in the value
            ab[1] = -(torch.arange(64, device="cuda").float() + 1.0) * 64.0
        ab = ab.contiguous()
        out = torch.full((8, 64), float("nan"), device="cuda")
        assert L.az_nn_debug_col_reduce2(ab[0].data_ptr(), ab[1].data_ptr(), out.data_ptr(), s) == 0
        torch.cuda.synchronize()
        bits = out.view(torch.int32)
        for op, base in (("sum", 0), ("max", 4)):
            assert torch.equal(bits[base], bits[base + 2]), (trial, op, "a")
            assert torch.equal(bits[base + 1], bits[base + 3]), (trial, op, "b")
        if trial == 0:      # and against the plain sums over the four rows of a column
            cols = ab.view(2, 4, 16)
            assert torch.equal(out[0], ((cols[0, 0] + cols[0, 1]) + (cols[0, 2] + cols[0, 3])).repeat(4))
            assert torch.equal(out[5], cols[1].max(0).values.repeat(4))
