"""The fused attention kernel with fewer issue slots (nn_common.h rsq_normal / col_sum2 / col_max2 / sum16_dpp, used by
the default forms of az_nn_attn_heads and az_nn_attn_block): bare reciprocal square roots, two column sums through one
set of lane swaps, the token means as DPP adds.  None of it may change a byte: every case compares the raw output arrays
of the default forms with those of az_nn_debug bit 8, which keeps rsqrtf() and the single reductions as they compiled
before.  Bits 16-27 of az_nn_debug cap az_nn_attn_heads' grid: one workgroup is 12 wavefronts, each on every 12th sample.

The weights are random in the checkpoint's shapes; the activations carry rows of exact zeros (the reciprocal square root's
smallest argument, eps itself) and rows of magnitude 1e18 (squares near 1e36, their sums still finite in f32)."""
import ctypes as C
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
LEGACY = 256                    # AZ_NN_DEBUG_LEGACY_TAIL
EPS = 1e-5


def _cap(n):                    # AZ_NN_DEBUG_GRID_CAP
    return (n & 0xfff) << 16


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
    twins = {}
    for sharp in (False, True):
        fast = FastConnect4Net.from_module(net)
        if sharp:       # sharpened q-norm weights: scores outside the bound, the max-subtracting softmax runs
            fast.qn_w = (fast.qn_w.float() * 40.0).to(fast.qn_w.dtype).contiguous()
        twins[sharp] = fast
    initial = L.az_nn_debug_flags()
    yield dict(torch=torch, L=L, twins=twins)
    L.az_nn_debug(initial)


def _inputs(torch, B, seed, extremes=True):
    """x (B, 42, 64) bf16 and a mask.  extremes: about one token row in eight is exactly zero and one in eight has
    entries +-1e18 x [0.5, 1); sample 0 gets both kinds in its first and its last token tile, a whole zero sample follows
    when there is room for one."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn((B, 42, 64), device="cuda", generator=gen) * 1.5
    if extremes:
        kind = torch.randint(0, 8, (B, 42), device="cuda", generator=gen)
        kind[0, 0], kind[0, 1], kind[0, 40], kind[0, 41] = 0, 1, 1, 0
        big = (torch.rand((B, 42, 64), device="cuda", generator=gen) * 0.5 + 0.5) * 1e18
        big = torch.where(torch.rand((B, 42, 64), device="cuda", generator=gen) < 0.5, -big, big)
        x = torch.where((kind == 1)[..., None], big, x)
        x = torch.where((kind == 0)[..., None], torch.zeros_like(x), x)
        if B > 1:
            x[1] = 0.0
    mask = torch.rand((B, 7), device="cuda", generator=gen) > 0.25
    mask[:, 3] = True
    return x.to(torch.bfloat16).contiguous(), mask.to(torch.uint8).contiguous(), gen


def _attn_heads(env, fast, x, m8, B, flags, eps=EPS, rows=None, n_rows=None):
    torch, L = env["torch"], env["L"]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = [torch.full(shape, float("nan"), device="cuda") for shape in ((B, 7), (B, 3), (B,))]
    before = L.az_nn_debug_flags()
    L.az_nn_debug(flags)
    try:
        assert L.az_nn_attn_heads(x.data_ptr(), fast.pre_w.data_ptr(), fast.qkvg_w.data_ptr(), fast.qn_w.data_ptr(),
                                  fast.kn_w.data_ptr(), fast.o_w.data_ptr(), C.byref(fast._heads_w),
                                  None if m8 is None else m8.data_ptr(), *[t.data_ptr() for t in out], B, eps,
                                  None if rows is None else rows.data_ptr(), None if n_rows is None else n_rows.data_ptr(), s) == 0
        torch.cuda.synchronize()
    finally:
        L.az_nn_debug(before)
    return out


def _attn_block(env, fast, x, B, flags, eps=EPS):
    torch, L = env["torch"], env["L"]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    y = torch.full_like(x, float("nan"))
    before = L.az_nn_debug_flags()
    L.az_nn_debug(flags)
    try:
        assert L.az_nn_attn_block(x.data_ptr(), fast.pre_w.data_ptr(), fast.qkvg_w.data_ptr(), fast.qn_w.data_ptr(),
                                  fast.kn_w.data_ptr(), fast.o_w.data_ptr(), y.data_ptr(), B, eps, None, s) == 0
        torch.cuda.synchronize()
    finally:
        L.az_nn_debug(before)
    return y


def _same_bytes(torch, a, b, tag):
    for name, u, v in zip(("probs", "wdl", "moves_left"), a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (tag, name)


def _heads_both_ways(env, fast, x, m8, B, cap, **kw):
    """az_nn_attn_heads under the default and under bit 8: the first is returned, the two are equal as bytes"""
    new = _attn_heads(env, fast, x, m8, B, _cap(cap), **kw)
    old = _attn_heads(env, fast, x, m8, B, _cap(cap) | LEGACY, **kw)
    _same_bytes(env["torch"], new, old, ("bit 8", B, cap))
    return new


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 25])
def test_attn_heads(env, B, sharp):
    """one sample; a full pair; a half-empty pair after a full one (3); 25: two wavefronts per workgroup with a second
    pair, uncapped and with everything in one workgroup"""
    torch = env["torch"]
    fast = env["twins"][sharp]
    x, m8, _ = _inputs(torch, B, 1500 + B)
    for cap in (0, 1):
        for mk in (m8, None):
            for t in _heads_both_ways(env, fast, x, mk, B, cap):
                assert torch.isfinite(t).all()


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("B", [1, 2, 3, 25])
def test_attn_block(env, B, sharp):
    torch = env["torch"]
    fast = env["twins"][sharp]
    x, _, _ = _inputs(torch, B, 1600 + B)
    new, old = _attn_block(env, fast, x, B, 0), _attn_block(env, fast, x, B, LEGACY)
    assert torch.isfinite(new.float()).all()
    assert torch.equal(new.view(torch.int16), old.view(torch.int16)), (B, sharp)


@pytest.mark.parametrize("sharp", [False, True])
def test_attn_heads_flush_twice(env, sharp):
    """one workgroup and 12 x 17 + 1 samples: every wavefront fills its 16 mean slots and flushes, then parks one more
    sample (the first wavefront two) and flushes a partial set"""
    torch = env["torch"]
    fast = env["twins"][sharp]
    B = 12 * 17 + 1
    x, m8, _ = _inputs(torch, B, 1700)
    for t in _heads_both_ways(env, fast, x, m8, B, 1):
        assert torch.isfinite(t).all()


@pytest.mark.parametrize("sharp", [False, True])
def test_attn_heads_compact_list(env, sharp):
    """25 samples scattered into 40 output rows: the listed rows equal bit 8's and are finite, the other 15 keep their
    NaN prefill; the samples past the device-side count are NaN and must not reach a listed row"""
    torch = env["torch"]
    fast = env["twins"][sharp]
    B, live = 40, 25
    x, m8, gen = _inputs(torch, B, 1800)
    x[live:] = float("nan")
    rows = torch.randperm(B, device="cuda", generator=gen).to(torch.int32).contiguous()
    n_rows = torch.tensor([live], dtype=torch.int64, device="cuda")
    new = _heads_both_ways(env, fast, x, m8, B, 0, rows=rows, n_rows=n_rows)
    listed = torch.zeros(B, dtype=torch.bool, device="cuda")
    listed[rows[:live].long()] = True
    assert listed.sum().item() == live
    for t in new:
        assert torch.isfinite(t[listed]).all()
        assert torch.isnan(t[~listed]).all()


@pytest.mark.parametrize("eps", [0.0, 1e-40])
def test_eps_below_flt_min_runs_the_guarded_form(env, eps):
    """An eps below FLT_MIN is outside rsq_normal()'s range: both settings launch the rsqrtf() form, so their bytes are
    equal, and the results are those of the two launches (az_nn_attn_block, az_nn_heads) at the same eps.
    eps = 1e-40 (a denormal) is where the guard matters: every output is finite.  eps = 0 is no working setting of
    either form, before this change or after it: the six padding tokens of a sample are rows of zeros, their statistic
    is 1 / sqrt(0 + 0) = inf and 0 x inf = NaN reaches every key - what is pinned is that the fused kernel and the two
    launches still agree, NaN for NaN.
    Bounds against the two launches where the values are finite: those of tests/test_attn_heads_gpu.py's _close (same
    rounding points, other f32 summation orders: a value next to a bf16 rounding boundary may round the other way, which
    moves an output by a few bf16 ulps of a logit) - maxima only, a mean over 25 samples says nothing about how rare such
    flips are."""
    torch, L = env["torch"], env["L"]
    fast = env["twins"][False]
    B = 25
    x, m8, _ = _inputs(torch, B, 1900, extremes=False)
    fused = _heads_both_ways(env, fast, x, m8, B, 0, eps=eps)
    y_new, y_old = _attn_block(env, fast, x, B, 0, eps=eps), _attn_block(env, fast, x, B, LEGACY, eps=eps)
    assert torch.equal(y_new.view(torch.int16), y_old.view(torch.int16))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    two = [torch.full(shape, float("nan"), device="cuda") for shape in ((B, 7), (B, 3), (B,))]
    assert L.az_nn_heads(y_new.data_ptr(), C.byref(fast._heads_w), m8.data_ptr(), *[t.data_ptr() for t in two], B, eps,
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
