"""Where the fused attention kernel's global loads sit (nn_attn_core.h, nn_attn_heads.hip): a sample's six row vectors
requested together, the residual rows one token tile ahead, the policy tail's row index and mask byte a sample ahead.
None of it may change a byte: every case compares the raw output arrays of the default forms with those of az_nn_debug
bit 8, which keeps the earlier load code verbatim.  Bits 16-27 cap az_nn_attn_heads' grid: one workgroup is 12
wavefronts, each on every 12th sample."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from test_oracle_golden import load
from test_stem_conv_gpu import _positions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
LEGACY = 256                    # AZ_NN_DEBUG_LEGACY_TAIL


def _cap(n):                    # AZ_NN_DEBUG_GRID_CAP
    return (n & 0xfff) << 16


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src import az_net
    from src.fast_net import FastConnect4Net, Positions, glue
    wts = load("g7_checkpoint_weights")
    net = az_net.Connect4Net(device="cuda").eval()
    az_net.load_reference_weights(net, {k: wts[k] for k in wts.files})
    L = glue()
    twins = {}
    for sharp in (False, True):
        fast = FastConnect4Net.from_module(net)
        if sharp:       # sharpened q-norm weights: scores outside the bound, the max-subtracting softmax runs
            fast.qn_w = (fast.qn_w.float() * 40.0).to(fast.qn_w.dtype).contiguous()
        twins[sharp] = fast
    initial = L.az_nn_debug_flags()
    yield dict(torch=torch, net=net, FastNet=FastConnect4Net, Positions=Positions, L=L, twins=twins)
    L.az_nn_debug(initial)


def _inputs(torch, B, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    x = (torch.randn((B, 42, 64), device="cuda", generator=gen) * 1.5).to(torch.bfloat16)
    mask = (torch.rand((B, 7), device="cuda", generator=gen) > 0.25)
    mask[:, 3] = True
    return x, mask.to(torch.uint8).contiguous(), gen


def _attn_heads(env, fast, x, m8, B, flags, rows=None, n_rows=None):
    torch, L = env["torch"], env["L"]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    probs = torch.full((B, 7), float("nan"), device="cuda")
    wdl = torch.full((B, 3), float("nan"), device="cuda")
    ml = torch.full((B,), float("nan"), device="cuda")
    before = L.az_nn_debug_flags()
    L.az_nn_debug(flags)
    try:
        assert L.az_nn_attn_heads(x.data_ptr(), fast.pre_w.data_ptr(), fast.qkvg_w.data_ptr(), fast.qn_w.data_ptr(),
                                  fast.kn_w.data_ptr(), fast.o_w.data_ptr(), C.byref(fast._heads_w),
                                  None if m8 is None else m8.data_ptr(), probs.data_ptr(), wdl.data_ptr(), ml.data_ptr(), B, 1e-5,
                                  None if rows is None else rows.data_ptr(), None if n_rows is None else n_rows.data_ptr(), s) == 0
        torch.cuda.synchronize()
    finally:
        L.az_nn_debug(before)
    return probs, wdl, ml


def _same_bytes(torch, a, b, tag):
    for name, u, v in zip(("probs", "wdl", "moves_left"), a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)), (tag, name)


def _both_ways(env, fast, x, m8, B, cap, rows=None, n_rows=None):
    """default and bit 8 (the earlier load order): the first is returned, the two are equal"""
    torch = env["torch"]
    new = _attn_heads(env, fast, x, m8, B, _cap(cap), rows, n_rows)
    old = _attn_heads(env, fast, x, m8, B, _cap(cap) | LEGACY, rows, n_rows)
    _same_bytes(torch, new, old, ("bit 8", B, cap))
    return new


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("B", [1, 12, 13, 25, 193, 401])
def test_attn_heads_one_workgroup(env, B, sharp):
    """one workgroup: a wavefront with no next sample (1); every wavefront exactly one sample (12); one wavefront with a
    next sample, eleven without (13); a half-empty pair after a full one (25); the 16-slot flush between two samples
    (193); many samples per wavefront (401)"""
    torch = env["torch"]
    fast = env["twins"][sharp]
    x, m8, _ = _inputs(torch, B, 1100 + B)
    for mk in (m8, None):
        new = _both_ways(env, fast, x, mk, B, 1)
        for t in new:
            assert torch.isfinite(t).all()


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("B", [777, 4099])
def test_attn_heads_uncapped(env, B, sharp):
    torch = env["torch"]
    fast = env["twins"][sharp]
    x, m8, _ = _inputs(torch, B, 1200 + B)
    for mk in (m8, None):
        new = _both_ways(env, fast, x, mk, B, 0)
        for t in new:
            assert torch.isfinite(t).all()


@pytest.mark.parametrize("sharp", [False, True])
@pytest.mark.parametrize("B,live,cap,stray", [(9, 5, 0, False), (401, 260, 1, False), (401, 260, 1, True), (9, 9, 0, True),
                                              (9, 5, 0, True)])
def test_attn_heads_compact_list(env, B, live, cap, stray, sharp):
    """The device-side count below `batch`, shuffled output rows, and NaN in every row of x at and past the count: a
    prefetch that went by the unclamped batch, or a tail that consumed a stray row, would carry the NaN into a listed
    row.  Listed rows equal the oracle's and are finite, every other row keeps its NaN prefill.
    stray: some listed indices lie outside the batch (negative, B, far beyond) and are dropped, never dereferenced."""
    torch = env["torch"]
    fast = env["twins"][sharp]
    x, m8, gen = _inputs(torch, B, 1300 + B + live)
    x[live:] = float("nan")
    rows = torch.randperm(B, device="cuda", generator=gen).to(torch.int32)
    n_bad = 0
    if stray:
        bad = torch.tensor([-1, B, B + 7, 2**31 - 1, -2**31], dtype=torch.int32, device="cuda")
        at = torch.arange(0, live, max(1, live // len(bad)), device="cuda")[:len(bad)]
        rows[at] = bad[:len(at)]
        n_bad = len(at)
    rows = rows.contiguous()
    n_rows = torch.tensor([live], dtype=torch.int64, device="cuda")
    new = _both_ways(env, fast, x, m8, B, cap, rows, n_rows)
    named = rows[:live].long()
    named = named[(named >= 0) & (named < B)]
    listed = torch.zeros(B, dtype=torch.bool, device="cuda")
    listed[named] = True
    assert listed.sum().item() == live - n_bad
    for t in new:
        assert torch.isfinite(t[listed]).all()
        assert torch.isnan(t[~listed]).all()


@pytest.mark.parametrize("sharp", [False, True])
def test_attn_block(env, sharp):
    """az_nn_attn_block shares the attention body: the six row vectors requested together against the earlier order"""
    torch, L = env["torch"], env["L"]
    fast = env["twins"][sharp]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    before = L.az_nn_debug_flags()
    try:
        for B in (1, 3, 50):
            x, _, _ = _inputs(torch, B, 1400 + B)
            ys = []
            for flags in (0, LEGACY):
                y = torch.full_like(x, float("nan"))
                L.az_nn_debug(flags)
                assert L.az_nn_attn_block(x.data_ptr(), fast.pre_w.data_ptr(), fast.qkvg_w.data_ptr(), fast.qn_w.data_ptr(),
                                          fast.kn_w.data_ptr(), fast.o_w.data_ptr(), y.data_ptr(), B, 1e-5, None, s) == 0
                torch.cuda.synchronize()
                ys.append(y)
            assert torch.isfinite(ys[0].float()).all()
            assert torch.equal(ys[0].view(torch.int16), ys[1].view(torch.int16)), (B, sharp)
    finally:
        L.az_nn_debug(before)


def test_native_model_forward_positions(env):
    """az_nn_model_forward_positions on 3000 positions: all three outputs equal under the default and bit 8"""
    torch, L = env["torch"], env["L"]
    B = 3000
    p1, p2, turn, sym, mask = _positions(np.random.default_rng(31), B)
    dev = [torch.from_numpy(a).cuda() for a in (p1.view(np.int64), p2.view(np.int64), turn, sym, mask)]
    pos = env["Positions"](*[t.data_ptr() for t in dev[:4]])
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    fast = env["FastNet"].from_module(env["net"])
    model = fast.native_model()
    assert model is not None
    nb = int(L.az_nn_model_scratch_bytes(model, B))
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    before = L.az_nn_debug_flags()
    outs = []
    try:
        for flags in (0, LEGACY):
            out = [torch.full(shape, float("nan"), device="cuda") for shape in ((B, 7), (B, 3), (B,))]
            L.az_nn_debug(flags)
            assert L.az_nn_model_forward_positions(model, C.byref(pos), dev[4].data_ptr(), *[t.data_ptr() for t in out], B, None, None,
                                                   scratch.data_ptr(), nb, s) == 0
            torch.cuda.synchronize()
            outs.append(out)
    finally:
        L.az_nn_debug(before)
    for t in outs[0]:
        assert torch.isfinite(t).all()
    _same_bytes(torch, outs[0], outs[1], "model, bit 8")
