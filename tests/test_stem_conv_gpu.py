"""az_nn_stem_conv_block_positions (nn_conv.hip): the folded stem and the first residual block as one kernel, against
the two launches it replaces (az_nn_stem_folded_positions + az_nn_conv_block), inside the native model object
(AZ_STEM_FUSED=1 against =0) and under bench.py.  The fused kernel runs the arithmetic of the two kernels with the same
rounding points and has no atomics, so every comparison here is bit for bit."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_oracle_golden import load

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")

BATCHES = (1, 3, 777, 4099, 26368)
COMPACT = ((9, 5), (4099, 3001), (26368, 20000))


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
    return dict(torch=torch, net=net, FastNet=FastConnect4Net, Positions=Positions, L=L)


def _wins(bb):
    """four in a row somewhere on a bitboard (bit = 7 * column + height)"""
    out = np.zeros(bb.shape, dtype=bool)
    for d in (1, 7, 6, 8):
        m = bb & (bb >> np.uint64(d))
        out |= (m & (m >> np.uint64(2 * d))) != 0
    return out


def _positions(rng, n):
    """n random legal Connect4 positions of all ages (0 .. 42 stones, games stop at a win), both sides to move, under
    both symmetry ids: bitboards of player +1 / -1, side to move, symmetry id, legal-column mask in the shown frame"""
    bb = np.zeros((2, n), dtype=np.uint64)
    height = np.zeros((n, 7), dtype=np.int64)
    plies = np.zeros(n, dtype=np.int64)
    target = rng.integers(0, 43, n)
    over = np.zeros(n, dtype=bool)
    for _ in range(42):
        open_ = height < 6
        act = (plies < target) & ~over & open_.any(1)
        if not act.any():
            break
        score = rng.random((n, 7)) + open_                      # a random column among the open ones
        col = score.argmax(1)
        bit = (np.uint64(1) << (7 * col + height[np.arange(n), col]).astype(np.uint64))
        side = plies & 1                                         # player +1 moves first
        for s in (0, 1):
            sel = act & (side == s)
            bb[s, sel] |= bit[sel]
            over[sel] |= _wins(bb[s, sel])
        height[np.arange(n)[act], col[act]] += 1
        plies += act
    turn = np.where(plies % 2 == 0, 1, -1).astype(np.int32)
    sym = rng.integers(0, 2, n).astype(np.int32)
    legal = height < 6
    mask = np.where(sym[:, None] != 0, legal[:, ::-1], legal).astype(np.uint8)
    mask[~mask.any(1), 3] = 1                                    # a full board: the heads need one open column
    return bb[0], bb[1], turn, sym, np.ascontiguousarray(mask)


class _Pos:
    """positions on the device + the az_nn_positions that names them"""

    def __init__(self, env, rng, n):
        torch = env["torch"]
        p1, p2, turn, sym, mask = _positions(rng, n)
        self.p1 = torch.from_numpy(p1.view(np.int64)).cuda()
        self.p2 = torch.from_numpy(p2.view(np.int64)).cuda()
        self.turn, self.sym, self.mask = torch.from_numpy(turn).cuda(), torch.from_numpy(sym).cuda(), torch.from_numpy(mask).cuda()
        self.c = env["Positions"](self.p1.data_ptr(), self.p2.data_ptr(), self.turn.data_ptr(), self.sym.data_ptr())


def _bits(t):
    import torch
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32)


def _kernel_pair(env, fast, pos, B, rows=None, n_rows=None):
    """(fused, two launches): y of the same positions, both on a NaN canary"""
    torch, L = env["torch"], env["L"]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rp = None if rows is None else rows.data_ptr()
    npp = None if n_rows is None else n_rows.data_ptr()
    blk = [getattr(fast, n).data_ptr() for n in fast.res[0]]            # weight, bias, gamma, beta of the first block
    y_f = torch.full((B, 42, 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    y_s = torch.full_like(y_f, float("nan"))
    y_2 = torch.full_like(y_f, float("nan"))
    assert L.az_nn_stem_conv_block_positions(C.byref(pos.c), fast.stem_frag.data_ptr(), fast.stem_pmap.data_ptr(), *blk,
                                             y_f.data_ptr(), B, 1e-5, rp, npp, s) == 0
    assert L.az_nn_stem_folded_positions(C.byref(pos.c), fast.stem_frag.data_ptr(), fast.stem_pmap.data_ptr(), y_s.data_ptr(),
                                         B, rp, npp, s) == 0
    assert L.az_nn_conv_block(y_s.data_ptr(), 64, blk[0], blk[1], blk[2], blk[3], 1, y_2.data_ptr(), B, 1e-5, npp, s) == 0
    torch.cuda.synchronize()
    return y_f, y_2


def test_fused_kernel_equals_stem_then_block(env):
    torch = env["torch"]
    fast = env["FastNet"].from_module(env["net"])
    rng = np.random.default_rng(21)
    for B in BATCHES:
        pos = _Pos(env, rng, B)
        y_f, y_2 = _kernel_pair(env, fast, pos, B)
        assert torch.isfinite(y_f.float()).all(), B
        assert torch.equal(_bits(y_f), _bits(y_2)), B


def test_fused_kernel_compact_lists(env):
    """batch_dev < batch and a shuffled gather list: the first n_rows rows of y are those of the two launches, the NaN
    canary behind them is untouched; indices outside the batch - inside the list, where both forms read row 0 instead,
    and behind it, where nothing may be read at all - are never dereferenced"""
    torch = env["torch"]
    fast = env["FastNet"].from_module(env["net"])
    rng = np.random.default_rng(22)
    gen = torch.Generator(device="cuda").manual_seed(22)
    for B, live in COMPACT:
        pos = _Pos(env, rng, B)
        for wild in (False, True):
            rows = torch.randperm(B, device="cuda", generator=gen).to(torch.int32).contiguous()
            if wild:
                rows[live:] = 2 ** 31 - 1
                rows[0], rows[live // 2], rows[live - 1] = -7, B, 2 ** 31 - 1
            n_rows = torch.tensor([live], dtype=torch.int64, device="cuda")
            y_f, y_2 = _kernel_pair(env, fast, pos, B, rows, n_rows)
            assert torch.isfinite(y_f[:live].float()).all(), (B, live, wild)
            assert torch.isnan(y_f[live:].float()).all(), (B, live, wild)
            assert torch.equal(_bits(y_f), _bits(y_2)), (B, live, wild)
            if wild:                                     # an index outside the batch shows row 0
                zero = torch.zeros(1, dtype=torch.int32, device="cuda")
                one = torch.tensor([1], dtype=torch.int64, device="cuda")
                y_0, _ = _kernel_pair(env, fast, pos, B, zero, one)
                for k in (0, live // 2, live - 1):
                    assert torch.equal(_bits(y_f[k]), _bits(y_0[0])), (B, live, k)


def _models(env, **more):
    """the native model created under AZ_STEM_FUSED=1 and =0 (the knob is read when the object is created)"""
    out = {}
    names = ["AZ_STEM_FUSED"] + list(more)
    old = {k: os.environ.get(k) for k in names}
    try:
        os.environ.update(more)
        for knob in ("1", "0"):
            os.environ["AZ_STEM_FUSED"] = knob
            fast = env["FastNet"].from_module(env["net"])
            model = fast.native_model()
            assert model is not None
            out[knob] = (fast, model)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out


def _forward(env, model, pos, B, rows=None, n_rows=None):
    torch, L = env["torch"], env["L"]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    nb = int(L.az_nn_model_scratch_bytes(model, B))
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    outs = [torch.full(shape, float("nan"), device="cuda") for shape in ((B, 7), (B, 3), (B,))]
    rp = None if rows is None else rows.data_ptr()
    npp = None if n_rows is None else n_rows.data_ptr()
    assert L.az_nn_model_forward_positions(model, C.byref(pos.c), pos.mask.data_ptr(), *[t.data_ptr() for t in outs], B, rp, npp,
                                           scratch.data_ptr(), nb, s) == 0
    torch.cuda.synchronize()
    return outs


def test_native_model_fused_equals_two_launches(env):
    torch, L = env["torch"], env["L"]
    models = _models(env)
    rng = np.random.default_rng(23)
    gen = torch.Generator(device="cuda").manual_seed(23)
    cases = [(B, None) for B in BATCHES] + list(COMPACT)
    for B, live in cases:
        pos = _Pos(env, rng, B)
        rows = n_rows = None
        if live is not None:
            rows = torch.randperm(B, device="cuda", generator=gen).to(torch.int32).contiguous()
            n_rows = torch.tensor([live], dtype=torch.int64, device="cuda")
        a = _forward(env, models["1"][1], pos, B, rows, n_rows)
        b = _forward(env, models["0"][1], pos, B, rows, n_rows)
        listed = torch.ones(B, dtype=torch.bool, device="cuda")
        if live is not None:
            listed[:] = False
            listed[rows[:live].long()] = True
        for x, y in zip(a, b):
            assert torch.isfinite(x[listed]).all() and torch.isnan(x[~listed]).all(), (B, live)
            assert torch.equal(_bits(x), _bits(y)), (B, live)


def test_profiled_call_runs_the_two_launches(env):
    """A call that carries event pairs (az_nn_model_profile) runs the stem and the first block as two launches, so
    the STEM and CONV rings fill, and returns the same bits.  Such a call also runs the attention block and the heads
    as two launches, whose f32 summation order is not that of the fused az_nn_attn_heads (tests/test_attn_heads_gpu.py),
    so the comparison is made where that kernel is out of the picture: models created under AZ_ATTN_HEADS_FUSED=0,
    the profiled call of the stem-fused model against its own plain call and against the plain call of the
    AZ_STEM_FUSED=0 model."""
    torch, L = env["torch"], env["L"]
    models = _models(env, AZ_ATTN_HEADS_FUSED="0")
    rng = np.random.default_rng(24)
    for B in (3, 4099):
        pos = _Pos(env, rng, B)
        want = _forward(env, models["1"][1], pos, B)
        want0 = _forward(env, models["0"][1], pos, B)
        assert L.az_nn_model_profile(1) == 0
        try:
            got = _forward(env, models["1"][1], pos, B)
            ms, n = (C.c_double * 4)(), (C.c_int64 * 4)()
            assert L.az_nn_model_profile_read_kernels(C.byref(ms), C.byref(n)) == 0
        finally:
            L.az_nn_model_profile(0)
        for x, y, z in zip(got, want, want0):
            assert torch.isfinite(x).all()
            assert torch.equal(_bits(x), _bits(y)) and torch.equal(_bits(x), _bits(z)), B
        assert n[0] == 1 and n[1] == 1 and ms[0] > 0.0 and ms[1] > 0.0, (list(n), list(ms))      # AZ_NN_PROFILE_STEM, _CONV


def test_bench_outputs_equal_under_both_settings(tmp_path):
    """bench.py --gpus 1 --dump-outputs: what the last timed ply hands its caller, all eight arrays, with the fused
    kernel and with the two launches"""
    dumps = []
    for knob in ("1", "0"):
        out = tmp_path / knob
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--dump-outputs", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1200, cwd=ROOT, env=dict(os.environ, AZ_STEM_FUSED=knob))
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert lines and json.loads(lines[-1])["value"] > 0
        dumps.append({f.name[:-4]: np.load(out / f.name) for f in out.iterdir()})
    assert set(dumps[0]) == {"visit_counts", "actions", "bb_p1", "bb_p2", "turn", "done", "winner", "root_stats"}
    for k in dumps[0]:
        assert np.array_equal(dumps[0][k], dumps[1][k]), k
