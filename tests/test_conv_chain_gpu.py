"""az_nn_stem_conv_chain_positions (nn_conv.hip, k_conv_chain): the stem block and the residual blocks behind it as one
launch, against the launches it replaces run in sequence in the same process - az_nn_stem_conv_block_positions, then
az_nn_conv_block twice - which tests/test_conv_slots_gpu.py and tests/test_stem_conv_gpu.py pin to recorded bytes.  Every
layer of the chain is the text of its own kernel, so every comparison is byte for byte, on BOTH scratch tensors (the
final one and the one the middle block wrote), each filled with a NaN canary first.

    free grid            batch 1, 3, 4, 5        a partial tile; one tile; one full + one partial: workgroups with a single
                                                 tile cross the layer switch
                         batch 13, batch_dev 9   gather list with one index outside the rows; rows 9.. keep the canary in
                                                 both tensors
    AZ_NN_CONV_GRID=1    batch 13                four tiles in one workgroup: both raw-buffer parities in front of a switch,
                                                 a layer's first tile staged into buffer 0 after an odd number of tiles
    AZ_NN_CONV_GRID=2    batch 17                workgroups with 3 and 2 tiles reach the switch at different times
    model                13 positions            az_nn_model_forward_positions under AZ_CONV_CHAIN=0 and the default

Inputs and bf16 weights come from a numpy seed (tools/record_conv_golden.py's generators); sample 0 is shown mirrored.
AZ_NN_CONV_GRID is read once per process, so the capped grids run in child processes - this file as a script - and so do
the two model runs, each under its own AZ_CONV_CHAIN."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_conv_golden as R  # noqa: E402

SEED = 2901
N_BLOCKS = 3
CANARY = 0x7FC0                                     # bf16 NaN as torch.full writes it
FREE = (1, 3, 4, 5)
LIVE = 9                                            # the compact case: 9 of 13


def make_inputs(batch, compact):
    """every host array of one case, from SEED, the batch and the form alone"""
    rng = np.random.default_rng([SEED, batch, int(compact)])
    d = {}
    d["p1"], d["p2"], d["turn"], d["sym"], _ = R.positions(rng, batch)
    d["sym"][0] = 1                                 # a mirrored sample in every case
    d["frag"] = R._bf16(rng.standard_normal((2, 4, 64, 8)) * 0.25)
    pmap = np.zeros((48, 68), dtype=np.float32)
    pmap[:R.CELLS, :64] = rng.standard_normal((R.CELLS, 64))
    d["pmap"] = pmap
    for i in range(N_BLOCKS):
        d["w%d" % i] = R._bf16(rng.standard_normal((64, 3, 3, 64)) * 0.06)
        d["bias%d" % i] = R._bf16(rng.standard_normal(64) * 0.1)
        d["gamma%d" % i] = R._bf16(1.0 + 0.3 * rng.standard_normal(64))
        d["beta%d" % i] = R._bf16(0.2 * rng.standard_normal(64))
    if compact:
        d["live"] = np.array([LIVE], dtype=np.int64)
        rows = rng.permutation(batch).astype(np.int32)
        rows[4] = batch + 3                         # outside the rows: shows row 0
        rows[LIVE:] = 2 ** 31 - 1                   # behind the list: never read
        d["rows"] = rows
    return d


def run_kernels(batch, compact=False):
    """(final, other) scratch tensors as uint16 (batch, 42, 64): of the separate launches, then of the chain"""
    import torch  # (before the engine library: one HIP runtime per process)
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src.fast_net import Positions, glue
    L = glue()
    assert L is not None, "no library in " + PKG
    host = make_inputs(batch, compact)
    assert (host["sym"] != 0).any()
    dev = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int16) if v.dtype == np.uint16 else v).cuda()
           for k, v in host.items()}
    ptr = lambda k: dev[k].data_ptr() if k in dev else None
    pos = Positions(ptr("p1"), ptr("p2"), ptr("turn"), ptr("sym"))
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    canary = lambda: torch.full((batch, R.CELLS, 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    blk = lambda i: [ptr("%s%d" % (n, i)) for n in ("w", "bias", "gamma", "beta")]
    # the reference: three launches, ping-pong between two tensors (N_BLOCKS odd: the result is in the first)
    a, b = canary(), canary()
    assert L.az_nn_stem_conv_block_positions(C.byref(pos), ptr("frag"), ptr("pmap"), *blk(0), a.data_ptr(), batch, 1e-5,
                                             ptr("rows"), ptr("live"), s) == 0
    x, y = a, b
    for i in range(1, N_BLOCKS):
        assert L.az_nn_conv_block(x.data_ptr(), 64, *blk(i), 1, y.data_ptr(), batch, 1e-5, ptr("live"), s) == 0
        x, y = y, x
    torch.cuda.synchronize()
    # the chain
    ca, cb = canary(), canary()
    arr = lambda n: (C.c_void_p * N_BLOCKS)(*[ptr("%s%d" % (n, i)) for i in range(N_BLOCKS)])
    assert L.az_nn_stem_conv_chain_positions(C.byref(pos), ptr("frag"), ptr("pmap"), N_BLOCKS, arr("w"), arr("bias"), arr("gamma"),
                                             arr("beta"), ca.data_ptr(), cb.data_ptr(), batch, 1e-5, ptr("rows"), ptr("live"), s) == 0
    torch.cuda.synchronize()
    bits = lambda t: t.view(torch.int16).cpu().numpy().view(np.uint16)
    return {"ref_final": bits(a), "ref_other": bits(b), "got_final": bits(ca), "got_other": bits(cb)}


def run_model():
    """probs, wdl, moves_left of 13 positions from the native model, created under this process's AZ_CONV_CHAIN"""
    import torch
    for p in (ROOT, PKG):
        if p not in sys.path:
            sys.path.insert(0, p)
    from src import az_net
    from src.fast_net import FastConnect4Net, Positions, glue
    from test_oracle_golden import load
    wts = load("g7_checkpoint_weights")
    net = az_net.Connect4Net(device="cuda").eval()
    az_net.load_reference_weights(net, {k: wts[k] for k in wts.files})
    L = glue()
    fast = FastConnect4Net.from_module(net)         # owns the weight tensors and the model object: alive to the end
    model = fast.native_model()
    assert model is not None
    batch = 13
    host = make_inputs(batch, False)
    dev = {k: torch.from_numpy(host[k].view(np.int64) if host[k].dtype == np.uint64 else host[k]).cuda() for k in ("p1", "p2", "turn", "sym")}
    pos = Positions(*[dev[k].data_ptr() for k in ("p1", "p2", "turn", "sym")])
    mask = torch.ones((batch, 7), dtype=torch.uint8, device="cuda")
    nb = int(L.az_nn_model_scratch_bytes(model, batch))
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    outs = [torch.full(shape, float("nan"), device="cuda") for shape in ((batch, 7), (batch, 3), (batch,))]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.az_nn_model_forward_positions(model, C.byref(pos), mask.data_ptr(), *[t.data_ptr() for t in outs], batch, None, None,
                                           scratch.data_ptr(), nb, s) == 0
    torch.cuda.synchronize()
    res = {k: t.cpu().numpy().view(np.uint32) for k, t in zip(("probs", "wdl", "moves_left"), outs)}
    del fast
    return res


def _child(args, **env):
    """this file as a script in a child process with `env` changed (None: removed); the arrays it wrote"""
    e = dict(os.environ)
    for k, v in env.items():
        e.pop(k, None)
        if v is not None:
            e[k] = v
    with tempfile.TemporaryDirectory() as tmp:
        raw = os.path.join(tmp, "raw.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args + ["--raw", raw], env=e, capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-3000:]
        with np.load(raw) as z:
            return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()


def _same(res, batch, live=None):
    assert res["ref_final"].shape == (batch, R.CELLS, 64)
    n = batch if live is None else live
    for k in ("ref_final", "ref_other", "got_final", "got_other"):
        assert (res[k][:n] != CANARY).any(axis=(1, 2)).all(), (k, "a listed row was not written")
        assert (res[k][n:] == CANARY).all(), (k, "a row past the batch was written")
    assert np.array_equal(res["got_final"], res["ref_final"]), "the final tensor"
    assert np.array_equal(res["got_other"], res["ref_other"]), "the middle block's tensor"


@pytest.mark.parametrize("batch", FREE)
def test_chain_equals_the_three_launches(built, batch):
    free = "AZ_NN_CONV_GRID" not in os.environ
    res = run_kernels(batch) if free else _child(["--kernels", str(batch)], AZ_NN_CONV_GRID=None)
    _same(res, batch)


def test_compact_batch_keeps_the_canary(built):
    """batch 13, 9 listed, one index outside the rows (both forms show row 0 there, pinned by test_stem_conv_gpu.py) and
    2^31 - 1 behind the list: rows 9 .. 12 of BOTH tensors are untouched"""
    free = "AZ_NN_CONV_GRID" not in os.environ
    res = run_kernels(13, True) if free else _child(["--kernels", "13", "--compact"], AZ_NN_CONV_GRID=None)
    _same(res, 13, LIVE)


@pytest.mark.parametrize("grid,batch", [("1", 13), ("2", 17)])
def test_capped_grid(built, grid, batch):
    _same(_child(["--kernels", str(batch)], AZ_NN_CONV_GRID=grid), batch)


def test_model_equal_with_and_without_the_chain(built):
    off = _child(["--model"], AZ_CONV_CHAIN="0", AZ_NN_CONV_GRID=None)
    on = _child(["--model"], AZ_CONV_CHAIN=None, AZ_NN_CONV_GRID=None)
    assert set(on) == {"probs", "wdl", "moves_left"}
    for k in on:
        assert np.isfinite(on[k].view(np.float32)).all(), k
        assert np.array_equal(on[k], off[k]), k


if __name__ == "__main__":
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", type=int, metavar="BATCH")
    ap.add_argument("--compact", action="store_true")
    ap.add_argument("--model", action="store_true")
    ap.add_argument("--raw", required=True)
    a = ap.parse_args()
    np.savez(a.raw, **(run_model() if a.model else run_kernels(a.kernels, a.compact)))
