"""The Connect4 stem's training forward and backward on the device (k_stem_fold, k_stem_fwd, k_stem_bwd, k_stem_reduce,
k_stem_unfold: az_train_dev_stem_fwd / _bwd in include/az_train.h, `stem` and `adopt_stem` in src/train_stem.py).

The kernels are held against the float64 restatement of the DIRECT form in tests/train_stem_ref.py on the same inputs.
Allowed deviation per quantity - y, dW, db, dE, dP: largest absolute difference over the quantity's largest magnitude - is
the larger of
    4 x the deviation of float32 torch (CPU) from the restatement on the same inputs, and
    1e-6;
the factor 4 covers a different but equally legitimate summation order.  float32 torch's own deviations on these inputs
are printed by tests/test_train_stem_cpu.py (1e-7 to 1.3e-6).  Measured on an MI355X: no case needed more than 0.42 of
its bound (db at N = 2).

Through the C ABI y, the four gradients and the workspace each sit between guard regions of 256 bytes; the guards and
every input are compared exactly afterwards, the table at the workspace's head is the same bytes after the backward as
after the forward, and every call runs twice from the same start and must give the same bytes.

1. N = 1, 2, 7, 65 with max_workgroups 0, 2 and 3 (an empty board in each batch of two or more); N = 257 under the default
   cap (two samples per workgroup);
2. planes are multipliers: 0.5 and -2, a cell with both planes at 1; garbage in plane 2 changes no byte;
3. stones on columns 0 and 6 only, with dy on column 0, column 6 or row 0 only: dW exactly zero at the taps that read
   outside the board; no opponent stone: d_piece_emb[1] exactly zero;
4. the AZ_ERR_ARG cases;
5. `stem` kernel route against the torch route, a non-contiguous upstream gradient, no_grad;
6. `adopt_stem`, alone and with `adopt_blocks` + `adopt_attention`, through three `train_step` batches against an
   unadopted twin and the float64 net; with all three adopted the first block gets a contiguous image."""
import ctypes as C
import functools

import numpy as np
import pytest

import train_gpu_harness as H
import train_loss_ref as TR
import train_stem_ref as R
from train_gpu_harness import AZ_ERR_ARG, Slab, fields, loaders, swap

pytestmark = pytest.mark.gpu

TABLE_BYTES = 15360
ROW_BYTES = 3840 * 4
INPUTS = ("state",) + R.PARAMS + ("dy",)
GRADS = ("dE", "dP", "dW", "db")
OUTPUTS = R.QUANTITIES + ("ws",)


@pytest.fixture(scope="module")
def env():
    return H.load_env(("az_net", "optim", "train_attn", "train_block", "train_loss", "train_stem"))


def structs(env, slab):
    abi = env["abi"]
    params = abi.TrainStemParamsC(*(slab.ptr(k) for k in R.PARAMS))
    grads = abi.TrainStemGradsC(*(slab.ptr(k) for k in GRADS), slab.ptr("ws"), slab.size["ws"])
    return params, grads


def make_slab(env, d, max_workgroups):
    n = d["state"].shape[0]
    ws = env["L"].az_train_stem_workspace_bytes(n, max_workgroups)
    assert ws > 0 and ws % 16 == 0
    out = dict(y=n * R.CH * R.CELLS * 4, **{"d" + k: d[k].nbytes for k in R.PARAMS}, ws=ws)
    return Slab(env["torch"], {k: d[k] for k in INPUTS}, out)


def run_stem(env, d, max_workgroups):
    """Forward and backward through the C ABI, twice from the same start -> the five quantities."""
    torch, L, abi = env["torch"], env["L"], env["abi"]
    n = d["state"].shape[0]
    slab = make_slab(env, d, max_workgroups)
    params, grads = structs(env, slab)
    images = []
    for _ in range(2):
        slab.upload()
        torch.cuda.synchronize()
        abi.check(L.az_train_dev_stem_fwd(C.byref(params), slab.ptr("state"), n, slab.ptr("y"), slab.ptr("ws"), slab.size["ws"],
                                          abi._stream()))
        torch.cuda.synchronize()
        image = slab.dev.cpu().numpy()
        assert slab.untouched_outside(image, ("y", "ws")), "the forward wrote outside y and the workspace"
        at = slab.at["ws"]
        table = image[at:at + TABLE_BYTES].copy()
        assert np.array_equal(image[at + TABLE_BYTES:at + slab.size["ws"]], slab.host[at + TABLE_BYTES:at + slab.size["ws"]]), \
            "the forward wrote past the table"
        abi.check(L.az_train_dev_stem_bwd(C.byref(params), slab.ptr("state"), slab.ptr("ws"), slab.ptr("dy"), n, max_workgroups,
                                          C.byref(grads), abi._stream()))
        torch.cuda.synchronize()
        image = slab.dev.cpu().numpy()
        assert slab.untouched_outside(image, OUTPUTS), "a guard region or an input was written"
        assert np.array_equal(image[at:at + TABLE_BYTES], table), "the backward wrote the table"
        images.append(image)
    assert np.array_equal(images[0], images[1]), "two calls on the same inputs differ"
    shapes = dict(y=(n, R.CH, R.ROWS, R.COLS), **{"d" + k: d[k].shape for k in R.PARAMS})
    got = {k: slab.get(images[0], k, s) for k, s in shapes.items()}
    assert all(np.isfinite(v).all() for v in got.values())
    return got


held = functools.partial(H.held, R)


# ---------------------------------------------------------------------------------------- 1. sizes and caps

@pytest.mark.parametrize("n", R.GPU_N)
def test_stem_through_the_c_abi(env, n):
    d, ref, own = R.inputs(n), R.reference(n), R.torch_deviations(n)
    assert n == 1 or (not d["state"][-1, :2].any() and d["state"][0, :2].any())
    first = None
    for cap in (0, 2, 3):
        got = run_stem(env, d, cap)
        held(got, ref, own, "N=%d cap=%d" % (n, cap))
        if first is None:
            first = got
        else:
            assert np.array_equal(got["y"], first["y"])     # what does not go through the partial rows does not depend on the cap


def test_default_cap_with_several_samples_per_workgroup(env):
    """N = 257 under the default cap of 256 workgroups: 129 of them walk two samples (the last one one), so the
    accumulators a workgroup keeps in registers across its samples and the 129-row sum are held on the path `adopt_stem`
    takes."""
    n = R.DEFAULT_CAP + 1
    d, ref, own = R.inputs(n), R.reference(n), R.torch_deviations(n)
    assert env["L"].az_train_stem_workspace_bytes(n, 0) == TABLE_BYTES + (1 + 129) * ROW_BYTES
    held(run_stem(env, d, 0), ref, own, "N=%d default cap" % n)


# ---------------------------------------------------------------------------------------- 2. planes are multipliers

def test_planes_are_multipliers_and_plane_two_is_not_read(env):
    d = R.multiplier_inputs()
    ref, own = R.case_reference("multipliers")
    got = run_stem(env, d, 0)
    held(got, ref, own, "multipliers")
    rng = np.random.default_rng(2)
    garbage = d["state"].copy()
    garbage[:, 2] = rng.standard_normal((7, R.ROWS, R.COLS)).astype(np.float32) * 1e30
    garbage[0, 2, 0, 0], garbage[1, 2, 0, 0] = np.nan, np.inf
    other = run_stem(env, dict(d, state=garbage), 0)
    for q in R.QUANTITIES:
        assert np.array_equal(got[q], other[q]), q


# ---------------------------------------------------------------------------------------- 3. padding and exact zeros

@pytest.mark.parametrize("which", ("col0", "col6", "row0", "plane1"))
def test_taps_outside_the_board_contribute_exact_zeros(env, which):
    d = R.padding_inputs(which)
    ref, own = R.case_reference(which)
    for cap in (0, 1):
        got = run_stem(env, d, cap)
        held(got, ref, own, "%s cap=%d" % (which, cap))
        zero, rest = R.exact_zeros(which, got)
        assert not zero.any() and rest.any(), which


# ---------------------------------------------------------------------------------------- 4. argument errors

def test_argument_errors_enqueue_and_write_nothing(env):
    torch, L = env["torch"], env["L"]
    d = R.inputs(7)
    n = 7
    slab = make_slab(env, d, 0)

    params, grads = structs(env, slab)

    def fwd(**kw):
        a = dict(params=params, state=slab.ptr("state"), n=n, y=slab.ptr("y"), ws=slab.ptr("ws"), size=slab.size["ws"])
        a.update(kw)
        return L.az_train_dev_stem_fwd(None if a["params"] is None else C.byref(a["params"]), a["state"], a["n"], a["y"], a["ws"],
                                       a["size"], None)

    def bwd(**kw):
        a = dict(params=params, state=slab.ptr("state"), table=slab.ptr("ws"), dy=slab.ptr("dy"), n=n, cap=0, grads=grads)
        a.update(kw)
        return L.az_train_dev_stem_bwd(None if a["params"] is None else C.byref(a["params"]), a["state"], a["table"], a["dy"], a["n"],
                                       a["cap"], None if a["grads"] is None else C.byref(a["grads"]), None)

    bad = []
    # null required pointers
    bad += [fwd(params=None), fwd(state=None), fwd(y=None), fwd(ws=None)]
    bad += [bwd(params=None), bwd(state=None), bwd(table=None), bwd(dy=None), bwd(grads=None)]
    bad += [f(params=swap(params, **{k: None})) for f in (fwd, bwd) for k in fields(params)]
    bad += [bwd(grads=swap(grads, **{k: None})) for k in fields(grads) if k != "workspace_bytes"]
    # 16-byte alignment (y, dy, the table, the workspace); 4-byte for the rest
    bad += [fwd(y=slab.ptr("y", 8)), fwd(ws=slab.ptr("ws", 4)), bwd(dy=slab.ptr("dy", 4)), bwd(table=slab.ptr("ws", 8)),
            bwd(grads=swap(grads, workspace=slab.ptr("ws", 4)))]
    bad += [fwd(state=slab.ptr("state", 2)), bwd(state=slab.ptr("state", 1)), fwd(params=swap(params, piece_emb=slab.ptr("E", 2))),
            fwd(params=swap(params, pos_emb=slab.ptr("P", 1))), bwd(params=swap(params, conv_weight=slab.ptr("W", 3))),
            bwd(params=swap(params, conv_bias=slab.ptr("b", 2))), bwd(grads=swap(grads, d_piece_emb=slab.ptr("dE", 2))),
            bwd(grads=swap(grads, d_pos_emb=slab.ptr("dP", 3))), bwd(grads=swap(grads, d_conv_weight=slab.ptr("dW", 1))),
            bwd(grads=swap(grads, d_conv_bias=slab.ptr("db", 2)))]
    # N, the cap, the workspace
    bad += [fwd(n=0), fwd(n=-1), fwd(n=2 ** 30 + 1), bwd(n=0), bwd(n=-3), bwd(n=2 ** 30 + 1)]
    bad += [fwd(size=TABLE_BYTES - 4), fwd(size=0), fwd(size=-1)]
    bad += [bwd(cap=-1), bwd(grads=swap(grads, workspace_bytes=slab.size["ws"] - 4)), bwd(grads=swap(grads, workspace_bytes=0))]
    assert bad == [AZ_ERR_ARG] * len(bad), bad
    size = L.az_train_stem_workspace_bytes
    assert size(1, 0) == TABLE_BYTES + 2 * ROW_BYTES
    assert size(0, 0) == -1 and size(7, -1) == -1 and size(2 ** 30 + 1, 0) == -1
    assert size(65, 3) == size(7, 3) == TABLE_BYTES + 4 * ROW_BYTES
    assert size(7, 0) == size(7, 100) == TABLE_BYTES + 8 * ROW_BYTES
    assert size(5000, 0) == TABLE_BYTES + 251 * ROW_BYTES and size(5000, 4000) == TABLE_BYTES + 1001 * ROW_BYTES
    torch.cuda.synchronize()
    assert np.array_equal(slab.dev.cpu().numpy(), slab.host), "a refused call wrote"
    # a 4-byte aligned state or parameter is taken; the forward needs no more than the table's bytes
    assert fwd(size=TABLE_BYTES) == 0 and fwd(state=slab.ptr("state", 4), n=6) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------- 5. stem

def test_stem_kernel_route_against_the_torch_route(env, monkeypatch):
    torch, TS = env["torch"], env["TS"]
    n = 7
    d, ref, own = R.inputs(n), R.reference(n), R.torch_deviations(n)
    state = torch.from_numpy(d["state"].copy()).cuda()
    results = {}
    for route in ("kernel", "torch"):
        t = [torch.from_numpy(d[k].copy()).cuda().requires_grad_(True) for k in R.PARAMS]
        y = TS.stem(state, *t, route=route)
        assert y.shape == (n, 64, 6, 7) and y.is_contiguous() == (route == "kernel")
        # the upstream gradient as a view that is not contiguous
        dy = torch.from_numpy(np.ascontiguousarray(d["dy"].transpose(0, 2, 3, 1))).cuda().permute(0, 3, 1, 2)
        assert not dy.is_contiguous()
        y.backward(dy)
        assert all(p.grad is not None and p.grad.shape == p.shape for p in t)
        results[route] = dict(y=y.detach().cpu().numpy(), **{"d" + k: p.grad.cpu().numpy() for k, p in zip(R.PARAMS, t)})
    held(results["kernel"], ref, own, "stem kernel")
    gpu_torch = R.deviations(results["torch"], ref)
    for q in R.QUANTITIES:
        print("stem torch route on the GPU %-3s %.3e" % (q, gpu_torch[q]))
        # each within the bound of the other's reference: the two float32 routes differ by no more than both bounds
        assert R.dev(results["kernel"][q], results["torch"][q]) <= R.bound(own[q]) + max(gpu_torch[q], R.FLOOR)
    # the default route of CUDA tensors is the kernel's; under no_grad, or with no parameter that needs one, only the forward runs
    t = [torch.from_numpy(d[k].copy()).cuda() for k in R.PARAMS]
    applied = []
    apply = TS._Stem.apply
    monkeypatch.setattr(TS._Stem, "apply", staticmethod(lambda *a: applied.append(1) or apply(*a)))
    y = TS.stem(state, *t)
    assert applied == [] and y.grad_fn is None and np.array_equal(y.cpu().numpy(), results["kernel"]["y"])
    t[2].requires_grad_(True)
    with torch.no_grad():
        y = TS.stem(state, *t)
    assert applied == [] and y.grad_fn is None and not y.requires_grad, "under no_grad nothing is saved"
    assert np.array_equal(y.cpu().numpy(), results["kernel"]["y"])
    y = TS.stem(state, *t, max_workgroups=3)
    assert applied == [1] and y.grad_fn is not None
    y.backward(torch.from_numpy(d["dy"]).cuda())
    assert R.dev(t[2].grad.cpu().numpy(), ref["dW"]) <= R.bound(own["dW"])
    with pytest.raises(ValueError, match="one device"):
        TS.stem(state, t[0].cpu(), *t[1:])
    with pytest.raises(ValueError, match="contiguous"):
        TS.stem(state.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2), *t)
    with pytest.raises(ValueError, match="float32"):
        TS.stem(state.half(), *t)


# ---------------------------------------------------------------------------------------- 6. adopt_stem under train_step

def module(env, dtype, device, stem, others):
    return H.module(env, dtype, device, ("blocks", "attention") * others + ("stem",) * stem, stem_bias=True)


@pytest.fixture(scope="module")
def baselines(env):
    """The unadopted float32 twin on the GPU and the float64 net on the CPU, run once for both cases."""
    return H.baselines(env, stem_bias=True)


@pytest.mark.parametrize("others", (False, True))
def test_adopted_stem_under_train_step(env, baselines, others, monkeypatch):
    """Three `train_step` batches of 64 rows of fixture G16's Connect4 batch: a module with its stem adopted (and, in the
    second case, its residual blocks and attention block too) against an unadopted twin of the same seed, both float32 on
    the GPU with the kernel loss route.  Float64 figures: the same net in double on the CPU with the torch loss route; the
    adopted module may deviate from them by 4 x what the twin does, or 1e-6."""
    torch, TL, TS = env["torch"], env["TL"], env["TS"]
    twin_values, exact_values = baselines["twin"], baselines["exact"]
    net = module(env, torch.float32, "cuda", True, others)
    seen = []
    stem = TS.stem

    def watched(*a, **kw):
        y = stem(*a, **kw)
        seen.append((y.is_contiguous(), y.grad_fn is not None))
        return y
    monkeypatch.setattr(TS, "stem", watched)
    values = TL.train_step(net, loaders(env)["cuda"], lambda b: b, n_epochs=1, route="kernel", **dict(TR.CONFIGS["b"]))
    assert len(seen) == 4 and all(c for c, _ in seen), "the first block receives a contiguous image"
    assert [g for _, g in seen] == [True, True, True, False], "three training batches, then one forward under no_grad"
    figures = []
    for i, what in ((0, "policy loss"), (1, "value loss"), (2, "aux loss"), (4, "grad norm")):
        exact = exact_values[i]
        dev, own = (abs(v[i] - exact) / abs(exact) for v in (values, twin_values))
        print("train_step others=%d %-11s exact %.9g  adopted %.3e  twin %.3e  bound %.3e" % (others, what, exact, dev, own, R.bound(own)))
        figures.append((what, dev, own))
    for what, dev, own in figures:
        assert dev <= R.bound(own), (what, dev, own)
    assert all(p.grad is not None for p in net.parameters())
    # restored, the module is the class's own again: its eval outputs are a fresh twin's forward on the same parameters
    assert TS.restore_stem(net) == 1
    if others:
        assert env["TB"].restore_blocks(net) == 3 and env["TA"].restore_attention(net) == 1
    other = module(env, torch.float32, "cuda", False, False)
    other.load_state_dict(net.state_dict())
    with torch.no_grad():
        a, b = (m.eval()(loaders(env)["cuda"][0][0]) for m in (net, other))
    assert all(torch.equal(x, y) for x, y in zip(a, b))
