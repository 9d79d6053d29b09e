"""The residual block's training forward and backward on the device (k_block_fwd, k_block_bwd, k_block_reduce:
az_train_dev_block_fwd / _bwd in include/az_train.h, `residual_block` and `adopt_blocks` in src/train_block.py).

The kernels are held against the float64 restatement of tests/train_block_ref.py on the same inputs.  Allowed deviation
per quantity - y, dx, dgamma, dbeta, dW, db: largest absolute difference over the quantity's largest magnitude - is the
larger of
    4 x the deviation of float32 torch (CPU) from the restatement on the same inputs, and
    1e-6;
the factor 4 covers a different but equally legitimate summation order over the 576-term and N * 42-term sums.  float32
torch's own deviations on these inputs are printed by tests/test_train_block_cpu.py (N = 65: y 2.9e-7, dx 2.0e-7,
dgamma 2.9e-7, dbeta 3.7e-7, dW 1.5e-6, db 5.6e-7).

Through the C ABI y, the saved tensors, dx, the four parameter gradients and the workspace each sit between guard
regions of 256 bytes; the guards and every input are compared exactly afterwards, and every call runs twice from the
same start and must give the same bytes.

1. N = 1, 2, 7, 65 with max_workgroups 0, 2 and 3, keep null and keep with whole channels at 0, one all-zero sample;
   N = 257 under the default cap (two samples per workgroup);
2. padding: columns 0 and 6, taps kx = 0 and kx = 2, exact zeros in dW;
3. a forward with null save pointers gives the same y;
4. the AZ_ERR_ARG cases;
5. `residual_block` kernel route against the torch route, a non-contiguous upstream gradient, no_grad;
6. `adopt_blocks` on the Connect4 module through three `train_step` batches against an unadopted twin;
7. a block with dropout 0.2."""
import ctypes as C
import functools

import numpy as np
import pytest

import train_block_ref as R
import train_gpu_harness as H
import train_loss_ref as TR
from train_gpu_harness import AZ_ERR_ARG, Slab, fields, swap

pytestmark = pytest.mark.gpu

INPUTS = ("x", "gamma", "beta", "W", "b", "keep", "dy")
OUTPUTS = ("y", "z", "stats", "dx", "dgamma", "dbeta", "dW", "db", "ws")


@pytest.fixture(scope="module")
def env():
    return H.load_env(("az_net", "optim", "train_block", "train_loss"))


def structs(env, slab):
    abi = env["abi"]
    params = abi.TrainBlockParamsC(slab.ptr("gamma"), slab.ptr("beta"), slab.ptr("W"), slab.ptr("b"))
    saved = abi.TrainBlockSavedC(slab.ptr("z"), slab.ptr("stats"))
    grads = abi.TrainBlockGradsC(slab.ptr("dx"), slab.ptr("dgamma"), slab.ptr("dbeta"), slab.ptr("dW"), slab.ptr("db"), slab.ptr("ws"),
                                 slab.size["ws"])
    return params, saved, grads


def make_slab(env, d, max_workgroups):
    n, ch = d["x"].shape[:2]
    ws = env["L"].az_train_block_workspace_bytes(n, max_workgroups)
    assert ws > 0 and ws % 16 == 0
    act = d["x"].nbytes
    out = dict(y=act, z=act, stats=8 * n, dx=act, dgamma=4 * ch, dbeta=4 * ch, dW=d["W"].nbytes, db=4 * ch, ws=ws)
    return Slab(env["torch"], {k: d[k] for k in INPUTS}, out)


def run_block(env, d, max_workgroups):
    """Forward and backward through the C ABI, twice from the same start -> the quantities and the saved tensors."""
    torch, L, abi = env["torch"], env["L"], env["abi"]
    n = d["x"].shape[0]
    slab = make_slab(env, d, max_workgroups)
    params, saved, grads = structs(env, slab)
    images = []
    for _ in range(2):
        slab.upload()
        torch.cuda.synchronize()
        abi.check(L.az_train_dev_block_fwd(C.byref(params), slab.ptr("x"), slab.ptr("keep"), n, R.EPS, slab.ptr("y"),
                                           C.byref(saved), abi._stream()))
        torch.cuda.synchronize()
        image = slab.dev.cpu().numpy()
        assert slab.untouched_outside(image, ("y", "z", "stats")), "the forward wrote outside y, z and stats"
        abi.check(L.az_train_dev_block_bwd(C.byref(params), slab.ptr("x"), slab.ptr("keep"), slab.ptr("dy"), C.byref(saved), n,
                                           max_workgroups, C.byref(grads), abi._stream()))
        torch.cuda.synchronize()
        image = slab.dev.cpu().numpy()
        assert slab.untouched_outside(image, OUTPUTS), "a guard region or an input was written"
        images.append(image)
    assert np.array_equal(images[0], images[1]), "two calls on the same inputs differ"
    shapes = dict(y=d["x"].shape, z=d["x"].shape, stats=(n, 2), dx=d["x"].shape, dgamma=d["gamma"].shape, dbeta=d["beta"].shape,
                  dW=d["W"].shape, db=d["b"].shape)
    got = {k: slab.get(images[0], k, s) for k, s in shapes.items()}
    assert all(np.isfinite(v).all() for v in got.values())
    return got


held = functools.partial(H.held, R)


# ---------------------------------------------------------------------------------------- 1. sizes, caps, keep

@pytest.mark.parametrize("keep_p", (R.KEEP_P, 0.0))
@pytest.mark.parametrize("n", R.GPU_N)
def test_block_through_the_c_abi(env, n, keep_p):
    d, ref, own = R.inputs(n, keep_p=keep_p), R.reference(n, keep_p), R.torch_deviations(n, keep_p)
    assert not d["x"][-1].any() and (d["keep"] is None) == (keep_p == 0.0)
    first = None
    for cap in (0, 2, 3):
        got = run_block(env, d, cap)
        held(got, ref, own, "N=%d keep_p=%.1f cap=%d" % (n, keep_p, cap))
        # what the forward saves: z and (mean, rstd), the all-zero sample's rstd 1 / sqrt(eps)
        assert R.dev(got["z"], ref["z"]) <= R.bound(own["y"])
        assert np.allclose(got["stats"][:, 0], ref["mean"], rtol=0, atol=1e-6) and np.allclose(got["stats"][:, 1], ref["rstd"], rtol=2e-6, atol=0)
        assert got["stats"][-1, 0] == 0.0 and got["stats"][-1, 1] == pytest.approx(1 / np.sqrt(R.EPS), rel=1e-6)
        if d["keep"] is not None:
            dropped = d["keep"] == 0
            assert np.array_equal(got["y"][dropped], d["x"][dropped]) and not got["dW"][0].any() and got["db"][0] == 0
        if first is None:
            first = got
        else:
            # what does not go through the partial rows does not depend on the cap
            assert all(np.array_equal(got[k], first[k]) for k in ("y", "z", "stats", "dx"))


def test_default_cap_with_several_samples_per_workgroup(env):
    """N = 257 under the default cap of 256 workgroups: 129 of them walk two samples (the last one), so the dW a
    workgroup keeps in registers across its samples and the 129-row reduction are held on the path `adopt_blocks` takes."""
    n = R.DEFAULT_CAP + 1
    d, ref, own = R.inputs(n), R.reference(n), R.torch_deviations(n)
    assert env["L"].az_train_block_workspace_bytes(n, 0) == 129 * env["L"].az_train_block_workspace_bytes(1, 0)
    held(run_block(env, d, 0), ref, own, "N=%d default cap" % n)


# ---------------------------------------------------------------------------------------- 2. padding

@pytest.mark.parametrize("kx", (0, 2))
def test_taps_outside_the_board_contribute_nothing(env, kx):
    d = R.padding_inputs(kx)
    ref, own = R.padding_reference(kx)
    assert not d["x"][:, :, :, 1:6].any() and d["x"][:, :, :, 0].all() and not d["W"][:, :, :, 1].any() and not d["W"][:, :, :, 2 - kx].any()
    got = run_block(env, d, 0)
    held(got, ref, own, "padding kx=%d" % kx, ("y", "dx", "dW"))
    zero = ref["dW"] == 0
    assert zero[:, :, :, 0].all() and zero[:, :, :, 2].all() and not zero[:, :, :, 1].any()
    assert (got["dW"][zero] == 0).all(), "a tap outside the board, or one on a zero column, contributed to dW"


# ---------------------------------------------------------------------------------------- 3. null save pointers

def test_forward_without_save_pointers_gives_the_same_y(env):
    torch, L, abi = env["torch"], env["L"], env["abi"]
    d = R.inputs(7)
    slab = make_slab(env, d, 0)
    params, saved, _ = structs(env, slab)
    ys = []
    for how in (C.byref(saved), None, C.byref(abi.TrainBlockSavedC(None, None))):
        slab.upload()
        abi.check(L.az_train_dev_block_fwd(C.byref(params), slab.ptr("x"), slab.ptr("keep"), 7, R.EPS, slab.ptr("y"), how, abi._stream()))
        torch.cuda.synchronize()
        image = slab.dev.cpu().numpy()
        assert slab.untouched_outside(image, ("y", "z", "stats") if len(ys) == 0 else ("y",)), "an eval forward wrote more than y"
        ys.append(slab.get(image, "y", d["x"].shape))
    assert np.array_equal(ys[0].view(np.uint32), ys[1].view(np.uint32)) and np.array_equal(ys[0].view(np.uint32), ys[2].view(np.uint32))


# ---------------------------------------------------------------------------------------- 4. argument errors

def test_argument_errors_enqueue_and_write_nothing(env):
    torch, L, abi = env["torch"], env["L"], env["abi"]
    d = R.inputs(7)
    n = 7
    slab = make_slab(env, d, 0)

    params, saved, grads = structs(env, slab)

    def fwd(**kw):
        a = dict(params=params, x=slab.ptr("x"), keep=slab.ptr("keep"), n=n, eps=R.EPS, y=slab.ptr("y"), saved=saved)
        a.update(kw)
        return L.az_train_dev_block_fwd(None if a["params"] is None else C.byref(a["params"]), a["x"], a["keep"], a["n"], a["eps"], a["y"],
                                        None if a["saved"] is None else C.byref(a["saved"]), None)

    def bwd(**kw):
        a = dict(params=params, x=slab.ptr("x"), keep=slab.ptr("keep"), dy=slab.ptr("dy"), saved=saved, n=n, cap=0, grads=grads)
        a.update(kw)
        return L.az_train_dev_block_bwd(None if a["params"] is None else C.byref(a["params"]), a["x"], a["keep"], a["dy"],
                                        None if a["saved"] is None else C.byref(a["saved"]), a["n"], a["cap"],
                                        None if a["grads"] is None else C.byref(a["grads"]), None)

    bad = []
    # null required pointers
    bad += [fwd(params=None), fwd(x=None), fwd(y=None), bwd(params=None), bwd(x=None), bwd(dy=None), bwd(saved=None), bwd(grads=None)]
    bad += [fwd(params=swap(params, **{k: None})) for k in fields(params)] + [bwd(params=swap(params, **{k: None})) for k in fields(params)]
    bad += [fwd(saved=swap(saved, z=None)), fwd(saved=swap(saved, stats=None)), bwd(saved=swap(saved, z=None)), bwd(saved=swap(saved, stats=None))]
    bad += [bwd(grads=swap(grads, **{k: None})) for k in ("dx", "d_norm_weight", "d_norm_bias", "d_conv_weight", "d_conv_bias", "workspace")]
    # 16-byte alignment (x, y, dy, dx, keep, conv_weight, d_conv_weight, saved z, workspace); 4-byte for the rest
    bad += [fwd(x=slab.ptr("x", 4)), fwd(y=slab.ptr("y", 8)), fwd(keep=slab.ptr("keep", 4)), bwd(dy=slab.ptr("dy", 4)), bwd(x=slab.ptr("x", 12))]
    bad += [fwd(params=swap(params, conv_weight=slab.ptr("W", 4))), fwd(saved=swap(saved, z=slab.ptr("z", 4))),
            bwd(grads=swap(grads, dx=slab.ptr("dx", 4))), bwd(grads=swap(grads, d_conv_weight=slab.ptr("dW", 8))),
            bwd(grads=swap(grads, workspace=slab.ptr("ws", 4)))]
    bad += [fwd(params=swap(params, norm_weight=slab.ptr("gamma", 2))), fwd(saved=swap(saved, stats=slab.ptr("stats", 1))),
            bwd(grads=swap(grads, d_conv_bias=slab.ptr("db", 2))), bwd(grads=swap(grads, d_norm_weight=slab.ptr("dgamma", 3)))]
    # N, eps, the cap, the workspace
    bad += [fwd(n=0), fwd(n=-1), fwd(n=2 ** 30 + 1), bwd(n=0), bwd(n=2 ** 30 + 1)]
    bad += [fwd(eps=0.0), fwd(eps=-1e-5), fwd(eps=float("nan")), fwd(eps=float("inf"))]
    bad += [bwd(cap=-1), bwd(grads=swap(grads, workspace_bytes=slab.size["ws"] - 4)), bwd(grads=swap(grads, workspace_bytes=0))]
    assert bad == [AZ_ERR_ARG] * len(bad), bad
    assert L.az_train_block_workspace_bytes(0, 0) == -1 and L.az_train_block_workspace_bytes(7, -1) == -1
    assert L.az_train_block_workspace_bytes(2 ** 30 + 1, 0) == -1
    assert L.az_train_block_workspace_bytes(65, 3) == 3 * L.az_train_block_workspace_bytes(1, 0)
    assert L.az_train_block_workspace_bytes(7, 3) == 3 * L.az_train_block_workspace_bytes(1, 0)
    assert L.az_train_block_workspace_bytes(7, 0) == L.az_train_block_workspace_bytes(7, 100) == 7 * L.az_train_block_workspace_bytes(1, 0)
    # an aligned 4-byte pointer that is not 16-byte aligned is taken where the header says so
    torch.cuda.synchronize()
    assert np.array_equal(slab.dev.cpu().numpy(), slab.host), "a refused call wrote"
    assert fwd(params=swap(params, norm_bias=slab.ptr("beta", 4))) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------- 5. residual_block

def test_residual_block_kernel_route_against_the_torch_route(env, monkeypatch):
    torch, TB = env["torch"], env["TB"]
    n = 7
    d, ref, own = R.inputs(n), R.reference(n), R.torch_deviations(n)
    names = ("x", "gamma", "beta", "W", "b")
    results = {}
    for route in ("kernel", "torch"):
        t = [torch.from_numpy(d[k].copy()).cuda().requires_grad_(True) for k in names]
        keep = torch.from_numpy(d["keep"]).cuda()
        y = TB.residual_block(*t, keep=keep, eps=R.EPS, route=route)
        # the upstream gradient as a view that is not contiguous: the block's output goes through a transpose
        dy = torch.from_numpy(np.ascontiguousarray(d["dy"].transpose(0, 1, 3, 2))).cuda()
        assert not dy.transpose(2, 3).is_contiguous()
        (y.transpose(2, 3) * dy).sum().backward()
        assert all(p.grad is not None and p.grad.shape == p.shape for p in t)
        results[route] = dict(y=y.detach().cpu().numpy(), **{q: p.grad.cpu().numpy() for q, p in zip(("dx", "dgamma", "dbeta", "dW", "db"), t)})
    held(results["kernel"], ref, own, "residual_block kernel")
    gpu_torch = R.deviations(results["torch"], ref)
    for q in R.QUANTITIES:
        print("residual_block torch route on the GPU %-7s %.3e" % (q, gpu_torch[q]))
        # each within the bound of the other's reference: the two float32 routes differ by no more than both bounds
        assert R.dev(results["kernel"][q], results["torch"][q]) <= R.bound(own[q]) + max(gpu_torch[q], R.FLOOR)
    # the default route of CUDA tensors is the kernel's
    t = [torch.from_numpy(d[k].copy()).cuda() for k in names]
    keep = torch.from_numpy(d["keep"]).cuda()
    calls = []
    launch = TB._launch_fwd
    monkeypatch.setattr(TB, "_launch_fwd", lambda *a: calls.append(a[-1]) or launch(*a))
    with torch.no_grad():
        t[0].requires_grad_(True)
        y = TB.residual_block(*t, keep=keep, eps=R.EPS)
    assert calls == [False] and y.grad_fn is None and not y.requires_grad, "under no_grad nothing is saved"
    assert np.array_equal(y.cpu().numpy(), results["kernel"]["y"])
    y = TB.residual_block(*t, keep=keep, eps=R.EPS)
    assert calls == [False, True] and y.grad_fn is not None
    with pytest.raises(ValueError, match="contiguous"):
        TB.residual_block(torch.empty(n, 6, 7, 64, device="cuda").permute(0, 3, 1, 2), *t[1:])
    with pytest.raises(ValueError, match="one device"):
        TB.residual_block(t[0].detach(), t[1].cpu(), *t[2:])


# ---------------------------------------------------------------------------------------- 6. adopt_blocks under train_step

def test_adopted_blocks_under_train_step(env):
    """Three `train_step` batches of 64 rows of fixture G16's Connect4 batch: an adopted module against an unadopted twin
    of the same seed, both float32 on the GPU with the kernel loss route.  Float64 figures: the same net in double on
    the CPU with the torch loss route; the adopted module may deviate from them by 4 x what the twin does, or 1e-6."""
    torch, TL, TB = env["torch"], env["TL"], env["TB"]
    loader, d_loader = H.loaders(env)["cpu"], H.loaders(env)["cuda"]
    knobs = dict(TR.CONFIGS["b"])
    nets, values = {}, {}
    for name, dtype, device, data, route in (("adopted", torch.float32, "cuda", d_loader, "kernel"),
                                             ("twin", torch.float32, "cuda", d_loader, "kernel"),
                                             ("exact", torch.float64, "cpu", loader, "torch")):
        nets[name] = H.module(env, dtype, device, ("blocks",) if name == "adopted" else ())
        values[name] = TL.train_step(nets[name], data, lambda b: b, n_epochs=1, route=route, **knobs)
    figures = []
    for i, what in ((0, "policy loss"), (1, "value loss"), (2, "aux loss"), (4, "grad norm")):
        exact = values["exact"][i]
        dev, own = (abs(values[k][i] - exact) / abs(exact) for k in ("adopted", "twin"))
        print("train_step %-11s exact %.9g  adopted %.3e  twin %.3e  bound %.3e" % (what, exact, dev, own, R.bound(own)))
        figures.append((what, dev, own))
    for what, dev, own in figures:
        assert dev <= R.bound(own), (what, dev, own)
    assert all(p.grad is not None for p in nets["adopted"].parameters())
    # restored, the module is the class's own again: its eval outputs are the twin's forward on the same parameters
    assert TB.restore_blocks(nets["adopted"]) == 3
    nets["twin"].load_state_dict(nets["adopted"].state_dict())
    with torch.no_grad():
        a, b = (nets[k].eval()(d_loader[0][0]) for k in ("adopted", "twin"))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------- 7. dropout

def test_a_block_with_dropout_drops_whole_channels_in_training_only(env):
    torch, TB, NET = env["torch"], env["TB"], env["NET"]
    torch.manual_seed(9)
    net = NET.Connect4Net(device="cpu").cuda()
    block = [m for m in net.hidden.children() if isinstance(m, NET._Res)][0]
    block.dropout = torch.nn.Dropout2d(0.2)
    TB.adopt_blocks(net)
    x = torch.randn(65, 64, 6, 7, device="cuda")
    net.train()
    xg = x.clone().requires_grad_(True)
    y = block(xg)
    dropped = ((y.detach() - x).abs().amax(dim=(2, 3)) == 0).float().mean().item()
    y.sum().backward()
    assert torch.isfinite(xg.grad).all() and block.conv.weight.grad is not None
    net.eval()
    with torch.no_grad():
        none = ((block(x) - x).abs().amax(dim=(2, 3)) == 0).float().mean().item()
    print("dropped in training %.3f of 4160, in eval %.3f" % (dropped, none))
    assert 0.15 <= dropped <= 0.25 and none == 0.0
