"""The gated attention block's training forward and backward on the device (k_attn_fwd, k_attn_bwd, k_attn_reduce:
az_train_dev_attn_fwd / _bwd in include/az_train.h, `gated_attention` and `adopt_attention` in src/train_attn.py).

The kernels are held against the float64 restatement of tests/train_attn_ref.py on the same inputs.  Allowed deviation
per quantity - y, dx and the six parameter gradients: largest absolute difference over the quantity's largest magnitude -
is the larger of
    4 x the deviation of float32 torch (CPU) from the restatement on the same inputs, and
    1e-6;
the factor 4 covers a different but equally legitimate summation order.  float32 torch's own deviations on these inputs
are printed by tests/test_train_attn_cpu.py (1e-7 to 9e-7 on the plain cases, 2e-6 to 9e-6 on the large-logit case).

Through the C ABI y, dx, the six parameter gradients and the workspace each sit between guard regions of 256 bytes; the
guards and every input are compared exactly afterwards, and every call runs twice from the same start and must give the
same bytes.

1. N = 1, 2, 7, 65 with max_workgroups 0, 2 and 3, null bits and p = 0.2 bits with garbage above bit 41, one head's bits
   all zero in one sample, one all-zero sample;
2. N = 257 under the default cap (two samples per workgroup);
3. N = 7 token-major against NCHW;
4. large logits (the two head norms' weights times 6);
5. all-zero bits: y is x's tokens exactly, five gradients exactly zero;
6. the AZ_ERR_ARG cases;
7. `gated_attention` kernel route against the torch route, a non-contiguous upstream gradient, a channels-last x, no_grad;
8. `adopt_attention`, alone and with `adopt_blocks`, through three `train_step` batches against an unadopted twin;
9. `attn.dropout_p = 0.2` in training mode."""
import ctypes as C
import functools

import numpy as np
import pytest

import train_attn_ref as R
import train_gpu_harness as H
import train_loss_ref as TR
from train_gpu_harness import AZ_ERR_ARG, Slab, fields, loaders, swap

pytestmark = pytest.mark.gpu

INPUTS = ("x",) + R.PARAMS + ("bits", "dy")
GRADS = R.QUANTITIES[1:]
OUTPUTS = R.QUANTITIES + ("ws",)


@pytest.fixture(scope="module")
def env():
    return H.load_env(("az_net", "optim", "train_attn", "train_block", "train_loss"))


def structs(env, slab):
    abi = env["abi"]
    params = abi.TrainAttnParamsC(*(slab.ptr(k) for k in R.PARAMS))
    grads = abi.TrainAttnGradsC(*(slab.ptr(k) for k in GRADS), slab.ptr("ws"), slab.size["ws"])
    return params, grads


def make_slab(env, d, max_workgroups):
    n = d["x"].shape[0]
    ws = env["L"].az_train_attn_workspace_bytes(n, max_workgroups)
    assert ws > 0 and ws % 16 == 0
    out = dict(y=d["x"].nbytes, dx=d["x"].nbytes, **{"d_" + k: d[v].nbytes for k, v in
                                                     zip(("pre", "qkv", "gate", "o", "qn", "kn"), R.PARAMS)}, ws=ws)
    return Slab(env["torch"], {k: d[k] for k in INPUTS}, out)


def run_attn(env, d, max_workgroups, token_major=0):
    """Forward and backward through the C ABI, twice from the same start -> the eight quantities.  With `token_major` d["x"]
    is [N, 42, 64] and so is the dx returned."""
    torch, L, abi = env["torch"], env["L"], env["abi"]
    n = d["x"].shape[0]
    slab = make_slab(env, d, max_workgroups)
    params, grads = structs(env, slab)
    images = []
    for _ in range(2):
        slab.upload()
        torch.cuda.synchronize()
        abi.check(L.az_train_dev_attn_fwd(C.byref(params), slab.ptr("x"), token_major, slab.ptr("bits"), d["keep_scale"], n, R.EPS,
                                          slab.ptr("y"), abi._stream()))
        torch.cuda.synchronize()
        image = slab.dev.cpu().numpy()
        assert slab.untouched_outside(image, ("y",)), "the forward wrote outside y"
        abi.check(L.az_train_dev_attn_bwd(C.byref(params), slab.ptr("x"), token_major, slab.ptr("bits"), d["keep_scale"], slab.ptr("dy"),
                                          n, R.EPS, max_workgroups, C.byref(grads), abi._stream()))
        torch.cuda.synchronize()
        image = slab.dev.cpu().numpy()
        assert slab.untouched_outside(image, OUTPUTS), "a guard region or an input was written"
        images.append(image)
    assert np.array_equal(images[0], images[1]), "two calls on the same inputs differ"
    shapes = dict(y=(n, R.TOK, R.CH), dx=d["x"].shape, **{"d_" + k: d[v].shape for k, v in
                                                          zip(("pre", "qkv", "gate", "o", "qn", "kn"), R.PARAMS)})
    got = {k: slab.get(images[0], k, s) for k, s in shapes.items()}
    assert all(np.isfinite(v).all() for v in got.values())
    return got


held = functools.partial(H.held, R)


def tokens_of(x):
    return np.ascontiguousarray(x.reshape(x.shape[0], R.CH, R.TOK).transpose(0, 2, 1))


# ---------------------------------------------------------------------------------------- 1. sizes, caps, masks

@pytest.mark.parametrize("keep_p", (R.KEEP_P, 0.0))
@pytest.mark.parametrize("n", R.GPU_N)
def test_attention_through_the_c_abi(env, n, keep_p):
    d, ref, own = R.inputs(n, keep_p), R.reference(n, keep_p), R.torch_deviations(n, keep_p)
    assert (n == 1 or not d["x"][-1].any()) and (d["bits"] is None) == (keep_p == 0.0)
    if d["bits"] is not None:
        assert not (d["bits"][0, 1] & R.LOW).any() and (d["bits"] >> 42).any()
    first = None
    for cap in (0, 2, 3):
        got = run_attn(env, d, cap)
        held(got, ref, own, "N=%d keep_p=%.1f cap=%d" % (n, keep_p, cap))
        if first is None:
            first = got
        else:
            # what does not go through the partial rows does not depend on the cap
            assert all(np.array_equal(got[k], first[k]) for k in ("y", "dx"))


def test_default_cap_with_several_samples_per_workgroup(env):
    """N = 257 under the default cap of 256 workgroups: 129 of them walk two samples (the last one), so the accumulators a
    workgroup keeps in registers across its samples and the 129-row reduction are held on the path `adopt_attention` takes."""
    n = R.DEFAULT_CAP + 1
    d, ref, own = R.inputs(n, R.KEEP_P), R.reference(n, R.KEEP_P), R.torch_deviations(n, R.KEEP_P)
    assert env["L"].az_train_attn_workspace_bytes(n, 0) == 129 * env["L"].az_train_attn_workspace_bytes(1, 0)
    held(run_attn(env, d, 0), ref, own, "N=%d default cap" % n)


# ---------------------------------------------------------------------------------------- 3. token-major x

def test_token_major_input_agrees_with_nchw(env):
    n = 7
    d, ref, own = R.inputs(n, R.KEEP_P), R.reference(n, R.KEEP_P), R.torch_deviations(n, R.KEEP_P)
    got = run_attn(env, dict(d, x=tokens_of(d["x"])), 0, token_major=1)
    assert got["dx"].shape == (n, R.TOK, R.CH)
    got["dx"] = got["dx"].transpose(0, 2, 1).reshape(d["x"].shape)      # back to NCHW for the comparison
    held(got, ref, own, "N=7 token-major")
    nchw = run_attn(env, d, 0)
    for q in R.QUANTITIES:
        assert R.dev(got[q], nchw[q]) <= R.bound(own[q]), q


# ---------------------------------------------------------------------------------------- 4. large logits

def test_large_logits_stay_finite_and_inside_the_bound(env):
    case = (7, R.KEEP_P, 6.0)
    d, ref, own = R.inputs(*case), R.reference(*case), R.torch_deviations(*case)
    held(run_attn(env, d, 0), ref, own, "N=7 qk_scale=6")      # run_attn asserts that every output is finite


# ---------------------------------------------------------------------------------------- 5. all-zero bits

def test_all_zero_bits_leave_the_tokens_exactly(env):
    d = dict(R.inputs(7, R.KEEP_P))
    d["bits"] = (d["bits"] >> 42) << 42                           # garbage above bit 41 only
    assert d["bits"].any() and not (d["bits"] & R.LOW).any()
    got = run_attn(env, d, 0)
    assert np.array_equal(got["y"], tokens_of(d["x"]))
    for q in ("d_o", "d_qkv", "d_gate", "d_qn", "d_kn"):
        assert not got[q].any(), q
    assert got["dx"].any()


# ---------------------------------------------------------------------------------------- 6. argument errors

def test_argument_errors_enqueue_and_write_nothing(env):
    torch, L, abi = env["torch"], env["L"], env["abi"]
    d = R.inputs(7, R.KEEP_P)
    n = 7
    slab = make_slab(env, d, 0)

    params, grads = structs(env, slab)

    def fwd(**kw):
        a = dict(params=params, x=slab.ptr("x"), tm=0, bits=slab.ptr("bits"), scale=d["keep_scale"], n=n, eps=R.EPS, y=slab.ptr("y"))
        a.update(kw)
        return L.az_train_dev_attn_fwd(None if a["params"] is None else C.byref(a["params"]), a["x"], a["tm"], a["bits"], a["scale"],
                                       a["n"], a["eps"], a["y"], None)

    def bwd(**kw):
        a = dict(params=params, x=slab.ptr("x"), tm=0, bits=slab.ptr("bits"), scale=d["keep_scale"], dy=slab.ptr("dy"), n=n, eps=R.EPS,
                 cap=0, grads=grads)
        a.update(kw)
        return L.az_train_dev_attn_bwd(None if a["params"] is None else C.byref(a["params"]), a["x"], a["tm"], a["bits"], a["scale"],
                                       a["dy"], a["n"], a["eps"], a["cap"], None if a["grads"] is None else C.byref(a["grads"]), None)

    bad = []
    # null required pointers
    bad += [fwd(params=None), fwd(x=None), fwd(y=None), bwd(params=None), bwd(x=None), bwd(dy=None), bwd(grads=None)]
    bad += [fwd(params=swap(params, **{k: None})) for k in fields(params)] + [bwd(params=swap(params, **{k: None})) for k in fields(params)]
    bad += [bwd(grads=swap(grads, **{k: None})) for k in fields(grads) if k != "workspace_bytes"]
    # 16-byte alignment (x, y, dy, dx, qkv_weight, o_weight, their gradients, the workspace); 8-byte for the bits; 4-byte for the rest
    bad += [fwd(x=slab.ptr("x", 4)), fwd(y=slab.ptr("y", 8)), bwd(dy=slab.ptr("dy", 4)), bwd(x=slab.ptr("x", 12))]
    bad += [fwd(params=swap(params, qkv_weight=slab.ptr("Wqkv", 4))), fwd(params=swap(params, o_weight=slab.ptr("Wo", 8))),
            bwd(grads=swap(grads, dx=slab.ptr("dx", 4))), bwd(grads=swap(grads, d_qkv_weight=slab.ptr("d_qkv", 8))),
            bwd(grads=swap(grads, d_o_weight=slab.ptr("d_o", 4))), bwd(grads=swap(grads, workspace=slab.ptr("ws", 4)))]
    bad += [fwd(bits=slab.ptr("bits", 4)), bwd(bits=slab.ptr("bits", 4))]
    bad += [fwd(params=swap(params, prenorm_weight=slab.ptr("pre", 2))), fwd(params=swap(params, gate_weight=slab.ptr("Wg", 1))),
            fwd(params=swap(params, q_norm_weight=slab.ptr("qn", 2))), fwd(params=swap(params, k_norm_weight=slab.ptr("kn", 3))),
            bwd(grads=swap(grads, d_prenorm_weight=slab.ptr("d_pre", 2))), bwd(grads=swap(grads, d_gate_weight=slab.ptr("d_gate", 3))),
            bwd(grads=swap(grads, d_q_norm_weight=slab.ptr("d_qn", 1))), bwd(grads=swap(grads, d_k_norm_weight=slab.ptr("d_kn", 2)))]
    # N, eps, keep_scale, the layout flag, the cap, the workspace
    bad += [fwd(n=0), fwd(n=-1), fwd(n=2 ** 30 + 1), bwd(n=0), bwd(n=2 ** 30 + 1)]
    bad += [f(eps=e) for f in (fwd, bwd) for e in (0.0, -1e-5, float("nan"), float("inf"))]
    bad += [f(scale=s) for f in (fwd, bwd) for s in (0.5, float("nan"), float("inf"))]
    bad += [fwd(bits=None), bwd(bits=None)]                      # null bits with a scale that is not 1
    bad += [fwd(tm=2), fwd(tm=-1), bwd(tm=2)]
    bad += [bwd(cap=-1), bwd(grads=swap(grads, workspace_bytes=slab.size["ws"] - 4)), bwd(grads=swap(grads, workspace_bytes=0))]
    assert bad == [AZ_ERR_ARG] * len(bad), bad
    one = L.az_train_attn_workspace_bytes(1, 0)
    assert one == 16736 * 4
    assert L.az_train_attn_workspace_bytes(0, 0) == -1 and L.az_train_attn_workspace_bytes(7, -1) == -1
    assert L.az_train_attn_workspace_bytes(2 ** 30 + 1, 0) == -1
    assert L.az_train_attn_workspace_bytes(65, 3) == 3 * one and L.az_train_attn_workspace_bytes(7, 3) == 3 * one
    assert L.az_train_attn_workspace_bytes(7, 0) == L.az_train_attn_workspace_bytes(7, 100) == 7 * one
    assert L.az_train_attn_workspace_bytes(5000, 0) == 250 * one and L.az_train_attn_workspace_bytes(5000, 4000) == 1000 * one
    torch.cuda.synchronize()
    assert np.array_equal(slab.dev.cpu().numpy(), slab.host), "a refused call wrote"
    # an aligned 4-byte pointer that is not 16-byte aligned is taken where the header says so; null bits with scale 1
    assert fwd(params=swap(params, q_norm_weight=slab.ptr("qn", 4))) == 0
    assert fwd(bits=None, scale=1.0) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------- 7. gated_attention

def test_gated_attention_kernel_route_against_the_torch_route(env, monkeypatch):
    torch, TA = env["torch"], env["TA"]
    n = 7
    d, ref, own = R.inputs(n, R.KEEP_P), R.reference(n, R.KEEP_P), R.torch_deviations(n, R.KEEP_P)
    names = ("x",) + R.PARAMS
    bits = torch.from_numpy(d["bits"]).cuda()
    results = {}
    for route, channels_last in (("kernel", False), ("kernel", True), ("torch", False)):
        t = [torch.from_numpy(d[k].copy()).cuda().requires_grad_(True) for k in names]
        x = t[0]
        if channels_last:
            x = t[0].contiguous(memory_format=torch.channels_last)
            assert not x.is_contiguous() and TA._token_major(x) == 1
        y = TA.gated_attention(x, *t[1:], keep_bits=bits, keep_scale=d["keep_scale"], eps=R.EPS, route=route)
        assert y.shape == (n, 42, 64)
        # the upstream gradient as a view that is not contiguous: the block's output goes through a transpose
        dy = torch.from_numpy(np.ascontiguousarray(d["dy"].transpose(0, 2, 1))).cuda()
        assert not dy.transpose(1, 2).is_contiguous()
        (y.transpose(1, 2) * dy).sum().backward()
        assert all(p.grad is not None and p.grad.shape == p.shape for p in t)
        results[route, channels_last] = dict(y=y.detach().cpu().numpy(), **{q: p.grad.cpu().numpy() for q, p in zip(GRADS, t)})
    held(results["kernel", False], ref, own, "gated_attention kernel")
    held(results["kernel", True], ref, own, "gated_attention kernel, channels-last")
    gpu_torch = R.deviations(results["torch", False], ref)
    for q in R.QUANTITIES:
        print("gated_attention torch route on the GPU %-7s %.3e" % (q, gpu_torch[q]))
        # each within the bound of the other's reference: the two float32 routes differ by no more than both bounds
        assert R.dev(results["kernel", False][q], results["torch", False][q]) <= R.bound(own[q]) + max(gpu_torch[q], R.FLOOR)
    # the default route of CUDA tensors is the kernel's; under no_grad nothing is saved
    t = [torch.from_numpy(d[k].copy()).cuda() for k in names]
    applied = []
    apply = TA._Attention.apply
    monkeypatch.setattr(TA._Attention, "apply", staticmethod(lambda *a: applied.append(1) or apply(*a)))
    with torch.no_grad():
        t[0].requires_grad_(True)
        y = TA.gated_attention(*t, keep_bits=bits, keep_scale=d["keep_scale"], eps=R.EPS)
    assert applied == [] and y.grad_fn is None and not y.requires_grad, "under no_grad nothing is saved"
    assert np.array_equal(y.cpu().numpy(), results["kernel", False]["y"])
    y = TA.gated_attention(*t, keep_bits=bits, keep_scale=d["keep_scale"], eps=R.EPS)
    assert applied == [1] and y.grad_fn is not None
    # any other stride pattern is copied once and gives the same bytes
    odd = torch.empty(n, 64, 7, 6, device="cuda").transpose(2, 3)
    odd.copy_(t[0].detach())
    assert TA._token_major(odd) is None
    with torch.no_grad():
        assert torch.equal(TA.gated_attention(odd, *t[1:], keep_bits=bits, keep_scale=d["keep_scale"], eps=R.EPS), y.detach())
    with pytest.raises(ValueError, match="one device"):
        TA.gated_attention(t[0].detach(), t[1].cpu(), *t[2:])
    with pytest.raises(ValueError, match="keep_bits"):
        TA.gated_attention(*t, keep_bits=bits.cpu(), keep_scale=d["keep_scale"])


# ---------------------------------------------------------------------------------------- 8. adopt_attention under train_step

def module(env, dtype, device, attention, blocks):
    return H.module(env, dtype, device, ("blocks",) * blocks + ("attention",) * attention)


@pytest.fixture(scope="module")
def baselines(env):
    """The unadopted float32 twin on the GPU and the float64 net on the CPU, run once for both cases."""
    return H.baselines(env)


@pytest.mark.parametrize("blocks", (False, True))
def test_adopted_attention_under_train_step(env, baselines, blocks):
    """Three `train_step` batches of 64 rows of fixture G16's Connect4 batch: a module with its attention block adopted
    (and, in the second case, its residual blocks too) against an unadopted twin of the same seed, both float32 on the GPU
    with the kernel loss route.  Float64 figures: the same net in double on the CPU with the torch loss route; the adopted
    module may deviate from them by 4 x what the twin does, or 1e-6."""
    torch, TL, TA = env["torch"], env["TL"], env["TA"]
    twin_values, exact_values = baselines["twin"], baselines["exact"]
    net = module(env, torch.float32, "cuda", True, blocks)
    values = TL.train_step(net, loaders(env)["cuda"], lambda b: b, n_epochs=1, route="kernel", **dict(TR.CONFIGS["b"]))
    figures = []
    for i, what in ((0, "policy loss"), (1, "value loss"), (2, "aux loss"), (4, "grad norm")):
        exact = exact_values[i]
        dev, own = (abs(v[i] - exact) / abs(exact) for v in (values, twin_values))
        print("train_step blocks=%d %-11s exact %.9g  adopted %.3e  twin %.3e  bound %.3e" % (blocks, what, exact, dev, own, R.bound(own)))
        figures.append((what, dev, own))
    for what, dev, own in figures:
        assert dev <= R.bound(own), (what, dev, own)
    assert all(p.grad is not None for p in net.parameters())
    # restored, the module is the class's own again: its eval outputs are a fresh twin's forward on the same parameters
    assert TA.restore_attention(net) == 1
    if blocks:
        assert env["TB"].restore_blocks(net) == 3
    other = module(env, torch.float32, "cuda", False, False)
    other.load_state_dict(net.state_dict())
    with torch.no_grad():
        a, b = (m.eval()(loaders(env)["cuda"][0][0]) for m in (net, other))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------- 9. dropout

def test_attention_dropout_in_training_mode_only(env):
    torch, TA, NET = env["torch"], env["TA"], env["NET"]
    torch.manual_seed(9)
    net = NET.Connect4Net(device="cpu").cuda()
    block = net.hidden[-1]
    block.attn.dropout_p = 0.2
    TA.adopt_attention(net)
    x = torch.randn(65, 64, 6, 7, device="cuda")
    net.eval()
    with torch.no_grad():
        plain = block(x)
    net.train()
    outs = []
    for _ in range(2):
        torch.manual_seed(3)
        xg = x.clone().requires_grad_(True)
        y = block(xg)
        y.sum().backward()
        assert torch.isfinite(y).all() and torch.isfinite(xg.grad).all() and block.attn.qkv_proj.weight.grad is not None
        outs.append((y.detach().clone(), xg.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "the same seed draws the same mask"
    assert not torch.equal(outs[0][0], plain)
    net.eval()
    with torch.no_grad():
        assert torch.equal(block(x), plain)
