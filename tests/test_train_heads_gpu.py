"""The Connect4 heads' training forward and backward on the device (k_heads_fwd, k_heads_bwd, k_heads_reduce:
az_train_dev_heads_fwd / _bwd in include/az_train.h, `heads`, `adopt_heads` and `adopt_all` in src/train_heads.py).

The kernels are held against the float64 restatement of tests/train_heads_ref.py on the same inputs.  Allowed deviation
per quantity - the three outputs, d_tokens and the eighteen parameter gradients: largest absolute difference over the
quantity's largest magnitude - is the larger of
    4 x the deviation of float32 torch (CPU) from the restatement on the same inputs, and
    1e-6;
the factor 4 covers a different but equally legitimate summation order.  Two refinements (tests/train_heads_ref.py):
log_p is measured on the legal entries alone, over the largest legal magnitude, and an illegal entry (about -1e9, where
one float32 ulp is 64) is held to 64 absolutely; d_row_gate_bias and d_policy_out_bias, sums that cancel, are measured
over the float64 sum of their terms' absolute values.  float32 torch's own deviations on these inputs are printed by
tests/test_train_heads_cpu.py (2e-8 to 8e-7 on the plain cases, up to 3.7e-6 on the saturated one).
Measured on an MI355X: no case needed more than 0.58 of its bound (d_policy_fc_weight in the saturated case).

Through the C ABI the three outputs, d_tokens, the eighteen gradients and the workspace each sit between guard regions of
256 bytes; the guards and every input are compared exactly afterwards, and every call runs twice from the same start and
must give the same bytes.

1. N = 1, 2, 7, 65 with max_workgroups 0, 2 and 3: null legal and keeps, and the standard mask with p = 0.2 keeps (one
   policy column's keep all zero in sample 0, sample N // 2's keep_pool all zero, an all-zero sample when N >= 2);
2. N = 257 under the default cap (two samples per workgroup);
3. saturation: row_gate.weight x 20 and out.weight x 50 - without the maxima taken out exp overflows;
4. exact cases: one entirely illegal sample; d_log_p = 0; d_value = 0 and d_steps = 0;
5. the AZ_ERR_ARG cases;
6. `heads` kernel route against the torch route, non-contiguous upstream gradients, one output unused, no_grad;
7. `adopt_heads` alone and `adopt_all` through three `train_step` batches against an unadopted twin and the float64 net;
8. dropout 0.2 in training mode."""
import ctypes as C

import numpy as np
import pytest

import train_gpu_harness as H
import train_heads_ref as R
import train_loss_ref as TR
from train_gpu_harness import AZ_ERR_ARG, Slab, fields, loaders, swap

pytestmark = pytest.mark.gpu

ROW_BYTES = R.ROW_FLOATS * 4
INPUTS = ("tokens",) + R.FIELDS + ("legal", "keep_policy", "keep_pool") + R.UPSTREAM
WRITTEN = R.QUANTITIES + ("ws",)


@pytest.fixture(scope="module")
def env():
    return H.load_env(("az_net", "optim", "train_attn", "train_block", "train_heads", "train_loss", "train_stem"))


def shapes(n):
    return dict(log_p=(n, R.COLS), value=(n, R.CLASSES), steps=(n,), d_tokens=(n, R.TOK, R.CH),
                **{"d_" + k: s for k, s in zip(R.FIELDS, R.SHAPES)})


def make_slab(env, d, max_workgroups):
    n = d["tokens"].shape[0]
    ws = env["L"].az_train_heads_workspace_bytes(n, max_workgroups)
    assert ws > 0 and ws % 16 == 0
    out = {k: int(np.prod(s)) * 4 for k, s in shapes(n).items()}
    out["ws"] = ws
    return Slab(env["torch"], {k: d[k] for k in INPUTS}, out)


def structs(env, slab):
    abi = env["abi"]
    params = abi.TrainHeadsParamsC(*(slab.ptr(k) for k in R.FIELDS))
    grads = abi.TrainHeadsGradsC(slab.ptr("d_tokens"), *(slab.ptr(k) for k in R.GRADS), slab.ptr("ws"), slab.size["ws"])
    return params, grads


def run_heads(env, d, max_workgroups):
    """Forward and backward through the C ABI, twice from the same start -> the QUANTITIES."""
    torch, L, abi = env["torch"], env["L"], env["abi"]
    n = d["tokens"].shape[0]
    slab = make_slab(env, d, max_workgroups)
    params, grads = structs(env, slab)
    images = []
    for _ in range(2):
        slab.upload()
        torch.cuda.synchronize()
        abi.check(L.az_train_dev_heads_fwd(C.byref(params), slab.ptr("tokens"), slab.ptr("legal"), slab.ptr("keep_policy"),
                                           slab.ptr("keep_pool"), n, R.EPS, slab.ptr("log_p"), slab.ptr("value"), slab.ptr("steps"),
                                           abi._stream()))
        torch.cuda.synchronize()
        image = slab.dev.cpu().numpy()
        assert slab.untouched_outside(image, R.OUTPUTS), "the forward wrote outside its three outputs"
        abi.check(L.az_train_dev_heads_bwd(C.byref(params), slab.ptr("tokens"), slab.ptr("legal"), slab.ptr("keep_policy"),
                                           slab.ptr("keep_pool"), slab.ptr("d_log_p"), slab.ptr("d_value"), slab.ptr("d_steps"), n, R.EPS,
                                           max_workgroups, C.byref(grads), abi._stream()))
        torch.cuda.synchronize()
        image = slab.dev.cpu().numpy()
        assert slab.untouched_outside(image, WRITTEN), "a guard region or an input was written"
        images.append(image)
    assert np.array_equal(images[0], images[1]), "two calls on the same inputs differ"
    got = {k: slab.get(images[0], k, s) for k, s in shapes(n).items()}
    assert all(np.isfinite(v).all() for v in got.values())
    return got


def held(got, ref, own, what, quantities=R.QUANTITIES):
    devs = H.held(R, got, ref, own, what, quantities)
    if "log_p" in quantities:
        print("%s %-22s kernel %.3e  torch %.3e  bound %.3e" % (what, "log_p_illegal", devs["log_p_illegal"], own["log_p_illegal"], R.ILLEGAL_ABS))
    assert devs.get("log_p_illegal", 0.0) <= R.ILLEGAL_ABS, (what, devs["log_p_illegal"])
    return devs


# ---------------------------------------------------------------------------------------- 1. sizes, caps, masks, keeps

@pytest.mark.parametrize("case", (R.KEPT, R.PLAIN))
@pytest.mark.parametrize("n", R.GPU_N)
def test_heads_through_the_c_abi(env, n, case):
    """Also what fails when the mean token is not divided by 42 (value, steps and every dual-head gradient) or when
    d_logit is not zeroed on illegal entries (the policy gradients of the masked case: d_log_p is non-zero there)."""
    d, ref, own = R.inputs(n, case), R.reference(n, case), R.torch_deviations(n, case)
    assert n == 1 or not d["tokens"][-1].any()
    if case == R.KEPT:
        assert d["legal"][0].all() and not d["keep_policy"][0, 2].any() and not d["keep_pool"][n // 2].any()
        assert n < 3 or (not d["legal"][1].any() and d["d_log_p"][1].all())
    else:
        assert d["legal"] is None and d["keep_policy"] is None and d["keep_pool"] is None
    first = None
    for cap in (0, 2, 3):
        got = run_heads(env, d, cap)
        held(got, ref, own, "N=%d case=%d cap=%d" % (n, case, cap))
        if first is None:
            first = got
        else:
            # what does not go through the partial rows does not depend on the cap
            assert all(np.array_equal(got[k], first[k]) for k in R.OUTPUTS + ("d_tokens",))


def test_default_cap_with_several_samples_per_workgroup(env):
    """N = 257 under the default cap of 256 workgroups: 129 of them walk two samples (the last one one), so the sums a
    workgroup keeps in registers across its samples and the 129-row reduction are held on the path `adopt_heads` takes."""
    n = R.DEFAULT_CAP + 1
    d, ref, own = R.inputs(n, R.KEPT), R.reference(n, R.KEPT), R.torch_deviations(n, R.KEPT)
    assert env["L"].az_train_heads_workspace_bytes(n, 0) == 129 * ROW_BYTES
    held(run_heads(env, d, 0), ref, own, "N=%d default cap" % n)


# ---------------------------------------------------------------------------------------- 3. saturation

def test_saturated_softmaxes_take_their_maxima_out(env):
    """row_gate.weight x 20 and out.weight x 50: row scores and logits reach the hundreds, where exp of the score itself
    overflows float32; with the column's and the row's maximum taken out every output is finite and inside the bound."""
    case = (7, R.SATURATED)
    d, ref, own = R.inputs(*case), R.reference(*case), R.torch_deviations(*case)
    legal = d["legal"]
    assert np.abs(ref["log_p"][legal]).max() > 89.0 and ref["row_score_max"] > 89.0, "scores and logits beyond what exp takes in float32"
    held(run_heads(env, d, 0), ref, own, "N=7 saturated")       # run_heads asserts that every output is finite


# ---------------------------------------------------------------------------------------- 4. exact cases

def test_an_entirely_illegal_sample(env):
    d = dict(R.inputs(1, R.PLAIN))
    d["legal"] = np.zeros((1, R.COLS), bool)
    for cap in (0, 1):
        got = run_heads(env, d, cap)
        want = np.float32(-np.log(7.0))
        assert np.all(got["log_p"] == got["log_p"][0, 0]), got["log_p"]
        assert abs(got["log_p"][0, 0] - want) <= np.spacing(np.abs(want)), (got["log_p"][0, 0], want)
        for k in R.POLICY:
            assert not got["d_" + k].any(), k
        assert all(got["d_" + k].any() for k in R.DUAL) and got["d_tokens"].any()


def test_no_policy_gradient_leaves_the_policy_head_exactly_alone(env):
    d = dict(R.inputs(7, R.KEPT))
    d["d_log_p"] = np.zeros_like(d["d_log_p"])
    got = run_heads(env, d, 0)
    for k in R.POLICY:
        assert not got["d_" + k].any(), k
    # only the mean token carries a gradient: every token of a sample gets the same row, byte for byte
    rows = got["d_tokens"].view(np.uint32)
    assert np.array_equal(rows, np.broadcast_to(rows[:, :1], rows.shape)) and got["d_tokens"].any()
    ref = R.restatement(d)
    own = R.deviations(R.torch_route(d), ref, ("d_tokens",) + tuple("d_" + k for k in R.DUAL))
    held(got, ref, own, "d_log_p=0", ("d_tokens",) + tuple("d_" + k for k in R.DUAL))


def test_no_value_gradient_leaves_the_dual_head_exactly_alone(env):
    d = dict(R.inputs(7, R.KEPT))
    d["d_value"], d["d_steps"] = np.zeros_like(d["d_value"]), np.zeros_like(d["d_steps"])
    got = run_heads(env, d, 0)
    for k in R.DUAL:
        assert not got["d_" + k].any(), k
    assert all(got["d_" + k].any() for k in R.POLICY)
    ref = R.restatement(d)
    own = R.deviations(R.torch_route(d), ref, ("d_tokens",) + tuple("d_" + k for k in R.POLICY))
    held(got, ref, own, "d_value=0", ("d_tokens",) + tuple("d_" + k for k in R.POLICY))


# ---------------------------------------------------------------------------------------- 5. argument errors

def test_argument_errors_enqueue_and_write_nothing(env):
    torch, L = env["torch"], env["L"]
    d = R.inputs(7, R.KEPT)
    n = 7
    slab = make_slab(env, d, 0)

    params, grads = structs(env, slab)

    def fwd(**kw):
        a = dict(params=params, tokens=slab.ptr("tokens"), legal=slab.ptr("legal"), kp=slab.ptr("keep_policy"), kq=slab.ptr("keep_pool"),
                 n=n, eps=R.EPS, log_p=slab.ptr("log_p"), value=slab.ptr("value"), steps=slab.ptr("steps"))
        a.update(kw)
        return L.az_train_dev_heads_fwd(None if a["params"] is None else C.byref(a["params"]), a["tokens"], a["legal"], a["kp"], a["kq"],
                                        a["n"], a["eps"], a["log_p"], a["value"], a["steps"], None)

    def bwd(**kw):
        a = dict(params=params, tokens=slab.ptr("tokens"), legal=slab.ptr("legal"), kp=slab.ptr("keep_policy"), kq=slab.ptr("keep_pool"),
                 d_log_p=slab.ptr("d_log_p"), d_value=slab.ptr("d_value"), d_steps=slab.ptr("d_steps"), n=n, eps=R.EPS, cap=0, grads=grads)
        a.update(kw)
        return L.az_train_dev_heads_bwd(None if a["params"] is None else C.byref(a["params"]), a["tokens"], a["legal"], a["kp"], a["kq"],
                                        a["d_log_p"], a["d_value"], a["d_steps"], a["n"], a["eps"], a["cap"],
                                        None if a["grads"] is None else C.byref(a["grads"]), None)

    square = ("policy_fc_weight", "pool_fc_weight", "fc_weight")
    bad = []
    # null required pointers
    bad += [fwd(params=None), fwd(tokens=None), fwd(log_p=None), fwd(value=None), fwd(steps=None)]
    bad += [bwd(params=None), bwd(tokens=None), bwd(d_log_p=None), bwd(d_value=None), bwd(d_steps=None), bwd(grads=None)]
    bad += [f(params=swap(params, **{k: None})) for f in (fwd, bwd) for k in fields(params)]
    bad += [bwd(grads=swap(grads, **{k: None})) for k in fields(grads) if k != "workspace_bytes"]
    # 16-byte alignment: tokens, d_tokens, the three 64 x 64 weights and their gradients, the keeps, the workspace
    bad += [fwd(tokens=slab.ptr("tokens", 4)), bwd(tokens=slab.ptr("tokens", 8)), fwd(kp=slab.ptr("keep_policy", 4)),
            fwd(kq=slab.ptr("keep_pool", 8)), bwd(kp=slab.ptr("keep_policy", 12)), bwd(kq=slab.ptr("keep_pool", 4)),
            bwd(grads=swap(grads, d_tokens=slab.ptr("d_tokens", 4))), bwd(grads=swap(grads, workspace=slab.ptr("ws", 8)))]
    bad += [f(params=swap(params, **{k: slab.ptr(k, 4)})) for f in (fwd, bwd) for k in square]
    bad += [bwd(grads=swap(grads, **{"d_" + k: slab.ptr("d_" + k, 8)})) for k in square]
    # 4-byte alignment for everything else
    bad += [fwd(params=swap(params, **{k: slab.ptr(k, 2)})) for k in R.FIELDS if k not in square]
    bad += [bwd(grads=swap(grads, **{"d_" + k: slab.ptr("d_" + k, 1)})) for k in R.FIELDS if k not in square]
    bad += [fwd(log_p=slab.ptr("log_p", 2)), fwd(value=slab.ptr("value", 1)), fwd(steps=slab.ptr("steps", 3)),
            bwd(d_log_p=slab.ptr("d_log_p", 2)), bwd(d_value=slab.ptr("d_value", 3)), bwd(d_steps=slab.ptr("d_steps", 1))]
    # N, eps, the cap, the workspace
    bad += [fwd(n=0), fwd(n=-1), fwd(n=2 ** 30 + 1), bwd(n=0), bwd(n=-3), bwd(n=2 ** 30 + 1)]
    bad += [f(eps=e) for f in (fwd, bwd) for e in (0.0, -1e-5, float("nan"), float("inf"))]
    bad += [bwd(cap=-1), bwd(grads=swap(grads, workspace_bytes=slab.size["ws"] - 4)), bwd(grads=swap(grads, workspace_bytes=0))]
    assert bad == [AZ_ERR_ARG] * len(bad), bad
    size = L.az_train_heads_workspace_bytes
    assert size(1, 0) == ROW_BYTES == 13128 * 4
    assert size(0, 0) == -1 and size(7, -1) == -1 and size(2 ** 30 + 1, 0) == -1
    assert size(65, 3) == size(7, 3) == 3 * ROW_BYTES
    assert size(7, 0) == size(7, 100) == 7 * ROW_BYTES
    assert size(5000, 0) == 250 * ROW_BYTES and size(5000, 4000) == 1000 * ROW_BYTES
    torch.cuda.synchronize()
    assert np.array_equal(slab.dev.cpu().numpy(), slab.host), "a refused call wrote"
    # what the header allows is taken: a 4-byte aligned small parameter, a legal of any alignment, null legal and keeps
    assert fwd(params=swap(params, policy_norm_weight=slab.ptr("policy_norm_weight", 4)), legal=slab.ptr("legal", 1), n=6) == 0
    assert fwd(legal=None, kp=None, kq=None) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------- 6. heads

def test_heads_kernel_route_against_the_torch_route(env, monkeypatch):
    torch, TH = env["torch"], env["TH"]
    n = 7
    d, ref, own = R.inputs(n, R.KEPT), R.reference(n, R.KEPT), R.torch_deviations(n, R.KEPT)
    legal = torch.from_numpy(d["legal"]).cuda()
    keeps = dict(keep_policy=torch.from_numpy(d["keep_policy"]).cuda(), keep_pool=torch.from_numpy(d["keep_pool"]).cuda())
    names = ("tokens",) + R.FIELDS
    results = {}
    for route in ("kernel", "torch"):
        t = [torch.from_numpy(d[k].copy()).cuda().requires_grad_(True) for k in names]
        out = TH.heads(t[0], legal, *t[1:], eps=R.EPS, route=route, **keeps)
        assert [tuple(o.shape) for o in out] == [(n, 7), (n, 3), (n,)]
        # the upstream gradients as views that are not contiguous
        ups = [torch.from_numpy(np.ascontiguousarray(d["d_log_p"].T)).cuda().t(), torch.from_numpy(np.ascontiguousarray(d["d_value"].T)).cuda().t(),
               torch.from_numpy(np.repeat(d["d_steps"], 2)).cuda()[::2]]
        assert not any(u.is_contiguous() for u in ups)
        torch.autograd.backward(list(out), ups)
        assert all(p.grad is not None and p.grad.shape == p.shape for p in t)
        results[route] = dict(zip(R.OUTPUTS, (o.detach().cpu().numpy() for o in out)), d_tokens=t[0].grad.cpu().numpy(),
                              **{"d_" + k: p.grad.cpu().numpy() for k, p in zip(R.FIELDS, t[1:])})
    held(results["kernel"], ref, own, "heads kernel")
    gpu_torch = R.deviations(results["torch"], ref)
    between = R.deviations(results["kernel"], dict(results["torch"], legal=ref["legal"], abs_ds=ref["abs_ds"], abs_dlogit=ref["abs_dlogit"]))
    for q in R.QUANTITIES:
        print("heads torch route on the GPU %-22s %.3e" % (q, gpu_torch[q]))
        # each within the bound of the other's reference: the two float32 routes differ by no more than both bounds
        assert between[q] <= R.bound(own[q]) + max(gpu_torch[q], R.FLOOR), q
    # one output unused: its gradient counts as zero
    t = [torch.from_numpy(d[k].copy()).cuda().requires_grad_(True) for k in names]
    out = TH.heads(t[0], legal, *t[1:], eps=R.EPS, **keeps)
    (out[1] * torch.from_numpy(d["d_value"]).cuda()).sum().backward()
    only = dict(d, d_log_p=np.zeros_like(d["d_log_p"]), d_steps=np.zeros_like(d["d_steps"]))
    only_ref = R.restatement(only)
    quantities = ("d_tokens",) + tuple("d_" + k for k in R.DUAL if k not in ("aux_out_weight", "aux_out_bias"))
    got = dict(d_tokens=t[0].grad.cpu().numpy(), **{"d_" + k: p.grad.cpu().numpy() for k, p in zip(R.FIELDS, t[1:])})
    held(got, only_ref, R.deviations(R.torch_route(only), only_ref, quantities), "value alone", quantities)
    assert not any(got["d_" + k].any() for k in R.POLICY + ("aux_out_weight", "aux_out_bias"))
    # the default route of CUDA tensors is the kernel's; under no_grad, or when nothing needs a gradient, nothing is saved
    t = [torch.from_numpy(d[k].copy()).cuda() for k in names]
    applied = []
    apply = TH._Heads.apply
    monkeypatch.setattr(TH._Heads, "apply", staticmethod(lambda *a: applied.append(1) or apply(*a)))
    out = TH.heads(t[0], legal, *t[1:], eps=R.EPS, **keeps)
    assert applied == [] and all(o.grad_fn is None for o in out)
    assert all(np.array_equal(o.cpu().numpy(), results["kernel"][k]) for o, k in zip(out, R.OUTPUTS))
    t[4].requires_grad_(True)
    with torch.no_grad():
        out = TH.heads(t[0], legal, *t[1:], eps=R.EPS, **keeps)
    assert applied == [] and all(o.grad_fn is None and not o.requires_grad for o in out), "under no_grad nothing is saved"
    out = TH.heads(t[0], legal, *t[1:], eps=R.EPS, max_workgroups=3, **keeps)
    assert applied == [1] and all(o.grad_fn is not None for o in out)
    torch.autograd.backward(list(out), [torch.from_numpy(d[k]).cuda() for k in R.UPSTREAM])
    assert R.dev(t[4].grad.cpu().numpy(), ref["d_policy_fc_weight"]) <= R.bound(own["d_policy_fc_weight"])
    # tokens that are not contiguous are copied once and give the same bytes
    odd = torch.empty(n, 64, 42, device="cuda").transpose(1, 2)
    odd.copy_(t[0])
    assert not odd.is_contiguous()
    with torch.no_grad():
        again = TH.heads(odd, legal, *t[1:], eps=R.EPS, **keeps)
    assert all(np.array_equal(o.cpu().numpy(), results["kernel"][k]) for o, k in zip(again, R.OUTPUTS))
    with pytest.raises(ValueError, match="one device"):
        TH.heads(t[0], legal, t[1].cpu(), *t[2:])
    with pytest.raises(ValueError, match="legal"):
        TH.heads(t[0], legal.cpu(), *t[1:])
    with pytest.raises(ValueError, match="float32"):
        TH.heads(t[0].half(), legal, *t[1:])


# ---------------------------------------------------------------------------------------- 7. adoption under train_step

def module(env, dtype, device):
    return H.module(env, dtype, device, stem_bias=True)


def adopted(env, which):
    net = module(env, env["torch"].float32, "cuda")
    if which == "heads":
        assert env["TH"].adopt_heads(net) == 1
    else:
        assert env["TH"].adopt_all(net) == (3, 1, 1, 1)
    return net


@pytest.fixture(scope="module")
def baselines(env):
    """The unadopted float32 twin on the GPU and the float64 net on the CPU, run once for both cases."""
    return H.baselines(env, stem_bias=True)


@pytest.mark.parametrize("which", ("heads", "all"))
def test_adopted_heads_under_train_step(env, baselines, which, monkeypatch):
    """Three `train_step` batches of 64 rows of fixture G16's Connect4 batch: a module with its heads adopted (and, in the
    second case, stem, residual blocks and attention block too: the whole batch in the project's kernels) against an
    unadopted twin of the same seed, both float32 on the GPU with the kernel loss route.  Float64 figures: the same net in
    double on the CPU with the torch loss route; the adopted module may deviate from them by 4 x what the twin does, or
    1e-6.  Losses and the gradient norm, not parameters: d row_gate.bias is rounding on either route, and AdamW's
    normalised step turns it into parameters that cannot be compared."""
    torch, TL, TH = env["torch"], env["TL"], env["TH"]
    twin_values, exact_values = baselines["twin"], baselines["exact"]
    net = adopted(env, which)
    seen = []
    heads = TH.heads

    def watched(*a, **kw):
        out = heads(*a, **kw)
        seen.append(out[0].grad_fn is not None)
        return out
    monkeypatch.setattr(TH, "heads", watched)
    values = TL.train_step(net, loaders(env)["cuda"], lambda b: b, n_epochs=1, route="kernel", **dict(TR.CONFIGS["b"]))
    assert seen == [True, True, True, False], "three training batches, then one forward under no_grad, one `heads` call each"
    figures = []
    for i, what in ((0, "policy loss"), (1, "value loss"), (2, "aux loss"), (4, "grad norm")):
        exact = exact_values[i]
        dev, own = (abs(v[i] - exact) / abs(exact) for v in (values, twin_values))
        print("train_step %-5s %-11s exact %.9g  adopted %.3e  twin %.3e  bound %.3e" % (which, what, exact, dev, own, R.bound(own)))
        figures.append((what, dev, own))
    for what, dev, own in figures:
        assert dev <= R.bound(own), (what, dev, own)
    assert all(p.grad is not None for p in net.parameters())
    # restored, the module is the class's own again: its eval outputs are a fresh twin's forward on the same parameters
    if which == "heads":
        assert TH.restore_heads(net) == 1
    else:
        assert TH.restore_all(net) == (3, 1, 1, 1)
    other = module(env, torch.float32, "cuda")
    other.load_state_dict(net.state_dict())
    state, mask = loaders(env)["cuda"][0][0], loaders(env)["cuda"][0][6]
    with torch.no_grad():
        a, b = (m.eval()(state, mask) for m in (net, other))
    assert all(torch.equal(x, y) for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------- 8. dropout

def test_heads_dropout_in_training_mode_only(env):
    torch, TH, NET = env["torch"], env["TH"], env["NET"]
    torch.manual_seed(9)
    net = NET.Connect4Net(device="cpu")
    with torch.no_grad():
        for lin in (net.policy_head.out, net.dual_head.value_out, net.dual_head.aux_out):
            lin.weight.normal_(0, 0.05)
    net = net.cuda()
    net.policy_head.dropout = torch.nn.Dropout(0.2)
    net.dual_head.pool_drop = torch.nn.Dropout(0.2)
    TH.adopt_heads(net)
    state, mask = loaders(env)["cuda"][0][0], loaders(env)["cuda"][0][6]
    net.eval()
    with torch.no_grad():
        plain = net(state, mask)
        assert all(torch.equal(a, b) for a, b in zip(net(state, mask), plain)), "eval forwards are equal"
    net.train()
    outs = []
    for seed in (3, 3, 4):
        torch.manual_seed(seed)
        net.zero_grad(set_to_none=True)
        out = net(state, mask)
        (out[0].clamp_min(-100).sum() + out[1].sum() + out[2].sum()).backward()
        assert all(torch.isfinite(o).all() for o in out) and all(torch.isfinite(p.grad).all() for p in net.parameters())
        outs.append([o.detach().clone() for o in out])
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1])), "the same seed draws the same factors"
    assert not torch.equal(outs[0][0], outs[2][0]) and not torch.equal(outs[0][1], outs[2][1]), "two training forwards differ"
    assert not torch.equal(outs[0][0], plain[0]) and not torch.equal(outs[0][1], plain[1])
    net.eval()
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(net(state, mask), plain))
    # the same factors handed to `heads` on both routes: the kernel route within the bound of the float64 restatement on these
    # inputs, the two float32 routes within both bounds of each other
    torch.manual_seed(5)
    kp, kq = TH.draw_keep((7, 7, 64), 0.2, "cuda"), TH.draw_keep((7, 64), 0.2, "cuda")
    assert set(np.unique(kp.cpu().numpy())) == {np.float32(0.0), np.float32(1.25)}
    d = dict(R.inputs(7, R.MASKED), keep_policy=kp.cpu().numpy(), keep_pool=kq.cpu().numpy())
    ref = R.restatement(d)
    own = R.deviations(R.torch_route(d), ref)
    legal = torch.from_numpy(d["legal"]).cuda()
    results = {}
    for route in ("kernel", "torch"):
        t = [torch.from_numpy(d[k].copy()).cuda().requires_grad_(True) for k in ("tokens",) + R.FIELDS]
        out = TH.heads(t[0], legal, *t[1:], keep_policy=kp, keep_pool=kq, eps=R.EPS, route=route)
        torch.autograd.backward(list(out), [torch.from_numpy(d[k]).cuda() for k in R.UPSTREAM])
        results[route] = dict(zip(R.OUTPUTS, (o.detach().cpu().numpy() for o in out)), d_tokens=t[0].grad.cpu().numpy(),
                              **{"d_" + k: p.grad.cpu().numpy() for k, p in zip(R.FIELDS, t[1:])})
    held(results["kernel"], ref, own, "drawn keeps, kernel route")
    gpu_torch = R.deviations(results["torch"], ref)
    between = R.deviations(results["kernel"], dict(results["torch"], legal=ref["legal"], abs_ds=ref["abs_ds"], abs_dlogit=ref["abs_dlogit"]))
    for q in R.QUANTITIES:
        assert between[q] <= R.bound(own[q]) + max(gpu_torch[q], R.FLOOR), q
