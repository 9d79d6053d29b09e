"""The Connect4 heads' training side without a GPU: the float64 restatement (tests/train_heads_ref.py) and the torch route
of `heads` (src/train_heads.py) against what the reference's own `ColumnPolicyHead` and `DualHead` returned, forward and
autograd (fixture G26, tests/golden/make_golden_heads.py); `adopt_heads` / `restore_heads` / `adopt_all` on
az_net.Connect4Net with the torch route against the class's forward; the refusals; the layouts of the two pointer structs;
and float32 torch's own deviation from float64 on the GPU tests' inputs (what their bounds rest on).

Deviations are measured as tests/train_heads_ref.py says (log_p on legal entries, the two cancelling sums over the sum of
their terms' absolute values).  Tolerances: G26 is float32 torch, so the float64 restatement may differ from it by float32
torch's own rounding, which the project's rule floors at 1e-6 (measured on these inputs: 2e-8 to 8e-7); the torch route is
a second float32 route with other roundings (rsqrt where the module has rms_norm), so it may differ from G26 by two such
roundings, 2e-6, and from the restatement by one.  An illegal log_p entry is about -1e9, one float32 ulp there is 64: held
to 64 absolutely."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_heads_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
INC = os.path.join(ROOT, "include")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g26_heads.npz")
ONE_ROUNDING, TWO_ROUNDINGS = 1e-6, 2e-6


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src import abi, az_net, train_attn, train_block, train_heads, train_stem
    return dict(TH=train_heads, TS=train_stem, TB=train_block, TA=train_attn, NET=az_net, abi=abi)


@pytest.fixture(scope="module")
def g26():
    return dict(np.load(GOLDEN))


def route_fn(TH):
    return lambda tok, legal, params, kp, kq: TH.heads(tok, legal, *params, keep_policy=kp, keep_pool=kq, eps=R.EPS, route="torch")


def test_fixture_is_the_seeded_inputs(g26):
    d = R.inputs(3, R.MASKED)
    for k in ("tokens", "legal") + R.FIELDS + R.UPSTREAM:
        assert np.array_equal(g26[k], d[k]), k
    assert g26["legal"][0].all() and not g26["legal"][1].any() and not g26["tokens"][-1].any() and g26["tokens"][0].any()
    assert d["keep_policy"] is None and d["keep_pool"] is None, "the reference's heads ran with dropout 0"
    for k in ("policy_out_weight", "value_out_weight", "aux_out_weight"):
        assert np.abs(g26[k]).max() > 0.05, "%s is off the zero the reference gives it" % k
    assert g26["d_log_p"][~g26["legal"]].all(), "the upstream gradient is non-zero on illegal entries"
    assert os.path.getsize(GOLDEN) < 230 * 1024
    # all seven illegal: every entry is -log 7, as torch gives
    assert np.allclose(g26["log_p"][1], -np.log(7.0), rtol=0, atol=1e-6)


def test_restatement_and_torch_route_hold_against_the_reference(env, g26):
    d = R.inputs(3, R.MASKED)
    ref = R.reference(3, R.MASKED)
    golden = dict(g26, abs_ds=ref["abs_ds"], abs_dlogit=ref["abs_dlogit"])       # the terms' sizes: float64's
    torch_route = R.torch_route(d, fn=route_fn(env["TH"]))
    for name, got, against, tol in (("restatement", ref, golden, ONE_ROUNDING), ("torch route", torch_route, golden, TWO_ROUNDINGS),
                                    ("torch route vs restatement", torch_route, ref, ONE_ROUNDING)):
        devs = R.deviations(got, against)
        for q, v in devs.items():
            print("G26 %-27s %-22s %.3e" % (name, q, v))
        for q, v in devs.items():
            assert v <= (R.ILLEGAL_ABS if q == "log_p_illegal" else tol), (name, q, v)
    # exact arithmetic makes d_row_gate_bias zero: float64 leaves 1e-15 of the terms' size
    assert abs(ref["d_row_gate_bias"][0]) <= 1e-13 * ref["abs_ds"]


def test_restatement_properties():
    """What the GPU tests' named cases rest on, in float64: the mask's gradient, the all-illegal row, the zero sample."""
    d, ref = R.inputs(7, R.KEPT), R.reference(7, R.KEPT)
    legal = d["legal"]
    assert legal[0].all() and not legal[1].any() and legal[2:].any() and not legal[2:].all()
    assert np.allclose(ref["log_p"][1], -np.log(7.0), rtol=0, atol=1e-12)
    assert (ref["log_p"][~legal] < -9e8).sum() == (~legal[[0, 2, 3, 4, 5, 6]]).sum()
    assert not d["keep_policy"][0, 2].any() and not d["keep_pool"][3].any() and not d["tokens"][-1].any()
    assert all(np.isfinite(ref[q]).all() for q in R.QUANTITIES)
    assert np.abs(ref["d_tokens"][-1]).max() > 0, "the zero sample still gets a gradient"
    # without the mask's zero on illegal entries the policy gradients move by far more than any bound
    plain = R.reference(7, R.PLAIN)
    assert R.dev(plain["d_policy_fc_weight"], R.reference(7, R.MASKED)["d_policy_fc_weight"]) > 1e-2
    sat = R.reference(7, R.SATURATED)
    assert np.isfinite(sat["log_p"]).all() and np.abs(sat["log_p"][legal]).max() > 89 and sat["row_score_max"] > 89, \
        "the saturated case's row scores and logits pass what exp takes in float32: without the maxima taken out it overflows"


def _seeded_net(NET, cls=None, seed=5):
    torch.manual_seed(seed)
    net = (cls or NET.Connect4Net)(device="cpu")
    with torch.no_grad():
        for p in list(net.policy_head.parameters()) + list(net.dual_head.parameters()):
            p.add_(0.05 * torch.randn_like(p))
    return net


def _outputs_and_grads(net, state, mask):
    net.zero_grad(set_to_none=True)
    out = net(state, mask)
    (out[0][out[0] > -1e8].sum() + 2 * out[1][:, 0].sum() + 3 * out[2].sum()).backward()
    grads = {k: p.grad.clone() for k, p in net.named_parameters()}
    # d row_gate.bias and d out.bias are zero in exact arithmetic (a softmax ignores a shift; with no gradient on illegal
    # entries d_logit adds to zero): what they hold is rounding of their terms, the same terms the weight's gradient sums
    # with factors of order one - so each is measured on its weight gradient's scale
    for layer in ("policy_head.row_gate", "policy_head.out"):
        grads[layer + ".weight"] = torch.cat([grads[layer + ".weight"].reshape(-1), grads.pop(layer + ".bias")])
    return [o.detach().clone() for o in out], list(grads.values())


def _close(a, b, tol):
    legal = a > -1e8
    assert torch.equal(legal, b > -1e8)
    scale = a[legal].abs().max()
    assert (a[legal] - b[legal]).abs().max() <= tol * scale, ((a[legal] - b[legal]).abs().max() / scale)
    assert (a[~legal] - b[~legal]).abs().max() <= R.ILLEGAL_ABS if (~legal).any() else True


def _state_and_mask(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    stone = torch.randint(0, 3, (n, 6, 7), generator=g)
    state = torch.stack([(stone == 1).float(), (stone == 2).float(), torch.ones(n, 6, 7)], 1)
    mask = torch.rand(n, 7, generator=g) < 0.7
    mask[0] = True
    return state, mask


@pytest.mark.parametrize("which", ("heads", "all"))
def test_adopt_and_restore_leave_the_module_as_it_was(env, which):
    """The adopted module with the torch route against the class's forward, outputs and every parameter's gradient.  Each
    adopted piece is another float32 route of the same formulas, within one float32 rounding (1e-6 of the quantity's
    largest magnitude) of the class's ops, which have their own: with the heads alone two roundings; with all six pieces
    adopted (three blocks, attention, stem, heads) a gradient that flows through all of them may gather seven."""
    TH = env["TH"]
    tol = TWO_ROUNDINGS if which == "heads" else 7 * ONE_ROUNDING
    net = _seeded_net(env["NET"]).train()
    keys, params = list(net.state_dict().keys()), [id(p) for p in net.parameters()]
    values = [v.clone() for v in net.state_dict().values()]
    state, mask = _state_and_mask(5)
    before = _outputs_and_grads(net, state, mask)
    if which == "heads":
        assert TH.adopt_heads(net, route="torch") == 1
    else:
        assert TH.adopt_all(net, route="torch") == (3, 1, 1, 1)
        assert net.embed(state) is state, "adopt_stem's pass-through is what the adopted forward finds on the instance"
    during = _outputs_and_grads(net, state, mask)
    # the mask as the class takes it: a numpy array, and one row without the batch dimension
    as_numpy = net(state, mask.numpy())
    assert all(torch.equal(a, b) for a, b in zip(as_numpy, net(state, mask)))
    one = net(state[:1], mask[0].numpy())
    assert one[0].shape == (1, 7) and torch.allclose(one[1], during[0][1][:1], rtol=0, atol=1e-5)
    assert net(state)[0].shape == (5, 7), "no mask: all legal"
    assert list(net.state_dict().keys()) == keys and [id(p) for p in net.parameters()] == params
    if which == "heads":
        assert TH.restore_heads(net) == 1 and TH.restore_heads(net) == 0
    else:
        assert TH.restore_all(net) == (3, 1, 1, 1) and TH.restore_all(net) == (0, 0, 0, 0)
    after = _outputs_and_grads(net, state, mask)
    for a, b, c in zip(before[0] + before[1], during[0] + during[1], after[0] + after[1]):
        _close(a, b, tol)
        assert torch.equal(a, c)
    assert "forward" not in net.__dict__ and "_az_heads_adopted" not in net.__dict__
    assert all(torch.equal(a, b) for a, b in zip(values, net.state_dict().values()))


def test_adopted_dropout_draws_in_training_mode_only(env):
    TH = env["TH"]
    net = _seeded_net(env["NET"])
    net.policy_head.dropout = torch.nn.Dropout(0.2)
    net.dual_head.pool_drop = torch.nn.Dropout(0.2)
    TH.adopt_heads(net, route="torch")
    state, mask = _state_and_mask(9)
    net.train()
    a, b = net(state, mask), net(state, mask)
    assert not torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    torch.manual_seed(1)
    a = net(state, mask)
    torch.manual_seed(1)
    b = net(state, mask)
    assert all(torch.equal(x, y) for x, y in zip(a, b)), "the same seed draws the same factors"
    net.eval()
    a, b = net(state, mask), net(state, mask)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    keep = TH.draw_keep((4000, 64), 0.2, "cpu")
    assert set(np.unique(keep.numpy())) == {np.float32(0.0), np.float32(1.25)} and abs(float(keep.mean()) - 1.0) < 0.02
    assert TH.draw_keep((2, 2), 0.0, "cpu") is None and not TH.draw_keep((2, 2), 1.0, "cpu").any()


def test_adopt_heads_refuses_other_modules(env):
    TH, NET = env["TH"], env["NET"]
    with pytest.raises(ValueError, match="policy_head"):
        TH.adopt_heads(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="route"):
        TH.adopt_heads(_seeded_net(NET), route="eager")
    with pytest.raises(ValueError, match="hidden"):
        TH.adopt_heads(NET.OthelloNet(device="cpu"))
    net = _seeded_net(NET)
    net.dual_head.value_out = torch.nn.Linear(64, 2)
    with pytest.raises(ValueError, match="dual_head.value_out.weight"):
        TH.adopt_heads(net)
    net = _seeded_net(NET)
    net.policy_head.fc = torch.nn.Linear(64, 64, bias=False)
    with pytest.raises(ValueError, match="policy_head.fc.bias"):
        TH.adopt_heads(net)
    for change in (lambda n: setattr(n.dual_head, "norm", torch.nn.RMSNorm(64, eps=1e-6)),
                   lambda n: setattr(n.policy_head, "norm", torch.nn.RMSNorm(64))):
        net = _seeded_net(NET)
        change(net)
        with pytest.raises(ValueError, match="one explicit eps"):
            TH.adopt_heads(net)
        assert "forward" not in net.__dict__ and "_az_heads_adopted" not in net.__dict__
    # adopt_all undoes what it had adopted before the refusal
    net = _seeded_net(NET)
    net.dual_head.norm = torch.nn.RMSNorm(64, eps=1e-6)
    with pytest.raises(ValueError, match="one explicit eps"):
        TH.adopt_all(net, route="torch")
    assert TH.restore_all(net) == (0, 0, 0, 0)


def test_kernel_route_refuses_what_it_cannot_take(env):
    TH = env["TH"]
    d = R.inputs(2, R.KEPT)
    tok, legal = torch.from_numpy(d["tokens"].copy()), torch.from_numpy(d["legal"].copy())
    params = [torch.from_numpy(d[k].copy()) for k in R.FIELDS]
    kp, kq = torch.from_numpy(d["keep_policy"].copy()), torch.from_numpy(d["keep_pool"].copy())

    def call(tokens=tok, legal=legal, params=params, **kw):
        return TH.heads(tokens, legal, *params, route="kernel", **kw)
    with pytest.raises(ValueError, match="CUDA"):
        call()
    with pytest.raises(ValueError, match="route"):
        TH.heads(tok, legal, *params, route="eager")
    with pytest.raises(ValueError, match=r"\[N, 42, 64\]"):
        call(tokens=torch.zeros(2, 64, 42))
    with pytest.raises(ValueError, match="at least one sample"):
        call(tokens=torch.zeros(0, 42, 64), legal=None)
    with pytest.raises(ValueError, match="float32"):
        call(tokens=tok.double())
    with pytest.raises(ValueError, match="dtype bool"):
        call(legal=legal.float())
    with pytest.raises(ValueError, match="dtype bool"):
        call(legal=legal[:1])
    with pytest.raises(ValueError, match="value_out_weight"):
        call(params=params[:14] + [torch.zeros(2, 64)] + params[15:])
    with pytest.raises(ValueError, match="contiguous"):
        call(params=params[:3] + [params[3].t()] + params[4:])
    with pytest.raises(ValueError, match="keep_policy"):
        call(keep_policy=kp[:, :6])
    with pytest.raises(ValueError, match="keep_pool"):
        call(keep_pool=kq[:1])
    # CPU tensors take the torch route by default
    out = TH.heads(tok, legal, *params, keep_policy=kp, keep_pool=kq)
    assert [tuple(o.shape) for o in out] == [(2, 7), (2, 3), (2,)]


def test_pointer_structs_have_the_compilers_layout(env, tmp_path):
    abi = env["abi"]
    mirrors = {"az_train_heads_params": abi.TrainHeadsParamsC, "az_train_heads_grads": abi.TrainHeadsGradsC}
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "az_train.h"', "int main() {",
             '    printf("params bytes %d\\n", AZ_TRAIN_HEADS_PARAMS_BYTES);', '    printf("grads bytes %d\\n", AZ_TRAIN_HEADS_GRADS_BYTES);']
    for struct, mirror in mirrors.items():
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (struct, struct))
        for field in mirror._fields_:
            lines.append('    printf("%s %s %%zu\\n", offsetof(%s, %s));' % (struct, field[0], struct, field[0]))
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["g++", "-std=c++17", "-I", INC, str(src), "-o", str(exe)], check=True)
    got = {tuple(ln.split()[:2]): int(ln.split()[2]) for ln in
           subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()}
    want = {("params", "bytes"): 144, ("grads", "bytes"): 168}
    for struct, mirror in mirrors.items():
        want[struct, "sizeof"] = C.sizeof(mirror)
        for field in mirror._fields_:
            want[struct, field[0]] = getattr(mirror, field[0]).offset
    assert got == want
    assert [C.sizeof(m) for m in mirrors.values()] == [144, 168]
    assert not any(m in abi.MIRRORS.values() for m in mirrors.values())
    # the mirrors, the module's table and the tests' list name the eighteen parameters in one order
    assert tuple(f[0] for f in abi.TrainHeadsParamsC._fields_) == R.FIELDS == tuple(p[0] for p in env["TH"].PARAMS)
    assert tuple(f[0] for f in abi.TrainHeadsGradsC._fields_) == ("d_tokens",) + R.GRADS + ("workspace", "workspace_bytes")
    assert tuple(p[2] for p in env["TH"].PARAMS) == R.SHAPES and sum(int(np.prod(s)) for s in R.SHAPES) == 13126
    names = [p[0] for p in abi.PROTOTYPES]
    at = names.index("az_train_heads_workspace_bytes")
    assert names[at - 1] == "az_train_dev_stem_bwd" and names[at:] == ["az_train_heads_workspace_bytes", "az_train_dev_heads_fwd",
                                                                       "az_train_dev_heads_bwd"]


CASES = [(n, case) for case in (R.KEPT, R.PLAIN) for n in R.GPU_N] + [(R.DEFAULT_CAP + 1, R.KEPT), (7, R.SATURATED)]


@pytest.mark.parametrize("n,case", CASES)
def test_float32_torchs_own_deviation_on_the_gpu_tests_inputs(n, case):
    """Printed, and held loosely: float32 torch stays within 1e-5 of float64 on these inputs, so four times its
    deviation is still a bound that catches a wrong term; on illegal entries it is off by less than one ulp of 1e9."""
    own = R.torch_deviations(n, case)
    print("N=%d case=%d " % (n, case) + "  ".join("%s %.2e" % (q, v) for q, v in own.items()))
    assert all(0 <= own[q] <= 1e-5 for q in R.QUANTITIES), own
    assert own["log_p_illegal"] <= R.ILLEGAL_ABS
    ref = R.reference(n, case)
    assert all(np.isfinite(ref[q]).all() for q in R.QUANTITIES)
    assert n == 1 or not R.inputs(n, case)["tokens"][-1].any(), "one sample is all zero"
