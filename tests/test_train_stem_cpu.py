"""The Connect4 stem's training side without a GPU: the float64 restatement (tests/train_stem_ref.py) and the torch route
of `stem` (src/train_stem.py) against what the reference's own `CNN` returned for `_embed_state`, `hidden[0]` and
`hidden[1]` (fixture G25, tests/golden/make_golden_stem.py), `adopt_stem` / `restore_stem` on az_net.Connect4Net and on a
subclass with the reference's method name, the refusals, the layouts of the two pointer structs, float32 torch's own
deviation from float64 on the GPU tests' inputs (what their bounds rest on), and the exact zeros of the padding cases in
the restatement.

Tolerance against G25 (float32, as the reference computes it): every quantity within 1e-6 of its largest magnitude, the
bound tests/test_train_block_cpu.py uses for G23.  Measured: the restatement 1.6e-7 (dW, db) to 5.2e-7 (y) - that is
float32 torch's own rounding, the fixture's; the torch route 0 (it is the same ops)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_stem_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
INC = os.path.join(ROOT, "include")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g25_stem.npz")


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src import abi, az_net, train_stem
    return dict(TS=train_stem, NET=az_net, abi=abi)


@pytest.fixture(scope="module")
def g25():
    return dict(np.load(GOLDEN))


def test_fixture_is_the_seeded_inputs(env, g25):
    d = R.inputs(3, 0)
    for k in ("state", "dy") + R.PARAMS:
        assert np.array_equal(g25[k], d[k]), k
    state = g25["state"]
    assert state.shape == (3, 3, 6, 7) and set(np.unique(state)) <= {0.0, 1.0}
    assert not state[-1, :2].any() and state[0, :2].any() and not (state[:, 0] * state[:, 1]).any()
    assert np.abs(g25["b"]).max() > 0.05, "the bias is off its default"
    assert np.array_equal(g25["orbit_map"], R.ORBIT) and tuple(R.ORBIT) == env["TS"].ORBIT_MAP
    assert np.array_equal(env["NET"]._orbit_map().numpy(), R.ORBIT)


def test_restatement_and_torch_route_equal_the_reference(env, g25):
    TS = env["TS"]
    args = tuple(g25[k] for k in ("state",) + R.PARAMS + ("dy",))
    routes = {"restatement": R.restatement(*args),
              "torch route": R.torch_route(*args, fn=lambda *a: TS.stem(*a, route="torch"))}
    for name, got in routes.items():
        for q, d in sorted(R.deviations(got, {k: g25[k] for k in R.QUANTITIES}).items()):
            print("G25 %-12s %-3s %.3e" % (name, q, d))
            assert d <= 1e-6, (name, q, d)


def _seeded_net(NET, cls=None):
    torch.manual_seed(5)
    net = (cls or NET.Connect4Net)(device="cpu")
    with torch.no_grad():
        net.hidden[0].bias.normal_(0, 0.1)
        for lin in (net.policy_head.out, net.dual_head.value_out, net.dual_head.aux_out):
            lin.weight.normal_(0, 0.05)
    return net


def test_torch_route_is_the_hand_assembled_module_ops_bit_for_bit(env):
    TS, NET = env["TS"], env["NET"]
    net = _seeded_net(NET)
    d = R.inputs(7)
    state, dy = torch.from_numpy(d["state"].copy()), torch.from_numpy(d["dy"].copy())
    params = (net.piece_emb.weight, net.pos_emb.weight, net.hidden[0].weight, net.hidden[0].bias)
    want = net.hidden[1](net.hidden[0](net.embed(state)))
    want.backward(dy)
    grads = [p.grad.clone() for p in params]
    net.zero_grad(set_to_none=True)
    got = TS.stem(state, *params, route="torch")
    got.backward(dy)
    assert torch.equal(got, want) and got.stride() == want.stride()
    for p, g in zip(params, grads):
        assert torch.equal(p.grad, g)
    # CPU tensors take the torch route by default; the restatement's hand-assembled ops are the same ones
    with torch.no_grad():
        assert torch.equal(TS.stem(state, *params), want)
        assert torch.equal(R.module_ops(state, *params), want)


def _outputs_and_grads(net, state):
    net.zero_grad(set_to_none=True)
    out = net(state)
    (out[0].sum() + 2 * out[1][:, 0].sum() + 3 * out[2].sum()).backward()
    return [o.detach().clone() for o in out], [p.grad.clone() for p in net.parameters()]


def _adopt_restore(env, net):
    TS = env["TS"]
    net.train()
    keys, params = list(net.state_dict().keys()), [id(p) for p in net.parameters()]
    values = [v.clone() for v in net.state_dict().values()]
    state = torch.from_numpy(R.inputs(7)["state"].copy())
    before = _outputs_and_grads(net, state)
    assert TS.adopt_stem(net, route="torch") == 1
    assert net.embed(state) is state if hasattr(type(net), "embed") else True, "an adopted module's embed returns the state"
    during = _outputs_and_grads(net, state)
    assert list(net.state_dict().keys()) == keys and [id(p) for p in net.parameters()] == params
    assert TS.restore_stem(net) == 1 and TS.restore_stem(net) == 0
    after = _outputs_and_grads(net, state)
    for a, b, c in zip(before[0] + before[1], during[0] + during[1], after[0] + after[1]):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert all("forward" not in m.__dict__ for m in net.hidden.children())
    assert not any(k in net.__dict__ for k in ("embed", "_embed_state", "_az_stem_adopted"))
    assert list(net.state_dict().keys()) == keys and [id(p) for p in net.parameters()] == params
    assert all(torch.equal(a, b) for a, b in zip(values, net.state_dict().values()))


def test_adopt_and_restore_leave_the_module_as_it_was(env):
    _adopt_restore(env, _seeded_net(env["NET"]))


def test_adopt_and_restore_on_a_module_with_the_references_method_name(env):
    NET = env["NET"]

    class Named(NET.Connect4Net):
        """The reference's spelling: forward goes through `_embed_state`."""

        def _embed_state(self, state):
            return NET.Connect4Net.embed(self, state)

        def forward(self, x, action_mask=None):
            tokens = self.hidden(self._embed_state(x))
            return (self.policy_head(tokens, None),) + tuple(self.dual_head(tokens))

    net = _seeded_net(NET, Named)
    _adopt_restore(env, net)
    env["TS"].adopt_stem(net, route="torch")
    state = torch.from_numpy(R.inputs(2)["state"].copy())
    assert net._embed_state(state) is state
    env["TS"].restore_stem(net)
    assert net._embed_state(state).shape == (2, 32, 6, 7)


def test_adopt_stem_refuses_other_modules(env):
    TS, NET = env["TS"], env["NET"]
    with pytest.raises(ValueError, match="hidden"):
        TS.adopt_stem(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="route"):
        TS.adopt_stem(_seeded_net(NET), route="eager")
    net = _seeded_net(NET)
    net.orbit_map[3] = 5
    with pytest.raises(ValueError, match="orbit_map"):
        TS.adopt_stem(net)
    for change in (lambda n: n.hidden.__setitem__(0, torch.nn.Conv2d(32, 64, 3, padding=1, bias=False)),
                   lambda n: n.hidden.__setitem__(0, torch.nn.Conv2d(32, 64, 3, padding=0)),
                   lambda n: n.hidden.__setitem__(0, torch.nn.Conv2d(32, 64, 5, padding=1)),
                   lambda n: n.hidden.__setitem__(0, torch.nn.Conv2d(16, 64, 3, padding=1)),
                   lambda n: n.hidden.__setitem__(1, torch.nn.ReLU())):
        net = _seeded_net(NET)
        change(net)
        with pytest.raises(ValueError, match="3 x 3, 32 -> 64"):
            TS.adopt_stem(net)
        assert "_az_stem_adopted" not in net.__dict__ and "forward" not in net.hidden[0].__dict__
    with pytest.raises(ValueError, match="hidden"):
        TS.adopt_stem(NET.OthelloNet(device="cpu"))


def test_kernel_route_refuses_what_it_cannot_take(env):
    TS = env["TS"]
    d = R.inputs(2)
    state, E, P, W, b = (torch.from_numpy(d[k].copy()) for k in ("state",) + R.PARAMS)
    with pytest.raises(ValueError, match="CUDA"):
        TS.stem(state, E, P, W, b, route="kernel")
    with pytest.raises(ValueError, match="route"):
        TS.stem(state, E, P, W, b, route="eager")
    with pytest.raises(ValueError, match=r"\[N, 3, 6, 7\]"):
        TS.stem(torch.zeros(2, 2, 6, 7), E, P, W, b, route="kernel")
    with pytest.raises(ValueError, match="at least one sample"):
        TS.stem(torch.zeros(0, 3, 6, 7), E, P, W, b, route="kernel")
    with pytest.raises(ValueError, match="contiguous"):
        TS.stem(torch.zeros(2, 6, 7, 3).permute(0, 3, 1, 2), E, P, W, b, route="kernel")
    with pytest.raises(ValueError, match="float32"):
        TS.stem(state.double(), E, P, W, b, route="kernel")
    with pytest.raises(ValueError, match="float32"):
        TS.stem(state, E, P.double(), W, b, route="kernel")
    with pytest.raises(ValueError, match="pos_emb"):
        TS.stem(state, E, torch.zeros(10, 32), W, b, route="kernel")
    with pytest.raises(ValueError, match="conv_weight"):
        TS.stem(state, E, P, torch.zeros(64, 64, 3, 3), b, route="kernel")
    with pytest.raises(ValueError, match="contiguous"):
        TS.stem(state, E, P, torch.zeros(64, 3, 3, 32).permute(0, 3, 1, 2), b, route="kernel")


def test_pointer_structs_have_the_compilers_layout(env, tmp_path):
    abi = env["abi"]
    mirrors = {"az_train_stem_params": abi.TrainStemParamsC, "az_train_stem_grads": abi.TrainStemGradsC}
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "az_train.h"', "int main() {",
             '    printf("table bytes %d\\n", AZ_TRAIN_STEM_TABLE_BYTES);']
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
    want = {("table", "bytes"): env["TS"].TABLE_BYTES}
    for struct, mirror in mirrors.items():
        want[struct, "sizeof"] = C.sizeof(mirror)
        for field in mirror._fields_:
            want[struct, field[0]] = getattr(mirror, field[0]).offset
    assert got == want
    assert [C.sizeof(m) for m in mirrors.values()] == [32, 48]
    assert not any(m in abi.MIRRORS.values() for m in mirrors.values())
    names = [p[0] for p in abi.PROTOTYPES]
    at = names.index("az_train_stem_workspace_bytes")
    assert names[at - 1] == "az_train_dev_attn_bwd" and names[at:at + 3] == ["az_train_stem_workspace_bytes", "az_train_dev_stem_fwd",
                                                                            "az_train_dev_stem_bwd"]


@pytest.mark.parametrize("n", R.GPU_N + (R.DEFAULT_CAP + 1,))
def test_float32_torchs_own_deviation_on_the_gpu_tests_inputs(n):
    """Printed, and held loosely: float32 torch stays within 1e-5 of float64 on these inputs, so four times its
    deviation is still a bound that catches a wrong term (a dropped tap moves dW by percents)."""
    own = R.torch_deviations(n)
    print("N=%d " % n + "  ".join("%s %.2e" % (q, own[q]) for q in R.QUANTITIES))
    assert all(0 <= own[q] <= 1e-5 for q in R.QUANTITIES), own
    d, ref = R.inputs(n), R.reference(n)
    assert all(np.isfinite(ref[q]).all() for q in R.QUANTITIES)
    assert n == 1 or not d["state"][-1, :2].any(), "one sample is an empty board"
    if n == 1:
        for name in ("multipliers", "col0", "col6", "row0", "plane1"):
            own = R.case_reference(name)[1]
            print("%s " % name + "  ".join("%s %.2e" % (q, own[q]) for q in R.QUANTITIES))
            assert all(0 <= own[q] <= 1e-5 for q in R.QUANTITIES), (name, own)


def test_the_empty_board_is_the_position_map_alone():
    """On the empty board t is the positional embedding of the orbits, whatever the piece embeddings are."""
    d, ref = R.inputs(3), R.reference(3)
    want = d["P"][R.ORBIT].T.reshape(R.EMBED, R.ROWS, R.COLS)
    assert np.array_equal(ref["t"][-1], want.astype(np.float64))
    assert not np.array_equal(ref["t"][0], ref["t"][-1]) and ref["dt"].shape == (3, R.EMBED, R.CELLS)


def test_multiplier_inputs_are_multipliers_not_thresholds():
    d = R.multiplier_inputs()
    values = set(np.unique(d["state"][0, :2]))
    assert {0.5, -2.0} <= values and (d["state"][1, 0, 0, 0], d["state"][1, 1, 0, 0]) == (1.0, 1.0)
    ref = R.case_reference("multipliers")[0]
    thresholded = dict(d, state=(d["state"] > 0.25).astype(np.float32))
    assert R.dev(R.restatement(*R.args(thresholded))["y"], ref["y"]) > 1e-2
    cell = ref["t"][1, :, 0, 0]
    assert np.allclose(cell, d["E"][0].astype(np.float64) + d["E"][1] + d["P"][0], rtol=0, atol=1e-15)


@pytest.mark.parametrize("which", ("col0", "col6", "row0", "plane1"))
def test_padding_inputs_have_exact_zeros_in_the_restatement(which):
    d = R.padding_inputs(which)
    assert not d["state"][:, :2, :, 1:6].any() and d["state"][:, :2, :, 0].any() and d["state"][:, :2, :, 6].any()
    ref = R.case_reference(which)[0]
    zero, rest = R.exact_zeros(which, ref)
    assert not zero.any() and rest.any() and (rest != 0).mean() > 0.9
