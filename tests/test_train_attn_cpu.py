"""The gated attention block's training side without a GPU: the float64 restatement (tests/train_attn_ref.py) and the
torch route of `gated_attention` (src/train_attn.py) against what the reference's own `AttentionBlock` returned (fixture
G24, tests/golden/make_golden_attn.py), the mask bits' conventions, `draw_keep_bits`, `adopt_attention` /
`restore_attention` on the reference-shaped Connect4 module, the refusals of the kernel route, the layouts of the two
pointer structs, and float32 torch's own deviation from float64 on the GPU tests' inputs (what their bounds rest on).

Tolerance against G24 (float32, as the reference computes it): every quantity within 1e-6 of its largest magnitude, the
bound tests/test_train_block_cpu.py uses for G23."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_attn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
INC = os.path.join(ROOT, "include")
GOLDEN = os.path.join(ROOT, "tests", "golden", "g24_gated_attention.npz")


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src import abi, az_net, train_attn
    return dict(TA=train_attn, NET=az_net, abi=abi)


@pytest.fixture(scope="module")
def g24():
    return dict(np.load(GOLDEN))


def route_block(TA):
    return lambda *a: TA.gated_attention(*a, route="torch")


def tensors(d, dtype=torch.float32):
    return [torch.tensor(d[k], dtype=dtype) for k in ("x",) + R.PARAMS]


def test_fixture_is_the_seeded_inputs(g24):
    d = R.inputs(3, 0)
    for k in ("x", "dy") + R.PARAMS:
        assert np.array_equal(g24[k], d[k]), k
    assert g24["x"].shape == (3, 64, 6, 7) and not g24["x"][-1].any() and float(g24["eps"]) == R.EPS
    assert g24["y"].shape == (3, 42, 64) and np.abs(g24["qn"] - 1).max() > 0.1 and np.abs(g24["pre"] - 1).max() > 0.1


def test_restatement_and_torch_route_equal_the_reference(env, g24):
    args = tuple(g24[k] for k in ("x",) + R.PARAMS) + (None, 1.0, g24["dy"], float(g24["eps"]))
    routes = {"restatement": R.restatement(*args), "torch route": R.torch_route(*args, block=route_block(env["TA"]))}
    for name, got in routes.items():
        for q, d in sorted(R.deviations(got, g24).items()):
            print("G24 %-12s %-7s %.3e" % (name, q, d))
            assert d <= 1e-6, (name, q, d)


def test_mask_bit_conventions(env):
    """All-ones bits with scale 1 are null bits; all-zero bits leave the tokens EXACTLY; bits 42 .. 63 change nothing."""
    TA = env["TA"]
    d = R.inputs(2, R.KEEP_P)
    t = tensors(d)
    null = TA.gated_attention(*t)
    ones = torch.full((2, 4, 42), R.LOW, dtype=torch.int64)
    assert torch.equal(TA.gated_attention(*t, keep_bits=ones, keep_scale=1.0), null)
    assert torch.equal(TA.gated_attention(*t, keep_bits=torch.full((2, 4, 42), -1, dtype=torch.int64), keep_scale=1.0), null)
    zeros = TA.gated_attention(*t, keep_bits=torch.zeros((2, 4, 42), dtype=torch.int64), keep_scale=1.25)
    assert torch.equal(zeros, t[0].flatten(2).transpose(1, 2))
    bits = torch.from_numpy(d["bits"])
    assert (bits >> 42).ne(0).any(), "the seeded words carry garbage above bit 41"
    a = TA.gated_attention(*t, keep_bits=bits, keep_scale=d["keep_scale"])
    b = TA.gated_attention(*t, keep_bits=bits & R.LOW, keep_scale=d["keep_scale"])
    assert torch.equal(a, b) and not torch.equal(a, null)
    assert torch.equal(TA.keep_mask(bits, torch.float64), torch.from_numpy(R.mask_of(d["bits"], 2)))
    # the restatement reads the words the same way
    ref_a = R.restatement(*[d[k] for k in ("x",) + R.PARAMS], d["bits"], d["keep_scale"], d["dy"])
    ref_b = R.restatement(*[d[k] for k in ("x",) + R.PARAMS], d["bits"] & R.LOW, d["keep_scale"], d["dy"])
    assert all(np.array_equal(ref_a[q], ref_b[q]) for q in R.QUANTITIES)
    assert R.dev(a.numpy(), ref_a["y"]) <= 1e-5


def test_draw_keep_bits(env):
    TA = env["TA"]
    gen = torch.Generator().manual_seed(5)
    bits, scale = TA.draw_keep_bits(64, 0.2, "cpu", gen)
    assert bits.shape == (64, 4, 42) and bits.dtype == torch.int64 and scale == pytest.approx(1.25)
    assert (bits >> 42).eq(0).all(), "a bit at 42 or above is set"
    kept = TA.keep_mask(bits).sum().item() / (64 * 4 * 42 * 42)
    sigma = (0.8 * 0.2 / 451584) ** 0.5
    print("kept %.5f of 451584 bits, 5 sigma = %.5f" % (kept, 5 * sigma))
    assert 64 * 4 * 42 * 42 == 451584 and abs(kept - 0.8) <= 5 * sigma <= 0.003
    again, _ = TA.draw_keep_bits(64, 0.2, "cpu", torch.Generator().manual_seed(5))
    assert torch.equal(bits, again)
    assert TA.draw_keep_bits(3, 0.0, "cpu") == (None, 1.0)
    none, scale = TA.draw_keep_bits(3, 1.0, "cpu")
    assert none.shape == (3, 4, 42) and not none.any() and scale == 1.0


def test_adopt_and_restore_leave_the_module_as_it_was(env):
    TA, NET = env["TA"], env["NET"]
    torch.manual_seed(5)
    net = NET.Connect4Net(device="cpu")
    with torch.no_grad():                       # the reference zeroes the heads' output weights: move them off zero
        for lin in (net.policy_head.out, net.dual_head.value_out, net.dual_head.aux_out):
            lin.weight.normal_(0, 0.05)
    keys, params = list(net.state_dict().keys()), [id(p) for p in net.parameters()]
    state = torch.zeros(4, 3, 6, 7)
    state[:, 0, 5, 3], state[:, 1, 5, 2], state[:, 2] = 1.0, 1.0, 1.0
    state[1, 0, 4, 3] = 1.0

    def run():
        net.zero_grad(set_to_none=True)
        out = net(state)
        (out[0][:, 2].sum() + out[1][:, 0].sum() + out[2].sum()).backward()
        return [o.detach().clone() for o in out], [p.grad.clone() for p in net.parameters()]

    before = run()
    assert TA.adopt_attention(net, route="torch") == 1
    during = run()
    assert list(net.state_dict().keys()) == keys and [id(p) for p in net.parameters()] == params
    assert TA.restore_attention(net) == 1 and TA.restore_attention(net) == 0
    after = run()
    # outputs against their own largest magnitude; gradients against the module's largest gradient entry: some
    # (a bias in front of a softmax) are zero but for rounding and have no magnitude of their own to be measured by
    grad_scale = max(g.abs().max().item() for g in before[1])
    for i, (a, b, c) in enumerate(zip(before[0] + before[1], during[0] + during[1], after[0] + after[1])):
        scale = a.abs().max().item() if i < len(before[0]) else grad_scale
        assert (a - b).abs().max().item() <= 1e-6 * scale and torch.equal(a, c)
    assert all("forward" not in m.__dict__ for m in net.hidden.children())
    with pytest.raises(ValueError, match="hidden"):
        TA.adopt_attention(torch.nn.Linear(2, 2))
    net.hidden[-1].attn.q_norm.eps = 1e-6
    with pytest.raises(ValueError, match="eps"):
        TA.adopt_attention(net)
    bare = torch.nn.Module()
    bare.hidden = torch.nn.Sequential(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="attention"):
        TA.adopt_attention(bare)


def test_adopted_dropout_draws_in_training_only(env):
    TA, NET = env["TA"], env["NET"]
    torch.manual_seed(9)
    net = NET.Connect4Net(device="cpu")
    block = net.hidden[-1]
    block.attn.dropout_p = 0.2
    TA.adopt_attention(net, route="torch")
    x = torch.randn(5, 64, 6, 7)
    with torch.no_grad():
        net.eval()
        a, b = block(x), block(x)
        net.train()
        torch.manual_seed(1)
        c = block(x)
        torch.manual_seed(1)
        d = block(x)
    assert torch.equal(a, b) and torch.equal(c, d) and not torch.equal(a, c) and torch.isfinite(c).all()


def test_kernel_route_refuses_what_it_cannot_take(env):
    TA = env["TA"]
    t = tensors(R.inputs(2, 0))
    with pytest.raises(ValueError, match="CUDA"):
        TA.gated_attention(*t, route="kernel")
    with pytest.raises(ValueError, match="route"):
        TA.gated_attention(*t, route="eager")
    with pytest.raises(ValueError, match=r"\[N, 64, 6, 7\]"):
        TA.gated_attention(torch.zeros(2, 16, 6, 7), *t[1:], route="kernel")
    with pytest.raises(ValueError, match="float32"):
        TA.gated_attention(t[0].double(), *t[1:], route="kernel")
    with pytest.raises(ValueError, match="qkv_weight"):
        TA.gated_attention(t[0], t[1], t[2][:, :32], *t[3:], route="kernel")
    with pytest.raises(ValueError, match="keep_bits"):
        TA.gated_attention(*t, keep_bits=torch.zeros(2, 4, 41, dtype=torch.int64), keep_scale=1.25, route="kernel")
    with pytest.raises(ValueError, match="keep_scale"):
        TA.gated_attention(*t, keep_scale=1.25, route="kernel")


def test_pointer_structs_have_the_compilers_layout(env, tmp_path):
    abi = env["abi"]
    mirrors = {"az_train_attn_params": abi.TrainAttnParamsC, "az_train_attn_grads": abi.TrainAttnGradsC}
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "az_train.h"', "int main() {"]
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
    want = {}
    for struct, mirror in mirrors.items():
        want[struct, "sizeof"] = C.sizeof(mirror)
        for field in mirror._fields_:
            want[struct, field[0]] = getattr(mirror, field[0]).offset
    assert got == want
    assert [C.sizeof(m) for m in mirrors.values()] == [48, 72]


@pytest.mark.parametrize("n", R.GPU_N)
def test_float32_torchs_own_deviation_on_the_gpu_tests_inputs(n):
    """Printed, and held loosely: float32 torch stays within 2e-5 of float64 on these inputs (the large-logit case
    included), so four times its deviation is still a bound that catches a wrong term."""
    cases = [(n, R.KEEP_P, 1.0), (n, 0.0, 1.0)] + ([(7, R.KEEP_P, 6.0)] if n == 7 else [])
    for case in cases:
        own, ref = R.torch_deviations(*case), R.reference(*case)
        print("N=%d keep_p=%.1f qk_scale=%g " % case + "  ".join("%s %.2e" % (q, own[q]) for q in R.QUANTITIES))
        assert all(0 <= own[q] <= 2e-5 for q in R.QUANTITIES), own
        assert all(np.isfinite(ref[q]).all() for q in R.QUANTITIES)
