"""The native learner without a GPU: the dropout contract's restatement (tests/learner_ref.py), the layout of the two
structs src/learner.py mirrors, what importing it pulls in, and what `NativeLearner` refuses.

The restatement is what tests/test_learner_gpu.py holds k_learn_keep to byte for byte, so its own properties are checked
here: the mixing function against plain Python integers, the kept share at p = 0.2 within 6 binomial standard deviations
of 0.8 (4096 groups per tensor: sigma = sqrt(0.8 * 0.2 / elements), derived from the count), zero bits above 41, the two
factor values, streams that differ by call and by tensor, and the threshold at the ends of [0, 1)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import learner_harness as LH
import learner_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
INC = os.path.join(ROOT, "include")
GROUPS = 4096
M64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def env():
    return LH.load_env()


def mix64_int(x):
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def draw_int(seed, call, a, b, j):
    s0 = mix64_int(seed ^ mix64_int((call + 0x9E3779B97F4A7C15 * (a + 1)) & M64) ^ (b << 32))
    return mix64_int((s0 + (j + 1) * 0x9E3779B97F4A7C15) & M64) >> 32


def test_the_restatement_is_the_generator():
    seed, call = 0xDEADBEEFCAFEF00D, 7
    d = LR.draws(seed, call, np.array([0, 1, 5, 2 ** 33 + 3], np.uint64), LR.KEEP_POLICY, 70)
    for gi, a in enumerate((0, 1, 5, 2 ** 33 + 3)):
        for j in (0, 1, 41, 63, 69):
            assert int(d[gi, j]) == draw_int(seed, call, a, LR.LEARN_STREAM + LR.KEEP_POLICY, j)


def within_six_sigma(kept, elements):
    sigma = (0.8 * 0.2 / elements) ** 0.5
    share = kept / elements
    print("kept share %.6f over %d elements, 6 sigma = %.6f" % (share, elements, 6 * sigma))
    return abs(share - 0.8) <= 6 * sigma


@pytest.mark.parametrize("tensor", (0, 2, LR.KEEP_POLICY, LR.KEEP_POOL))
def test_factors_at_a_fifth(tensor):
    f = LR.keep_factors(3, 1, GROUPS, tensor, 0.2)
    assert f.shape == (GROUPS, 64) and f.dtype == np.float32
    assert set(np.unique(f).tolist()) == {0.0, float(np.float32(1.25))} and LR.factor(0.2) == np.float32(1.25)
    assert within_six_sigma(int((f != 0).sum()), f.size)


def test_bits_at_a_fifth():
    n = GROUPS // (LR.HEADS * LR.TOKENS) + 1                    # at least 4096 words
    w = LR.keep_bits(3, 1, n, 0.2)
    assert w.shape == (n, 4, 42) and w.dtype == np.uint64 and w.size >= GROUPS
    assert not (w >> np.uint64(42)).any()
    kept = sum(int(((w >> np.uint64(j)) & np.uint64(1)).sum()) for j in range(42))
    assert within_six_sigma(kept, w.size * 42)
    # bit j of word a is draw j of group a
    d = LR.draws(3, 1, np.arange(5), LR.KEEP_ATTN, 42)
    flat = w.reshape(-1)
    for a in range(5):
        for j in (0, 17, 41):
            assert ((int(flat[a]) >> j) & 1) == int(d[a, j] >= LR.thr(0.2))


def test_another_call_or_tensor_gives_other_draws():
    base = LR.draws(3, 1, np.arange(64), 0, 64)
    assert np.array_equal(base, LR.draws(3, 1, np.arange(64), 0, 64))
    for other in (LR.draws(3, 2, np.arange(64), 0, 64), LR.draws(3, 1, np.arange(64), 1, 64), LR.draws(4, 1, np.arange(64), 0, 64),
                  LR.draws(3, 1, np.arange(64), LR.KEEP_POOL, 64)):
        assert (other != base).mean() > 0.99
    assert (base[0] != base[1]).mean() > 0.9                   # and another group


def test_thresholds():
    assert LR.thr(0.0) == 0                                     # every draw is kept
    assert LR.thr(0.5) == 1 << 31
    assert LR.thr(1.0 - 2.0 ** -33) == 0xFFFFFFFF               # floor(2^32 - 0.5 + 0.5) = 2^32 counts as 2^32 - 1
    assert LR.thr(0.2) == int(np.floor(0.2 * 2.0 ** 32 + 0.5)) == 858993459
    k = LR.keeps(1, 0, 3, 3, (0.5, 0.0, 0.1, 0.0))
    assert k["attn"] is None and k["pool"] is None and len(k["blocks"]) == 3 and k["policy"].shape == (3, 7, 64)


def test_struct_mirrors_have_the_compilers_layout(env, tmp_path):
    LN = env["LN"]
    assert set(LN.MIRRORS) == {"az_learn_config", "az_learn_out"}
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "az_train.h"', "int main() {"]
    for struct, mirror in LN.MIRRORS.items():
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (struct, struct))
        for field in mirror._fields_:
            lines.append('    printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));'
                         % (struct, field[0], struct, field[0], struct, field[0]))
    for name in ("AZ_LEARN_CONFIG_BYTES", "AZ_LEARN_OUT_BYTES", "AZ_LEARN_ROLE_BLOCK", "AZ_LEARN_ROLE_ATTN", "AZ_LEARN_ROLE_HEADS",
                 "AZ_LEARN_ROLES", "AZ_LEARN_MAX_BLOCKS", "AZ_LEARN_KEEP_ATTN", "AZ_LEARN_KEEP_POLICY", "AZ_LEARN_KEEP_POOL"):
        lines.append('    printf("define %s %%d 0\\n", (int)%s);' % (name, name))
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["g++", "-std=c++17", "-I", INC, str(src), "-o", str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        struct, field, *numbers = ln.split()
        got[struct, field] = tuple(int(n) for n in numbers)
    want = {}
    for struct, mirror in LN.MIRRORS.items():
        want[struct, "sizeof"] = (C.sizeof(mirror),)
        for field in mirror._fields_:
            d = getattr(mirror, field[0])
            want[struct, field[0]] = (d.offset, d.size)
    defines = {k[1]: v[0] for k, v in got.items() if k[0] == "define"}
    assert {k: v for k, v in got.items() if k[0] != "define"} == want
    assert defines["AZ_LEARN_CONFIG_BYTES"] == C.sizeof(LN.LearnConfigC) and defines["AZ_LEARN_OUT_BYTES"] == C.sizeof(LN.LearnOutC)
    assert (defines["AZ_LEARN_ROLE_BLOCK"], defines["AZ_LEARN_ROLE_ATTN"], defines["AZ_LEARN_ROLE_HEADS"], defines["AZ_LEARN_ROLES"]) == \
        (LN.ROLE_BLOCK, LN.ROLE_ATTN, LN.ROLE_HEADS, LN.ROLES)
    assert defines["AZ_LEARN_MAX_BLOCKS"] == LN.MAX_BLOCKS
    assert (defines["AZ_LEARN_KEEP_ATTN"], defines["AZ_LEARN_KEEP_POLICY"], defines["AZ_LEARN_KEEP_POOL"]) == \
        (LN.KEEP_ATTN, LN.KEEP_POLICY, LN.KEEP_POOL) == (LR.KEEP_ATTN, LR.KEEP_POLICY, LR.KEEP_POOL)


def test_the_stream_constant_is_the_headers():
    text = open(os.path.join(PKG, "csrc", "dev_rng.h")).read()
    assert "LEARN_STREAM = 0x%X;" % LR.LEARN_STREAM in text


def test_importing_the_learner_does_not_import_the_engine(env):
    code = ("import sys; sys.path.insert(0, %r); import src.learner; "
            "print(sorted(m for m in ('src.MCTS_cpp', 'src.mcts_cpp', 'src.selfplay', 'src.match') if m in sys.modules))" % PKG)
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "[]"


def test_what_the_learner_refuses(env):
    torch, LN, NET, O = env["torch"], env["LN"], env["NET"], env["O"]
    with pytest.raises(ValueError, match="CUDA"):
        LN.NativeLearner(LH.module(env, "cpu"), 128)                    # the right module on the wrong device
    with pytest.raises(ValueError, match="hidden"):
        LN.NativeLearner(NET.OthelloNet(device="cpu"), 128)
    narrow = NET.Connect4Net(h_dim=32, heads=2, device="cpu")
    narrow.opt = torch.optim.AdamW(O.reference_param_groups(narrow, 1e-3), lr=1e-3)
    with pytest.raises(ValueError):
        LN.NativeLearner(narrow, 128)
    with pytest.raises(ValueError, match="max_rows"):
        LN.NativeLearner(LH.module(env, "cpu"), 0)
    with pytest.raises(ValueError, match="rate"):
        LN.NativeLearner(LH.module(env, "cpu", dropout=(0.0, 0.0, 1.0, 0.0)), 128)
    assert LN.keep_factor(0.2) == float(np.float32(1.25)) == float(LR.factor(0.2))
    assert LN.keep_factor(0.1) == float(LR.factor(0.1))
