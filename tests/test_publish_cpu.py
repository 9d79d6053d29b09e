"""Publishing weights without a GPU: the numpy restatement of the evaluator's layout function (tests/publish_ref.py, what
tests/test_publish_gpu.py holds k_publish to byte for byte) against the inference twin built on the CPU, and the layout of
the struct src/publish.py mirrors.

* every buffer of `FastConnect4Net(state_dict, "cpu")` except the folded stem's two equals the restatement in bytes, in
  the twin's MEMORY order;
* the folded stem against a float64 evaluation on the same bf16-rounded weights, within bounds that are DERIVED (u = 2^-24,
  S the sum of absolute products of an entry):
      |hi + lo - T64| <= 34 u S + 2^-17 |T64|     32 products and 32 additions of relative error u each, first order,
                                                  plus what two bf16 halves can hold of a float32 (2 x 8 significand bits,
                                                  the low half's rounding is 2^-9 of a remainder below 2^-8 |T|)
      |pmap - P64|      <= 290 u S'               at most 9 x 32 products, as many additions and the bias: the running sum
                                                  passes 289 roundings, a product one, |b| is inside S'
  `fast_net.fold_stem` is held to the same two bounds: the reference route lies inside them, so they are not vacuous, and
  the shares are printed;
* inputs on which every float32 partial sum is exact: the restatement equals `fold_stem` in bytes, fragments included;
* four wrong variants of the restatement are rejected by these same comparisons;
* the bf16 helper against torch: ties to even, overflow to infinity, infinities, float32 denormals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import publish_ref as PR
import train_gpu_harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def env():
    e = H.load_env(("az_net", "optim"))
    from src import fast_net, publish
    e["FN"], e["PB"] = fast_net, publish
    return e


@pytest.fixture(scope="module")
def seeded(env):
    """The seeded 3-block module with its heads' outputs and the stem's bias off zero -> (state dict as numpy, the twin on
    the CPU)."""
    torch = env["torch"]
    net = H.module(env, torch.float32, "cpu", stem_bias=True)
    sd = net.state_dict()
    return {k: v.numpy().copy() for k, v in sd.items()}, env["FN"].FastConnect4Net(sd, "cpu")


def memory(env, t):
    """A twin buffer's bytes in memory order: uint16 for bf16, float32 as it is."""
    torch = env["torch"]
    if t.dim() == 4 and not t.is_contiguous():      # a channels_last OIHW weight: its memory is [o][ky][kx][c]
        assert t.is_contiguous(memory_format=torch.channels_last)
        t = t.permute(0, 2, 3, 1)
    t = t.contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def test_the_restatement_is_the_twin(env, seeded):
    sd, twin = seeded
    ref = PR.layout(sd)
    assert PR.n_blocks_of(sd) == 3 and sd["hidden.0.bias"].any() and sd["policy_head.out.weight"].any()
    buffers = dict(twin.named_buffers())
    checked = 0
    for name, want in ref.items():
        if name in ("stem_frag", "stem_pmap", "scalars"):
            continue
        got = memory(env, buffers[name])
        assert got.dtype == np.uint16 and got.size == want.size, name
        assert np.array_equal(got.reshape(-1), want.reshape(-1)), name
        checked += 1
    assert checked == 5 + 4 * 3 + 5 + 15
    # every buffer of the twin is covered: what is left are the folded stem's two and the three float32 biases
    assert set(buffers) - set(ref) == {"p_gate_b", "p_out_b", "d_aux_b"}
    assert ref["scalars"].tobytes() == np.concatenate([buffers[n].numpy() for n in ("p_gate_b", "p_out_b", "d_aux_b")]).tobytes()
    assert ref["stem_frag"].shape == tuple(buffers["stem_frag"].shape) and ref["stem_pmap"].shape == tuple(buffers["stem_pmap"].shape)
    # the order the ABI compares in is the twin's memory order, not the logical one
    assert not np.array_equal(memory(env, buffers["stem_w"]).reshape(-1), PR.bf16_bits(sd["hidden.0.weight"]).reshape(-1))


def fold_errors(sd, frag, pmap):
    """(the largest share of the T bound, of the pmap bound) a folded stem uses, after the structural zeros are checked."""
    t64, s, p64, sp = PR.fold_float64(sd)
    hi, lo = PR.unfragment(np.asarray(frag).reshape(2, 4, 64, 8))
    assert not hi[:, 18:].any() and not lo[:, 18:].any()
    pmap = np.asarray(pmap, np.float32).reshape(48, 68)
    assert not pmap[42:].view(np.uint32).any() and not pmap[:, 64:].view(np.uint32).any()
    t = PR.bf16_float(hi)[:, :18].astype(np.float64) + PR.bf16_float(lo)[:, :18].astype(np.float64)
    share_t = np.abs(t - t64) / (34 * U * s + 2.0 ** -17 * np.abs(t64))
    share_p = np.abs(pmap[:42, :64].astype(np.float64) - p64) / (290 * U * sp)
    return float(share_t.max()), float(share_p.max())


def test_the_folded_stem_is_within_derived_bounds_of_float64(env, seeded):
    sd, twin = seeded
    ref = PR.layout(sd)
    mine = fold_errors(sd, ref["stem_frag"], ref["stem_pmap"])
    theirs = fold_errors(sd, memory(env, twin.stem_frag), twin.stem_pmap.numpy())
    print("share of the bounds (T, pmap): restatement %.3f %.4f   fold_stem %.3f %.4f" % (mine + theirs))
    assert mine[0] <= 1.0 and mine[1] <= 1.0
    assert theirs[0] <= 1.0 and theirs[1] <= 1.0


def exact_state(sd, seed=5):
    """W and bias k / 128 with |k| <= 127, embeddings k / 16 with |k| <= 15: every product has at most 11 significant bits
    below 2^4 and every partial sum of at most 289 of them fits float32 exactly."""
    rng = np.random.default_rng(seed)
    out = dict(sd)
    out["hidden.0.weight"] = (rng.integers(-127, 128, (64, 32, 3, 3)) / 128.0).astype(np.float32)
    out["hidden.0.bias"] = (rng.integers(-127, 128, 64) / 128.0).astype(np.float32)
    out["piece_emb.weight"] = (rng.integers(-15, 16, (2, 32)) / 16.0).astype(np.float32)
    out["pos_emb.weight"] = (rng.integers(-15, 16, (24, 32)) / 16.0).astype(np.float32)
    return out


def test_exact_inputs_give_fold_stems_bytes(env, seeded):
    torch, FN = env["torch"], env["FN"]
    sd = exact_state(seeded[0])
    frag, pmap = PR.fold(sd)
    tt = {k: torch.from_numpy(sd[k]) for k in ("hidden.0.weight", "hidden.0.bias", "piece_emb.weight", "pos_emb.weight")}
    f2, p2 = FN.fold_stem(tt["hidden.0.weight"], tt["hidden.0.bias"], tt["piece_emb.weight"][0], tt["piece_emb.weight"][1],
                          tt["pos_emb.weight"][torch.from_numpy(PR.ORBIT)])
    assert memory(env, f2).tobytes() == frag.tobytes()
    assert p2.numpy().tobytes() == pmap.tobytes()
    # and both are float64's values: nothing was rounded on the way
    t64, _, p64, _ = PR.fold_float64(sd)
    hi, lo = PR.unfragment(frag)
    assert np.array_equal(PR.bf16_float(hi)[:, :18].astype(np.float64) + PR.bf16_float(lo)[:, :18].astype(np.float64), t64)
    assert np.array_equal(pmap[:42, :64].astype(np.float64), p64)


def test_wrong_variants_are_rejected(seeded):
    sd = seeded[0]
    right = PR.fold(sd)
    assert max(fold_errors(sd, *right)) <= 1.0
    # own and opponent planes swapped: the T comparison fails, pmap does not depend on the planes
    frag, pmap = PR.fold(sd, swap_planes=True)
    share = fold_errors(sd, frag, pmap)
    assert share[0] > 1.0 and share[1] <= 1.0 and frag.tobytes() != right[0].tobytes()
    # W left unrounded in the fold: both comparisons fail (2^-9 per weight against 2^-19 of S)
    share = fold_errors(sd, *PR.fold(sd, round_w=False))
    assert share[0] > 1.0 and share[1] > 1.0
    # a tap outside the board counted: pmap fails at the border cells, T is untouched
    frag, pmap = PR.fold(sd, outside=True)
    assert fold_errors(sd, frag, pmap)[1] > 1.0 and frag.tobytes() == right[0].tobytes()
    inner = [7 * y + x for y in range(1, 5) for x in range(1, 6)]
    assert pmap[inner].tobytes() == right[1][inner].tobytes()
    # the bias added before the sum instead of after: only rounding differs, so the float64 bound cannot see it - the
    # byte comparison, which is what the kernel is held to, does
    frag, pmap = PR.fold(sd, bias_first=True)
    assert pmap.tobytes() != right[1].tobytes() and frag.tobytes() == right[0].tobytes()
    # ... and on exact inputs no order can matter: there the two agree
    ex = exact_state(sd)
    assert PR.fold(ex, bias_first=True)[1].tobytes() == PR.fold(ex)[1].tobytes()


def test_bf16_helper_is_torchs(env):
    torch = env["torch"]
    bits = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000,      # ties: down to even, up to even, just above, just below
                     0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0x7F7F7FFF,                              # the largest finite values: to infinity or not
                     0x7F800000, 0xFF800000, 0x00000000, 0x80000000,                              # infinities and zeros
                     0x00000001, 0x007FFFFF, 0x00008000, 0x00018000, 0x807F8000, 0x00800000], np.uint32)    # denormals, the smallest normal
    rng = np.random.default_rng(3)
    bits = np.concatenate([bits, rng.integers(0, 2 ** 32, 1 << 16, dtype=np.uint64).astype(np.uint32)])
    x = bits.view(np.float32)
    x = x[~np.isnan(x)]
    want = torch.from_numpy(x.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    got = PR.bf16_bits(x)
    assert np.array_equal(got, want)
    first = PR.bf16_bits(bits[:12].view(np.float32)).tolist()
    assert first == [0x3F80, 0x3F82, 0x3F81, 0x3F80, 0xBF80, 0xBF82, 0x7F80, 0xFF80, 0x7F80, 0x7F7F, 0x7F80, 0xFF80]
    assert np.array_equal(PR.bf16_round(x).view(np.uint32), want.astype(np.uint32) << 16)


def test_the_mirror_has_the_compilers_layout(env, tmp_path):
    PB, abi = env["PB"], env["abi"]
    assert set(PB.MIRRORS) == {"az_nn_publish_src"} and PB.MAX_BLOCKS == abi.MAX_BLOCKS
    mirror = PB.PublishSrcC
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "az_nn.h"', '#include "az_train.h"', "int main() {",
             '    printf("sizeof %zu %d\\n", sizeof(az_nn_publish_src), (int)AZ_NN_PUBLISH_SRC_BYTES);',
             '    printf("define %d %d\\n", (int)AZ_NN_MAX_BLOCKS, (int)(AZ_LEARN_ROLE_HEADS - AZ_LEARN_ROLE_ATTN));']
    for field in mirror._fields_:
        lines.append('    printf("%s %%zu %%zu\\n", offsetof(az_nn_publish_src, %s), sizeof(((az_nn_publish_src *)0)->%s));'
                     % (field[0], field[0], field[0]))
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["g++", "-std=c++17", "-I", INC, str(src), "-o", str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        name, *numbers = ln.split()
        got[name] = tuple(int(n) for n in numbers)
    assert got.pop("sizeof") == (C.sizeof(mirror), C.sizeof(mirror)) == (488, 488)
    assert got.pop("define") == (PB.MAX_BLOCKS, len(PB.ATTN))
    want = {f[0]: (getattr(mirror, f[0]).offset, getattr(mirror, f[0]).size) for f in mirror._fields_}
    assert got == want and len(want) == 4 + 1 + 4 + 6 + 18
    # the fields that follow the blocks are the learner's roles in order: az_learn_publish fills them by index
    assert [f[0] for f in mirror._fields_[9:]] == [n for n, _, _ in PB.ATTN + PB.HEADS]
    assert [n for n, _, _ in PB.HEADS] == list(abi.TrainHeadsParamsC._NAMES) and [n for n, _, _ in PB.ATTN] == [f[0] for f in abi.TrainAttnParamsC._fields_]


def test_importing_publish_does_not_import_the_engine(env):
    import sys
    code = ("import sys; sys.path.insert(0, %r); import src.publish; "
            "print(sorted(m for m in ('src.MCTS_cpp', 'src.mcts_cpp', 'src.selfplay', 'src.match', 'src.learner', 'src.fused') if m in sys.modules))" % H.PKG)
    out = subprocess.run([sys.executable, "-c", code], check=True, capture_output=True, text=True).stdout
    assert out.strip() == "[]"
