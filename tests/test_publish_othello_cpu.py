"""Publishing Othello weights without a GPU: the numpy restatement of the Othello evaluator's layout function
(tests/publish_othello_ref.py, what tests/test_publish_othello_gpu.py holds k_publish_othello to byte for byte) against the
inference twin built on the CPU, and the layout of the struct src/publish.py mirrors.

* every array of `FastOthelloNet(net)` on the CPU that is a cast, a permutation or one float32 add - the packed convolution
  weights, the bottleneck's, the embedding table, board_w, v_conv_w, a_fc_wt, a_fc_w16 - equals the restatement in bytes;
* the BatchNorm affines agree with `fast_othello._bn_affine` within DERIVED bounds, not in bytes (torch's float32 sqrt is
  not correctly rounded everywhere; numpy's is).  With u = 2^-24:
      |scale - scale_t| <= 4 u |scale|                      one ulp (2 u) of the root, then one rounding (u) of the division
                                                            on each side
      |shift - shift_t| <= 8 u (|mean * scale| + |shift|)   the product inherits the scale's 4 u and is rounded on each side
                                                            (6 u of |mean * scale|), the subtraction is rounded on each side
  and the restatement is within 3 u |scale| of a float64 evaluation (the sum's rounding u reaches the root as u / 2, the
  root's own rounding adds u, the division's u: 2.5 u to first order; the shares are printed);
* five wrong variants of the restatement are rejected by these same comparisons;
* the struct mirrors have the compiler's layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import publish_othello_ref as POR
import train_gpu_harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
U = 2.0 ** -24


@pytest.fixture(scope="module")
def env():
    e = H.load_env(("az_net",))
    from src import fast_othello, publish
    e["FO"], e["PB"] = fast_othello, publish
    return e


def randomise(torch, net, seed):
    """Every parameter off its initial value (the zeroed output layers too) and every BatchNorm with running statistics,
    gammas of both signs and betas of its own."""
    gen = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_((torch.randn(p.shape, generator=gen) * 0.05).to(p.device))
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                n = m.num_features
                m.weight.copy_((1.0 + 0.5 * torch.randn(n, generator=gen)).to(m.weight.device))
                m.bias.copy_((0.3 * torch.randn(n, generator=gen)).to(m.bias.device))
                m.running_mean.copy_((0.5 * torch.randn(n, generator=gen)).to(m.weight.device))
                m.running_var.copy_((0.25 + 3.0 * torch.rand(n, generator=gen)).to(m.weight.device))
    return net


def numpy_sd(net):
    return {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def bits(t):
    """A twin array's bytes: uint16 for bf16, float32 as it is."""
    import torch
    t = t.detach().contiguous()
    return t.view(torch.int16).cpu().numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.cpu().numpy()


@pytest.fixture(scope="module")
def seeded(env):
    """A one-block module with randomised BatchNorm state -> (module, state dict as numpy, its twin on the CPU, eps)"""
    torch = env["torch"]
    torch.manual_seed(5)
    net = randomise(torch, env["NET"].OthelloNet(num_res_blocks=1, device="cpu"), 6)
    return net, numpy_sd(net), env["FO"].FastOthelloNet(net), float(net.stem[1].eps)


def test_the_restatement_is_the_twin_in_bytes(env, seeded):
    torch = env["torch"]
    net, sd, twin, eps = seeded
    ref = POR.layout(sd, eps)
    assert POR.n_blocks_of(sd) == 1 and twin.n_body == 4 and len(twin.layers) == 6
    assert POR.ORBIT.tolist() == net.orbit_map.tolist() == env["PB"].othello_orbit_map()
    for i, layer in enumerate(twin.layers):
        assert np.array_equal(bits(layer[0]).reshape(-1), ref["conv%d_w" % i].reshape(-1)), i
        assert ("conv%d_pre_scale" % i in ref) == (layer[1] is not None)
        assert ("conv%d_post_scale" % i in ref) == (layer[2][0] is not twin.layers[1][2][0])      # the shared ones / zeros: no BatchNorm behind
    assert [tuple(layer[4:]) for layer in twin.layers] == [(32, 8, 2), (256, 10, 1), (256, 10, 1), (256, 10, 1), (256, 10, 0), (256, 8, 1)]
    assert np.array_equal(bits(twin.dual_w).reshape(-1), ref["dual_w16"].reshape(-1))
    assert np.array_equal(bits(twin.embed_table), ref["embed_table"])
    assert np.array_equal(bits(twin.board_w), ref["board_w"])
    assert bits(twin.v_conv_w).tobytes() == ref["v_conv_w"].tobytes()
    # what native_model() makes of the 512 x 512 weight (the object is host memory: it needs no GPU)
    assert twin.native_model() is not None
    keep = twin.__dict__["_model_keep"]
    assert bits(keep["a_fc_w16"]).tobytes() == ref["a_fc_w16"].tobytes()
    w = net.dual_head.aux_out[1].weight.detach()
    assert bits(w.t()).tobytes() == ref["a_fc_wt"].tobytes()
    assert any(v.shape == (512, 512) and v.dtype == torch.float32 and bits(v).tobytes() == ref["a_fc_wt"].tobytes() for v in keep.values())
    assert bits(w.reshape(512, 8, 64).transpose(1, 2).reshape(512, 512).to(torch.bfloat16)).tobytes() == ref["a_fc_w16"].tobytes()
    for name, key in POR.COPIES:
        assert ref[name].tobytes() == sd[key].tobytes()
    assert ref["scalars"].tolist() == [twin.board_b, float(net.policy_head.pass_fc.bias.detach()), float(net.dual_head.aux_out[5].bias.detach())]
    assert not ref["dual_w16"][:, :, :, [16 * g + tl for g in range(4) for tl in range(8, 16)], :].any()       # rows 8 .. 15 of the padded weight
    assert ref["dual_scale16"][8:].tolist() == [1.0] * 8 and ref["dual_shift16"][8:].view(np.uint32).tolist() == [0] * 8


def affines(env, seeded):
    """[(name, the four BatchNorm tensors, the twin's (scale, shift) as numpy)] of all eight BatchNorms of the module"""
    net, sd, twin, _ = seeded
    FO = env["FO"]
    out = []
    for i, (_, pre, post) in enumerate(POR.conv_names(1)):
        if pre is not None:
            out.append(("conv%d pre" % i, POR.norm_of(sd, pre), tuple(bits(t) for t in twin.layers[i][1])))
        if post is not None:
            out.append(("conv%d post" % i, POR.norm_of(sd, post), tuple(bits(t) for t in twin.layers[i][2])))
    out.append(("dual", POR.norm_of(sd, "dual_head.stem.1"), (bits(twin.dual_s)[:8], bits(twin.dual_b)[:8])))
    out.append(("v", POR.norm_of(sd, "dual_head.value_out.1"), tuple(bits(t).reshape(-1) for t in FO._bn_affine(net.dual_head.value_out[1]))))
    assert np.array_equal(out[-1][2][0], bits(twin.v_bn[0]).reshape(-1))
    return out


def test_batchnorm_affines_are_within_derived_bounds(env, seeded):
    eps = seeded[3]
    all_of = affines(env, seeded)
    assert len(all_of) == 8
    worst = [0.0, 0.0, 0.0]
    for name, norm, (scale_t, shift_t) in all_of:
        scale, shift = POR.bn_affine(*norm, eps)
        s64, _ = POR.bn_affine64(*norm, eps)
        mean = norm[2].astype(np.float64)
        d = scale.astype(np.float64)
        share = (np.abs(d - scale_t) / (4 * U * np.abs(d)), np.abs(shift.astype(np.float64) - shift_t) / (8 * U * (np.abs(mean * d) + np.abs(shift))),
                 np.abs(d - s64) / (3 * U * np.abs(d)))
        worst = [max(a, float(b.max())) for a, b in zip(worst, share)]
        print("%-10s share of the bounds: scale %.3f  shift %.3f  float64 %.3f" % ((name,) + tuple(float(s.max()) for s in share)))
        assert all(s.max() <= 1.0 for s in share), name
    assert worst[2] > 0.05          # the bounds are of the errors' order, not vacuous


def test_wrong_variants_are_rejected(env, seeded):
    net, sd, twin, eps = seeded
    ref = POR.layout(sd, eps)
    # kinds 2 and 3 swapped: legal_emb[0] under "legal"
    wrong = POR.embed_table(sd, swap_kinds=True)
    assert not np.array_equal(wrong, bits(twin.embed_table)) and np.array_equal(wrong[0::4], ref["embed_table"][0::4])
    assert np.array_equal(wrong[2::4], ref["embed_table"][3::4])
    # g and tl swapped in the lane index
    for i in (0, 1):
        wrong = POR.pack_conv(sd[POR.conv_names(1)[i][0]], swap_lane=True)
        assert wrong.shape == ref["conv%d_w" % i].shape and not np.array_equal(wrong.reshape(-1), bits(twin.layers[i][0]).reshape(-1))
        assert np.array_equal(np.sort(wrong.reshape(-1)), np.sort(ref["conv%d_w" % i].reshape(-1)))      # the same values, elsewhere
    norm = POR.norm_of(sd, "stem.1")
    right = POR.bn_affine(*norm, eps)
    s64, _ = POR.bn_affine64(*norm, eps)
    # eps added after the root: the float64 bound sees it (eps / sqrt(var) of the scale against 3 u)
    wrong = POR.bn_affine(*norm, eps, eps_after_root=True)
    assert (np.abs(wrong[0].astype(np.float64) - s64) > 3 * U * np.abs(s64)).any()
    assert (np.abs(right[0].astype(np.float64) - s64) <= 3 * U * np.abs(s64)).all()
    # the shift from the unrounded scale: only a rounding differs, so no bound can see it - the byte comparison, which is
    # what the kernel is held to, does
    wrong = POR.bn_affine(*norm, eps, unrounded_scale=True)
    assert wrong[0].tobytes() == right[0].tobytes() and wrong[1].tobytes() != right[1].tobytes()
    # a_fc_w16 in channel-major order
    wrong = POR.a_fc_w16(sd["dual_head.aux_out.1.weight"], channel_major=True)
    assert twin.native_model() is not None
    assert wrong.tobytes() != bits(twin.__dict__["_model_keep"]["a_fc_w16"]).tobytes()


def test_the_mirrors_have_the_compilers_layout(env, tmp_path):
    PB, abi = env["PB"], env["abi"]
    assert set(PB.OTHELLO_MIRRORS) == {"az_nn_othello_bn_src", "az_nn_othello_publish_src"} and set(PB.MIRRORS) == {"az_nn_publish_src"}
    assert len(abi.MIRRORS) == 17
    lines = ["#include <cstddef>", "#include <cstdio>", '#include "az_nn.h"', "int main() {",
             '    printf("define %d %d\\n", (int)AZ_NN_OTHELLO_MAX_CONVS, (int)AZ_NN_OTHELLO_PUBLISH_SRC_BYTES);']
    for struct, mirror in PB.OTHELLO_MIRRORS.items():
        lines.append('    printf("%s sizeof %%zu\\n", sizeof(%s));' % (struct, struct))
        for field in mirror._fields_:
            lines.append('    printf("%s %s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s *)0)->%s));' % (struct, field[0], struct, field[0], struct, field[0]))
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["g++", "-std=c++17", "-I", INC, str(src), "-o", str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        struct, field, *numbers = ln.split()
        got[struct, field] = tuple(int(n) for n in numbers)
    assert got.pop(("define", str(PB.OTHELLO_MAX_CONVS))) == (C.sizeof(PB.OthelloPublishSrcC),) == (1368,)
    want = {}
    for struct, mirror in PB.OTHELLO_MIRRORS.items():
        want[struct, "sizeof"] = (C.sizeof(mirror),)
        for field in mirror._fields_:
            d = getattr(mirror, field[0])
            want[struct, field[0]] = (d.offset, d.size)
    assert got == want and len(PB.OthelloPublishSrcC._fields_) == 3 + 3 + 3 + 2 + 6 + 1 + 7
    # the C compiler's assertion too
    c = tmp_path / "layout.c"
    c.write_text('#include "az_nn.h"\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-I", INC, str(c), "-o", str(tmp_path / "layout_c")], check=True)
    # the state dict names the source struct is filled from exist in the module, with the shapes it checks
    sd = env["NET"].OthelloNet(num_res_blocks=1, device="cpu").state_dict()
    for _, name, shape in PB.O_TENSORS:
        assert tuple(sd[name].shape) == shape, name
    for weight, pre, post, c_in in PB.othello_conv_names(1):
        assert tuple(sd[weight].shape) == (256, c_in, 3, 3)
        for prefix in (pre, post):
            assert prefix is None or all("%s.%s" % (prefix, k) in sd for _, k in PB.BN_FIELDS)
    assert [(w, a, b) for w, a, b, _ in PB.othello_conv_names(3)] == POR.conv_names(3)
