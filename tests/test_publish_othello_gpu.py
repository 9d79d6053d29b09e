"""Publishing trained Othello weights into a live evaluator (az_nn_othello_publish_dev, az_nn_model_publish_othello,
src/publish.py `publish_othello`) on the GPU, against the numpy restatement tests/publish_othello_ref.py - which
tests/test_publish_othello_cpu.py holds to the inference twin and to float64 - byte for byte:

* the one launch through ctypes: sources in a slab at offsets that are 4- but not 16-byte aligned, destinations as fill
  pattern between guard regions, the post arrays of layers without a BatchNorm behind them as fill pattern too, 1 and 3
  blocks, with and without a_fc_w16, twice.  The inputs: variances in [2^-6, 4] and an exact 0, negative and zero gammas,
  weights on bf16 ties both ways, infinities, float32 denormals; every float32 intermediate of an affine is normal or zero;
* a copy whose destination is its source is skipped, a partially overlapping one refused; every refusal leaves the slab
  untouched;
* the live model: the same handle over the same addresses computes, in bytes, what a NEW model over buffers uploaded from
  the restatement computes; the biases; a capturing stream and a Connect4 model are refused;
* `publish_othello(fast)` against a fresh `FastOthelloNet(net)`: every buffer in bytes, the BatchNorm affines within the
  bound tests/test_publish_othello_cpu.py derives, `forward` within othello_ref.HEADS_FLOOR (what
  tests/test_othello_kernels_gpu.py holds the evaluator's two heads kernels to against each other);
* `FusedSearch.publish_weights()` for Othello; what the Python entry point refuses.

Where a forward is needed it is 16 positions: both sides to move, the four symmetry ids the engine uses."""
import ctypes as C
import math

import numpy as np
import pytest

import othello_ref as R
import publish_othello_ref as POR
import scenarios as S
import train_gpu_harness as H
from test_publish_othello_cpu import U, bits, numpy_sd, randomise
from train_gpu_harness import AZ_ERR_ARG, FILL, Slab

pytestmark = pytest.mark.gpu

BATCH = 16
EPS = 1e-5
SPECIAL = np.array([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x3F808001, 0x3F807FFF,        # ties down and up to even, both signs, just off a tie
                    0x7F800000, 0xFF800000, 0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF,                    # infinities, the largest finite values
                    0x00000001, 0x007FFFFF, 0x00018000, 0x807F8000, 0x00800000], np.uint32).view(np.float32)      # denormals, the smallest normal


@pytest.fixture(scope="module")
def env():
    e = H.load_env(("az_net",))
    from src import MCTS_cpp, fast_net, fast_othello, fused, publish
    e.update(FO=fast_othello, FN=fast_net, PB=publish, W=MCTS_cpp, F=fused)
    return e


def make_net(env, n_blocks, seed, device="cuda"):
    torch = env["torch"]
    torch.manual_seed(seed)
    return randomise(torch, env["NET"].OthelloNet(num_res_blocks=n_blocks, device="cpu"), seed + 1000).to(device).eval()


def perturb(env, net, seed, keep_biases=False):
    """Seeded noise on every parameter and on every BatchNorm's running statistics, in place (`keep_biases`: not on the
    three biases that travel by value)."""
    torch = env["torch"]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if not (keep_biases and name in POR.SCALARS):
                p.add_((torch.randn(p.shape, generator=gen) * 0.03).to(p.device))
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.add_((torch.randn(m.num_features, generator=gen) * 0.05).to(m.weight.device))
                m.running_var.mul_((0.8 + 0.4 * torch.rand(m.num_features, generator=gen)).to(m.weight.device))


def special_sd(env, n_blocks, seed):
    """A module's state dict as numpy with the inputs the byte test is about (the module's docstring)."""
    sd = numpy_sd(make_net(env, n_blocks, seed, "cpu"))
    rng = np.random.default_rng(seed)
    for key in [k for k in sd if k.endswith("running_var")]:
        prefix = key[:-len("running_var")]
        n = sd[key].size
        var = np.exp2(rng.uniform(-6.0, 2.0, n)).astype(np.float32)
        var[0], var[1], var[2] = 0.0, 2.0 ** -6, 4.0
        gamma = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.uniform(0.05, 2.0, n)).astype(np.float32)
        gamma[1], gamma[3] = 0.0, -0.75
        mean = (np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.uniform(1e-3, 1.0, n)).astype(np.float32)
        mean[4] = 0.0
        sd[key], sd[prefix + "weight"], sd[prefix + "running_mean"] = var, gamma, mean
        # every intermediate normal or zero: flushing denormals is not part of the contract
        a = (var + np.float32(EPS)).astype(np.float32)
        scale, shift = POR.bn_affine(gamma, sd[prefix + "bias"], mean, var, EPS)
        for x in (a, np.sqrt(a), scale, (mean * scale).astype(np.float32), shift):
            assert np.isfinite(x).all() and ((np.abs(x) >= np.finfo(np.float32).tiny) | (x == 0)).all(), key
    for key in ("stem.0.weight", "stem.3.conv1.weight", "dual_head.stem.0.weight", "policy_head.board_out.weight", "dual_head.aux_out.1.weight",
                "policy_head.pass_norm.weight", "dual_head.value_out.0.weight"):
        flat = sd[key].reshape(-1)
        at = rng.choice(flat.size, SPECIAL.size, replace=False)
        flat[at] = SPECIAL
        flat[:2] = SPECIAL[:2]
    # the embedding's one add on a tie: 1 + 2^-8 rounds down to even, 1 + 3 * 2^-8 up
    sd["pos_emb.weight"][0, 0], sd["piece_emb.weight"][0, 0], sd["piece_emb.weight"][1, 0] = 1.0, 2.0 ** -8, 3 * 2.0 ** -8
    table = POR.embed_table(sd)
    assert table[0, 0] == 0x3F80 and table[1, 0] == 0x3F82
    return sd


def geometry(n_blocks):
    """(c_in, h_in, pad, residual) of every convolution, in the order of az_nn_othello_weights.conv"""
    return [(32, 8, 2, 0)] + [(256, 10, 1, 0), (256, 10, 1, 1)] * n_blocks + [(256, 10, 1, 0), (256, 10, 0, 0), (256, 8, 1, 0)]


def source_keys(PB, n_blocks):
    keys = [name for _, name, _ in PB.O_TENSORS]
    for weight, pre, post, _ in PB.othello_conv_names(n_blocks):
        keys.append(weight)
        keys += ["%s.%s" % (p, k) for p in (pre, post) if p is not None for _, k in PB.BN_FIELDS]
    return keys + ["%s.%s" % (p, k) for _, p, _ in PB.O_NORMS for _, k in PB.BN_FIELDS]


def source_struct(PB, n_blocks, eps, at):
    """az_nn_othello_publish_src over `at(state dict key)`"""
    src = PB.OthelloPublishSrcC()
    src.n_body, src.n_convs, src.bn_eps = 2 * n_blocks + 2, 2 * n_blocks + 4, eps

    def norm(into, prefix):
        for field, k in PB.BN_FIELDS:
            setattr(into, field, at("%s.%s" % (prefix, k)))
    for field, name, _ in PB.O_TENSORS:
        setattr(src, field, at(name))
    for i, (weight, pre, post, _) in enumerate(PB.othello_conv_names(n_blocks)):
        src.conv_weight[i] = at(weight)
        if pre is not None:
            norm(src.conv_pre[i], pre)
        if post is not None:
            norm(src.conv_post[i], post)
    for field, prefix, _ in PB.O_NORMS:
        norm(getattr(src, field), prefix)
    return src


def weights_struct(env, n_blocks, w16, at, biases=(0.0, 0.0, 0.0)):
    """az_nn_othello_weights over `at(name in publish_othello_ref.layout)`; `at` gives None for what is not there"""
    abi = env["abi"]
    w = abi._OthelloW()
    w.embed_table, w.n_body, w.n_convs = at("embed_table"), 2 * n_blocks + 2, 2 * n_blocks + 4
    for i, (c_in, h_in, pad, res) in enumerate(geometry(n_blocks)):
        layer = w.conv[i]
        layer.w_packed = at("conv%d_w" % i)
        layer.pre_scale, layer.pre_shift = at("conv%d_pre_scale" % i), at("conv%d_pre_shift" % i)
        layer.post_scale, layer.post_shift = at("conv%d_post_scale" % i), at("conv%d_post_shift" % i)
        layer.residual, layer.c_in, layer.h_in, layer.pad = res, c_in, h_in, pad
    w.dual_w16, w.dual_scale16, w.dual_shift16 = at("dual_w16"), at("dual_scale16"), at("dual_shift16")
    for name in abi._HeadsW._PTRS:
        setattr(w.heads, name, at(name))
    w.heads.a_fc_w16 = at("a_fc_w16") if w16 else None
    w.heads.board_b, w.heads.pass_fc_b, w.heads.a_out_b = biases
    w.heads.aux_to_score, w.heads.eps = 8.0, 1e-5
    return w


class Call:
    """One az_nn_othello_publish_dev call laid out in a slab: every source behind 1 to 3 floats of padding (4- but not
    16-byte aligned), every destination, the post arrays of layers without a BatchNorm behind them and the 16-byte scalar
    slot as fill pattern."""

    def __init__(self, env, sd, w16, eps=EPS):
        torch, PB = env["torch"], env["PB"]
        self.n_blocks = POR.n_blocks_of(sd)
        self.ref = POR.layout(sd, eps, w16)
        inputs, self.shift = {}, {}
        for i, key in enumerate(source_keys(PB, self.n_blocks)):
            pad = (1, 3, 2)[i % 3]
            inputs[key] = np.concatenate([np.full(pad, 7.0, np.float32), np.asarray(sd[key], np.float32).ravel()])
            self.shift[key] = 4 * pad
        self.written = [n for n in self.ref if n != "scalars"]
        outs = {n: self.ref[n].nbytes for n in self.written}
        self.unwritten = [n for i in range(2 * self.n_blocks + 4) for n in ("conv%d_post_scale" % i, "conv%d_post_shift" % i) if n not in outs]
        outs.update({n: 1024 for n in self.unwritten})
        outs["scalars"] = 16
        self.slab = Slab(torch, inputs, outs)
        assert all(self.slab.ptr(k, s) % 16 in (4, 8, 12) for k, s in self.shift.items())
        self.src = source_struct(PB, self.n_blocks, eps, lambda key: self.slab.ptr(key, self.shift[key]))
        self.dst = weights_struct(env, self.n_blocks, w16, self.slab.ptr)
        self.scalars = self.slab.ptr("scalars")

    def image(self, env):
        env["torch"].cuda.synchronize()
        return self.slab.dev.cpu().numpy()

    def untouched(self, env):
        return np.array_equal(self.image(env), self.slab.host)

    def problems(self, image, skip=()):
        """Every destination that is not the restatement's bytes, and anything written outside them."""
        slab, out = self.slab, []
        for name in self.written:
            if name not in skip and image[slab.at[name]:slab.at[name] + slab.size[name]].tobytes() != self.ref[name].tobytes():
                out.append(name)
        at = slab.at["scalars"]
        if image[at:at + 12].tobytes() != self.ref["scalars"].tobytes() or not (image[at + 12:at + 16] == FILL).all():
            out.append("scalars")
        if not slab.untouched_outside(image, [n for n in self.written if n not in skip] + ["scalars"]):
            out.append("outside the destinations")
        return out


def stream(env):
    return C.c_void_p(env["torch"].cuda.current_stream().cuda_stream)


def clone(struct):
    return type(struct).from_buffer_copy(struct)


# ---------------------------------------------------------------------------------------- 1. the launch in bytes

@pytest.mark.parametrize("w16", (True, False))
@pytest.mark.parametrize("n_blocks", (1, 3))
def test_one_launch_writes_the_restatements_bytes(env, n_blocks, w16):
    L = env["L"]
    call = Call(env, special_sd(env, n_blocks, 200 + n_blocks), w16)
    assert len(call.unwritten) == 2 * 2 * n_blocks and ("a_fc_w16" in call.written) == w16
    images = []
    for _ in range(2):
        assert L.az_nn_othello_publish_dev(C.byref(call.src), C.byref(call.dst), call.scalars, stream(env)) == 0
        images.append(call.image(env))
    assert call.problems(images[0]) == []
    assert np.array_equal(images[1], images[0])


def test_aliased_copies(env):
    L = env["L"]
    call = Call(env, special_sd(env, 1, 210), True)
    # the destination IS the source: no job, everything else as ever
    dst = clone(call.dst)
    dst.heads.pass_norm_w, dst.heads.a_fc_b = call.src.pass_norm_weight, call.src.a_fc_bias
    assert L.az_nn_othello_publish_dev(C.byref(call.src), C.byref(dst), call.scalars, stream(env)) == 0
    assert call.problems(call.image(env), skip=("pass_norm_w", "a_fc_b")) == []
    call.slab.upload()
    # any other overlap of the two ranges
    for field, source, shift in (("a_norm_w", "a_norm_weight", 4), ("a_norm_w", "a_norm_weight", -4), ("v_fc_b", "v_fc_bias", 8),
                                 ("pass_fc_w", "pass_fc_weight", 1020)):
        dst = clone(call.dst)
        setattr(dst.heads, field, getattr(call.src, source) + shift)
        assert L.az_nn_othello_publish_dev(C.byref(call.src), C.byref(dst), call.scalars, stream(env)) == AZ_ERR_ARG, (field, shift)
    assert call.untouched(env)


# ---------------------------------------------------------------------------------------- 2. the live model

@pytest.fixture(scope="module")
def positions(env):
    """16 positions on the device -> (az_nn_positions, the mask tensor, the tensors that keep them alive, planes, bool masks)"""
    torch = env["torch"]
    boards, turns = S.ot_openings(np.random.default_rng(31), BATCH, 40, 0)
    turns[::3] *= -1
    syms = np.array([0, 2, 6, 7], np.int32)[np.arange(BATCH) % 4]
    masks = np.zeros((BATCH, 65), np.uint8)
    for i in range(BATCH):                                                        # the mask is in the shown frame
        mv = S.ot_moves(np.ascontiguousarray(R.SYMMETRIES[int(syms[i])](boards[i])), int(turns[i]))
        masks[i, mv if mv else [64]] = 1
    assert (turns > 0).any() and (turns < 0).any()
    bb1, bb2 = S.ot_bitboards(boards)
    dev = [torch.from_numpy(bb1.view(np.int64)).cuda(), torch.from_numpy(bb2.view(np.int64)).cuda(), torch.from_numpy(turns.astype(np.int32)).cuda(),
           torch.from_numpy(syms).cuda(), torch.from_numpy(masks).cuda()]
    # the same boards as feature planes for the twin's torch route (unsymmetrised; its mask in that frame)
    planes = np.stack([(boards == turns[:, None, None]), (boards == -turns[:, None, None]), np.ones_like(boards) * turns[:, None, None]], 1).astype(np.float32)
    plain = np.zeros((BATCH, 65), bool)
    for i in range(BATCH):
        mv = S.ot_moves(boards[i], int(turns[i]))
        plain[i, mv if mv else [64]] = True
    return env["abi"].Positions(*[t.data_ptr() for t in dev[:4]]), dev[4], dev, torch.from_numpy(planes).cuda(), torch.from_numpy(plain).cuda()


def forward(env, model, positions):
    """(probs, wdl, utility) of the 16 positions from an az_nn_model, as uint32"""
    torch, L = env["torch"], env["L"]
    nb = int(L.az_nn_model_scratch_bytes(model, BATCH))
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    outs = [torch.full(shape, float("nan"), device="cuda") for shape in ((BATCH, 65), (BATCH, 3), (BATCH,))]
    assert L.az_nn_model_forward_positions(model, C.byref(positions[0]), positions[1].data_ptr(), *[t.data_ptr() for t in outs], BATCH, None, None,
                                           scratch.data_ptr(), nb, stream(env)) == 0
    torch.cuda.synchronize()
    res = [t.cpu().numpy() for t in outs]
    assert all(np.isfinite(r).all() for r in res)
    return [r.view(np.uint32) for r in res]


def twin_arrays(fast):
    """name in publish_othello_ref.layout -> the tensor of a twin (and of its native model) that holds it"""
    model = fast.native_model()
    assert model is not None
    keep = fast.__dict__["_model_keep"]
    out = {"embed_table": fast.embed_table, "dual_w16": fast.dual_w, "dual_scale16": fast.dual_s, "dual_shift16": fast.dual_b, "board_w": fast.board_w,
           "v_conv_w": fast.v_conv_w, "v_bn_s": fast.v_bn[0], "v_bn_b": fast.v_bn[1], "a_fc_w16": keep["a_fc_w16"]}
    out["a_fc_wt"] = [v for k, v in keep.items() if k != "a_fc_w16" and tuple(v.shape) == (512, 512)][0]
    sd = fast.net.state_dict()
    for name, key in POR.COPIES:                 # the model reads these straight from the module's parameters
        out[name] = sd[key]
        assert getattr(fast._model_w.heads, name) == sd[key].data_ptr(), name
    for i, (wp, pre, post, *_) in enumerate(fast.layers):
        out["conv%d_w" % i] = wp
        if pre is not None:
            out["conv%d_pre_scale" % i], out["conv%d_pre_shift" % i] = pre
        out["conv%d_post_scale" % i], out["conv%d_post_shift" % i] = post
    return out


AFFINE = ("scale", "shift", "scale16", "shift16", "v_bn_s", "v_bn_b")


def against_ref(fast, ref):
    """The arrays of a twin that differ from publish_othello_ref.layout in bytes."""
    got = twin_arrays(fast)
    return [name for name, want in ref.items() if name != "scalars" and bits(got[name]).tobytes() != want.tobytes()]


def test_the_live_model_computes_the_new_weights(env, positions):
    torch, L, abi = env["torch"], env["L"], env["abi"]
    net = make_net(env, 3, 30)
    fast = env["FO"].FastOthelloNet(net)
    handle = fast.native_model()
    before = forward(env, handle, positions)
    addresses = {n: t.data_ptr() for n, t in twin_arrays(fast).items()}
    perturb(env, net, 77)
    biases = fast.publish_from()
    after = forward(env, handle, positions)
    # a new model over buffers uploaded from the restatement, with the published biases
    sd = numpy_sd(net)
    ref = POR.layout(sd, EPS)
    up = {n: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for n, v in ref.items()}
    ones, zeros = torch.ones(256, device="cuda"), torch.zeros(256, device="cuda")

    def at(name):
        if name in up:
            return up[name].data_ptr()
        return ones.data_ptr() if name.endswith("post_scale") else zeros.data_ptr() if name.endswith("post_shift") else None
    w = weights_struct(env, 3, True, at, biases)
    other = C.c_void_p()
    assert L.az_nn_model_create_othello(C.byref(w), C.byref(other)) == 0
    try:
        want = forward(env, other, positions)
    finally:
        L.az_nn_model_destroy(other)
    for x, y in zip(after, want):
        assert np.array_equal(x, y)
    assert not np.array_equal(after[0], before[0]) and not np.array_equal(after[1], before[1])
    assert {n: t.data_ptr() for n, t in twin_arrays(fast).items()} == addresses
    assert fast.native_model() is handle and against_ref(fast, ref) == []
    out = (C.c_float * 3)()
    assert L.az_nn_model_othello_head_biases(handle, C.byref(out)) == 0
    module = np.array([sd[k].reshape(-1)[0] for k in POR.SCALARS], np.float32)
    assert np.array(list(out), np.float32).tobytes() == module.tobytes() == np.array(biases, np.float32).tobytes()
    hw = fast._model_w.heads
    assert np.array([hw.board_b, hw.pass_fc_b, hw.a_out_b, fast.board_b], np.float32).tobytes() == module.tobytes() + module[:1].tobytes()
    assert hw.aux_to_score == 8.0 and math.isclose(hw.eps, 1e-5, rel_tol=1e-6)
    # setting and reading the biases back on the host
    assert L.az_nn_model_set_othello_head_biases(handle, 0.5, -0.25, 2.0) == 0 and L.az_nn_model_othello_head_biases(handle, C.byref(out)) == 0
    assert list(out) == [0.5, -0.25, 2.0]
    assert L.az_nn_model_set_othello_head_biases(handle, *biases) == 0
    # a capturing stream is refused (the call waits), and so is a model of another kind, by every entry point
    src, _keep = env["PB"].othello_source_struct(fast)
    slot = fast.publish_slot
    image = {n: bits(t).tobytes() for n, t in twin_arrays(fast).items()}
    graph, dummy = torch.cuda.CUDAGraph(), torch.zeros(8, device="cuda")
    with torch.cuda.graph(graph):
        dummy.add_(1.0)
        refused = L.az_nn_model_publish_othello(handle, C.byref(src), slot.data_ptr(), stream(env))
    assert refused == AZ_ERR_ARG
    connect4 = env["FN"].FastConnect4Net.from_module(env["NET"].Connect4Net(device="cuda"))
    c4 = connect4.native_model()
    hash_model = C.c_void_p()
    assert L.az_nn_model_create_hash(1, C.byref(hash_model)) == 0
    try:
        cases = {"connect4 model": L.az_nn_model_publish_othello(c4, C.byref(src), slot.data_ptr(), stream(env)),
                 "hash model": L.az_nn_model_publish_othello(hash_model, C.byref(src), slot.data_ptr(), stream(env)),
                 "null model": L.az_nn_model_publish_othello(None, C.byref(src), slot.data_ptr(), stream(env)),
                 "connect4 model's othello biases": L.az_nn_model_othello_head_biases(c4, C.byref(out)),
                 "connect4 model's othello biases set": L.az_nn_model_set_othello_head_biases(c4, 0.0, 0.0, 0.0),
                 "othello model's connect4 biases": L.az_nn_model_head_biases(handle, C.byref(out)),
                 "othello model's connect4 biases set": L.az_nn_model_set_head_biases(handle, 0.0, 0.0, 0.0),
                 # az_nn_model_publish keeps refusing Othello models
                 "othello model, connect4 publish": L.az_nn_model_publish(handle, C.byref(env["PB"].PublishSrcC()), slot.data_ptr(), stream(env)),
                 "null source struct": L.az_nn_model_publish_othello(handle, None, slot.data_ptr(), stream(env)),
                 "null scalars": L.az_nn_model_publish_othello(handle, C.byref(src), None, stream(env))}
    finally:
        L.az_nn_model_destroy(hash_model)
    assert {k: v for k, v in cases.items() if v != AZ_ERR_ARG} == {}
    torch.cuda.synchronize()
    assert {n: bits(t).tobytes() for n, t in twin_arrays(fast).items()} == image


# ---------------------------------------------------------------------------------------- 3. against a fresh twin

def test_publish_equals_a_fresh_twin(env, positions):
    torch, FO = env["torch"], env["FO"]
    net = make_net(env, 3, 40)
    fast = FO.FastOthelloNet(net)
    perturb(env, net, 41)
    biases = env["PB"].publish_othello(fast, net)
    fresh = FO.FastOthelloNet(net)
    a, b = twin_arrays(fast), twin_arrays(fresh)
    assert list(a) == list(b)
    sd = numpy_sd(net)
    for name in a:
        x, y = bits(a[name]).reshape(-1), bits(b[name]).reshape(-1)
        if not name.endswith(AFFINE):
            assert x.tobytes() == y.tobytes(), name
        elif name.endswith(("scale", "scale16", "v_bn_s")):
            # the bound of tests/test_publish_othello_cpu.py: |scale - scale_t| <= 4 u |scale|, |shift - shift_t| <= 8 u (|mean * scale| + |shift|)
            shift_name = name.replace("scale", "shift") if "scale" in name else "v_bn_b"
            sx, sy = bits(a[shift_name]).reshape(-1), bits(b[shift_name]).reshape(-1)
            if fast.layers[1][2][0] is a[name]:
                assert x.tobytes() == y.tobytes() and sx.tobytes() == sy.tobytes(), name          # the shared ones / zeros
                continue
            prefix = {"dual_scale16": "dual_head.stem.1", "v_bn_s": "dual_head.value_out.1"}.get(name)
            if prefix is None:
                i, which = int(name[4:name.index("_")]), name.split("_")[1]
                prefix = POR.conv_names(3)[i][1 if which == "pre" else 2]
            n = sd[prefix + ".running_mean"].size
            mean = sd[prefix + ".running_mean"].astype(np.float64)
            d, s = x[:n].astype(np.float64), sx[:n].astype(np.float64)
            share = (np.abs(d - y[:n]) / (4 * U * np.abs(d))).max(), (np.abs(s - sy[:n]) / (8 * U * (np.abs(mean * d) + np.abs(s)))).max()
            print("%-18s share of the bounds against the fresh twin: scale %.3f  shift %.3f" % (name, share[0], share[1]))
            assert share[0] <= 1.0 and share[1] <= 1.0, name
            assert x[n:].tobytes() == y[n:].tobytes() and sx[n:].tobytes() == sy[n:].tobytes()
    assert fast.board_b == fresh.board_b == biases[0]
    hw, fw = fast._model_w.heads, fresh._model_w.heads
    assert (hw.board_b, hw.pass_fc_b, hw.a_out_b) == (fw.board_b, fw.pass_fc_b, fw.a_out_b) == biases
    assert against_ref(fast, POR.layout(sd, EPS)) == []
    # the torch route: the evaluator's existing tolerance between two routes to the same outputs
    x, mask = positions[3], positions[4]
    got, want = fast.predict_device(x, mask), fresh.predict_device(x, mask)
    torch.cuda.synchronize()
    errs = [float((g.double() - w.double()).abs().max()) for g, w in zip(got, want)]
    print("published twin against a fresh one, forward: probs %.3g  wdl %.3g  utility %.3g  (allowed %.3g)" % (*errs, R.HEADS_FLOOR))
    assert all(torch.isfinite(g).all() for g in got) and got[0].std().item() > 1e-4
    assert all(e <= R.HEADS_FLOOR for e in errs)


# ---------------------------------------------------------------------------------------- 4. FusedSearch.publish_weights

def test_fused_search_publishes_in_place(env):
    W = env["W"]
    net = make_net(env, 3, 51)
    boards, turns = S.ot_openings(np.random.default_rng(9), 8, 30, 0)

    def wrapper():
        w = W.BatchedMCTS(8, 1.4, 800, 0.0, 16, noise_epsilon=0.0, fpu_reduction=0.2, use_symmetry=False, game_name="Othello",
                          score_utility_factor=0.15, score_scale=8.0)
        w.seed(7)
        return w, w._fused_runner(net, True)

    def result(w):
        return w.get_visits_count().copy()

    wa, fa = wrapper()
    assert fa.fast is None and fa.publish_weights() == "rebuilt" and fa.fast is not None       # a wrapper without a twin
    wa.batch_playout(net, boards, turns, vl_batch=4, fused=True)                                # W0
    old = result(wa)
    fa._graphs["marker"] = None                                     # whatever was captured, and one entry in any case
    fast, model, graphs, runs = fa.fast, fa.fast.native_model(), dict(fa._graphs), dict(fa._eager_runs)
    print("graphs captured at W0: %d, shapes run eagerly: %d" % (len(graphs) - 1, len(runs)))
    perturb(env, net, 78, keep_biases=True)                                                     # W1: the three biases as they were
    assert fa.publish_weights() == "published"
    assert fa.fast is fast and fast.native_model() is model
    assert fa._graphs == graphs and fa._eager_runs == runs and len(runs) > 0                    # the biases did not change in bits: all kept
    del fa._graphs["marker"]
    version = fa._fast_version
    fa._sync_fast_net()
    assert fa.fast is fast and fa._fast_version == version                                      # no rebuild
    wb, fb = wrapper()
    fb._sync_fast_net()                                                                         # built fresh at W1
    assert fb.publish_weights() == "published" and fb.fast is not fast
    ref = POR.layout(numpy_sd(net), EPS)
    assert against_ref(fast, ref) == [] and against_ref(fb.fast, ref) == []                     # torch's sqrt is out of the comparison
    for i in range(8):
        wa.mcts.reset_env(i)
    wa.seed(7)
    wa.batch_playout(net, boards, turns, vl_batch=4, fused=True)
    wb.batch_playout(net, boards, turns, vl_batch=4, fused=True)
    a, b = result(wa), result(wb)
    assert (a.sum(1) == 15).all() and np.array_equal(a, b)
    assert not np.array_equal(a, old)                                                           # and the new weights are what searched
    # a changed bias drops the graphs and the eager runs
    with env["torch"].no_grad():
        net.policy_head.pass_fc.bias.add_(0.125)
    fa._graphs["marker"] = None
    assert fa.publish_weights() == "published" and fa._graphs == {} and fa._eager_runs == {}


# ---------------------------------------------------------------------------------------- 5. argument errors

def test_argument_errors_write_nothing(env):
    L, PB = env["L"], env["PB"]
    call = Call(env, special_sd(env, 1, 61), True)
    src, dst, sc, s = call.src, call.dst, call.scalars, stream(env)
    dev = lambda a, b, c: L.az_nn_othello_publish_dev(None if a is None else C.byref(a), None if b is None else C.byref(b), c, s)   # noqa: E731

    def changed(struct, path, value):
        """A copy of `struct` with one field set; `path` like "heads.a_fc_wt", "conv.1.w_packed", "conv_post.0.mean"; a
        callable value is given the old one."""
        out = clone(struct)
        target, names = out, path.split(".")
        for name in names[:-1]:
            target = target[int(name)] if name.isdigit() else getattr(target, name)
        old = target[int(names[-1])] if names[-1].isdigit() else getattr(target, names[-1])
        new = value(old) if callable(value) else value
        if names[-1].isdigit():
            target[int(names[-1])] = new
        else:
            setattr(target, names[-1], new)
        return out

    def both(path, value):
        return dev(changed(src, path, value), changed(dst, path, value), sc)

    plus = lambda k: (lambda old: old + k)      # noqa: E731
    pre0 = clone(src)
    for field, _ in PB.BN_FIELDS:               # a BatchNorm in front of the stem, which the destination has none for
        setattr(pre0.conv_pre[0], field, getattr(src.conv_post[0], field))
    cases = {
        "null src": dev(None, dst, sc), "null dst": dev(src, None, sc), "null scalars": dev(src, dst, None),
        "null source": dev(changed(src, "pos_emb", None), dst, sc), "null conv source": dev(changed(src, "conv_weight.2", None), dst, sc),
        "null last source": dev(changed(src, "a_out_bias", None), dst, sc), "null bias source": dev(changed(src, "pass_fc_bias", None), dst, sc),
        "null embed_table": dev(src, changed(dst, "embed_table", None), sc), "null w_packed": dev(src, changed(dst, "conv.1.w_packed", None), sc),
        "null a_fc_wt": dev(src, changed(dst, "heads.a_fc_wt", None), sc), "null dual_scale16": dev(src, changed(dst, "dual_scale16", None), sc),
        "null copy destination": dev(src, changed(dst, "heads.v_fc_b", None), sc), "null v_bn_b": dev(src, changed(dst, "heads.v_bn_b", None), sc),
        "null post_shift under a BatchNorm": dev(src, changed(dst, "conv.0.post_shift", None), sc),
        "n_body 0": both("n_body", 0), "n_body 3": both("n_body", 3), "n_body 16": dev(changed(changed(src, "n_body", 16), "n_convs", 18), changed(changed(dst, "n_body", 16), "n_convs", 18), sc),
        "n_convs not n_body + 2": both("n_convs", 5), "n_body differs": dev(changed(changed(src, "n_body", 2), "n_convs", 4), dst, sc),
        "n_body differs the other way": dev(src, changed(changed(dst, "n_body", 2), "n_convs", 4), sc),
        "c_in 64": dev(src, changed(dst, "conv.1.c_in", 64), sc), "h_in 9": dev(src, changed(dst, "conv.1.h_in", 9), sc),
        "pad 3": dev(src, changed(dst, "conv.0.pad", 3), sc), "the stem's geometry on a 256-channel layer": dev(src, changed(dst, "conv.1.pad", 2), sc),
        "eps nan": dev(changed(src, "bn_eps", float("nan")), dst, sc), "eps inf": dev(changed(src, "bn_eps", float("inf")), dst, sc),
        "eps negative": dev(changed(src, "bn_eps", -1e-5), dst, sc),
        "a BatchNorm without its mean": dev(changed(src, "conv_post.0.mean", None), dst, sc),
        "a BatchNorm with only its var": dev(changed(changed(changed(src, "conv_pre.1.weight", None), "conv_pre.1.bias", None), "conv_pre.1.mean", None), dst, sc),
        "the bottleneck's BatchNorm without its weight": dev(changed(src, "dual_bn.weight", None), dst, sc),
        "pre_scale without conv_pre": dev(changed(changed(changed(changed(src, "conv_pre.1.weight", None), "conv_pre.1.bias", None), "conv_pre.1.mean", None), "conv_pre.1.var", None), dst, sc),
        "conv_pre without pre_scale": dev(pre0, dst, sc), "pre_scale without pre_shift": dev(src, changed(dst, "conv.1.pre_shift", None), sc),
        "conv_pre, neither pre_scale nor pre_shift": dev(src, changed(changed(dst, "conv.1.pre_shift", None), "conv.1.pre_scale", None), sc),
        "w_packed at 8 bytes": dev(src, changed(dst, "conv.0.w_packed", plus(8)), sc), "dual_w16 at 8 bytes": dev(src, changed(dst, "dual_w16", plus(8)), sc),
        "embed_table at 8 bytes": dev(src, changed(dst, "embed_table", plus(8)), sc), "a_fc_w16 at 2 bytes": dev(src, changed(dst, "heads.a_fc_w16", plus(2)), sc),
        "a_fc_wt at 4 bytes": dev(src, changed(dst, "heads.a_fc_wt", plus(4)), sc), "board_w at 1 byte": dev(src, changed(dst, "heads.board_w", plus(1)), sc),
        "v_bn_s at 2 bytes": dev(src, changed(dst, "heads.v_bn_s", plus(2)), sc), "post_scale at 2 bytes": dev(src, changed(dst, "conv.0.post_scale", plus(2)), sc),
        "copy destination at 2 bytes": dev(src, changed(dst, "heads.a_out_w", plus(2)), sc), "v_conv_w at 2 bytes": dev(src, changed(dst, "heads.v_conv_w", plus(2)), sc),
        "source at 2 bytes": dev(changed(src, "conv_weight.0", plus(2)), dst, sc), "embedding source at 2 bytes": dev(changed(src, "legal_emb", plus(2)), dst, sc),
        "BatchNorm source at 2 bytes": dev(changed(src, "conv_post.0.mean", plus(2)), dst, sc), "bias source at 2 bytes": dev(changed(src, "a_out_bias", plus(2)), dst, sc),
        "scalars at 2 bytes": dev(src, dst, sc + 2),
    }
    assert {k: v for k, v in cases.items() if v != AZ_ERR_ARG} == {}
    assert call.untouched(env)
    # and the same structs, unchanged, are accepted through the model entry point: the refusals above were the changes'
    model = C.c_void_p()
    assert L.az_nn_model_create_othello(C.byref(dst), C.byref(model)) == 0
    try:
        assert L.az_nn_model_publish_othello(model, C.byref(changed(src, "n_body", 6)), sc, s) == AZ_ERR_ARG and call.untouched(env)
        assert L.az_nn_model_publish_othello(model, C.byref(src), sc, s) == 0
        assert call.problems(call.image(env)) == []
        out = (C.c_float * 3)()
        assert L.az_nn_model_othello_head_biases(model, C.byref(out)) == 0
        assert np.array(list(out), np.float32).tobytes() == call.ref["scalars"].tobytes()
    finally:
        L.az_nn_model_destroy(model)


def test_what_the_python_entry_point_refuses(env):
    torch, PB, FO = env["torch"], env["PB"], env["FO"]
    net = make_net(env, 1, 62)
    fast = FO.FastOthelloNet(net)
    image = {n: bits(t).tobytes() for n, t in twin_arrays(fast).items()}
    with pytest.raises(ValueError, match="load_state_dict"):                    # a foreign module
        PB.publish_othello(fast, make_net(env, 1, 63))
    with pytest.raises(ValueError, match="needs a FastOthelloNet"):
        PB.publish_othello(net)

    def refused(match, change, restore):
        change()
        try:
            with pytest.raises(ValueError, match=match):
                fast.publish_from()
        finally:
            restore()

    ph, dh = net.policy_head, net.dual_head
    w = dh.aux_out[1].weight
    data = w.data
    # a wrong shape, a non-contiguous tensor, another dtype: each names the tensor
    refused(r"dual_head\.aux_out\.1\.weight has shape", lambda: setattr(w, "data", data[:, :256].contiguous()), lambda: setattr(w, "data", data))
    refused(r"dual_head\.aux_out\.1\.weight must be a contiguous", lambda: setattr(w, "data", data.t()), lambda: setattr(w, "data", data))
    norm_w = ph.pass_norm.weight.data           # put back as the same storage: the native model aliases it
    refused(r"policy_head\.pass_norm\.weight must be a contiguous float32", lambda: setattr(ph.pass_norm.weight, "data", norm_w.double()),
            lambda: setattr(ph.pass_norm.weight, "data", norm_w))
    var = net.stem[1].running_var
    refused(r"stem\.1\.running_var must be a contiguous float32 CUDA", lambda: setattr(net.stem[1], "running_var", var.cpu()),
            lambda: setattr(net.stem[1], "running_var", var))
    # mixed BatchNorm eps
    refused(r"policy_head\.stem\.5 has eps", lambda: setattr(ph.stem[5], "eps", 1e-3), lambda: setattr(ph.stem[5], "eps", EPS))
    # another orbit map
    orbit = net.orbit_map.clone()
    refused("orbit_map", lambda: net.orbit_map.__setitem__(5, 3), lambda: net.orbit_map.copy_(orbit))
    # another depth: a twin of one block whose module grew
    other = FO.FastOthelloNet(make_net(env, 1, 64))
    other.net = make_net(env, 3, 65)
    with pytest.raises(ValueError, match="residual blocks"):
        other.publish_from()
    torch.cuda.synchronize()
    assert {n: bits(t).tobytes() for n, t in twin_arrays(fast).items()} == image and fast.publish_from() is not None
