"""Publishing trained Connect4 weights into a live evaluator (az_nn_publish_dev, az_nn_model_publish, az_learn_publish,
src/publish.py) on the GPU, against the numpy restatement tests/publish_ref.py - which tests/test_publish_cpu.py holds to
the inference twin and to float64 - byte for byte:

* the one launch through ctypes: sources in a slab, some only 4-byte aligned, destinations between guard regions, with
  and without the folded stem, 1, 3 and 8 blocks, twice;
* exact inputs: publishing into an existing twin gives the buffers and the forward of a fresh `from_module`;
* the live model: the same handle over the same addresses computes the new weights' outputs;
* a learner publishes what it trained; `FusedSearch.publish_weights`; every argument error leaves the slab untouched.

Where a forward is needed it is 64 positions: both sides to move, both symmetry ids, at least one full column."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import learner_harness as LH
import publish_ref as PR
import scenarios as S
import train_gpu_harness as H
from test_oracle_golden import bits
from test_publish_cpu import exact_state
from train_gpu_harness import AZ_ERR_ARG, FILL, Slab

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(H.ROOT, "tools"))
import record_conv_golden as R  # noqa: E402

BATCH = 64
BIAS_KEYS = PR.SCALARS


@pytest.fixture(scope="module")
def env():
    e = LH.load_env()
    from src import MCTS_cpp, fast_net, fused, publish
    e.update(FN=fast_net, PB=publish, W=MCTS_cpp, F=fused)
    return e


def make_net(env, n_blocks, seed, device="cuda"):
    """A seeded Connect4 module with every tensor off its initial value (norm weights off one, biases and the heads'
    zeroed outputs off zero)."""
    torch = env["torch"]
    torch.manual_seed(seed)
    net = env["NET"].Connect4Net(num_res_blocks=n_blocks, device="cpu")
    with torch.no_grad():
        for p in net.parameters():
            p.add_(torch.randn_like(p) * 0.05)
    return net.to(device).eval()


def perturb(env, net, seed):
    """Seeded noise on every parameter, in place."""
    torch = env["torch"]
    gen = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for p in net.parameters():
            p.add_((torch.randn(p.shape, generator=gen) * 0.03).to(p.device))


def numpy_sd(net):
    return {k: v.detach().cpu().numpy().copy() for k, v in net.state_dict().items()}


def source_fields(PB, n_blocks):
    """[(field of az_nn_publish_src, block index or None, state dict key)]"""
    out = [(f, None, key) for f, key, _ in PB.STEM]
    for k in range(n_blocks):
        out += [(f, k, "hidden.%d.%s" % (k + 2, key)) for f, key, _ in PB.BLOCK]
    out += [(f, None, "hidden.%d.attn.%s" % (n_blocks + 2, key)) for f, key, _ in PB.ATTN]
    return out + [(f, None, key) for f, key, _ in PB.HEADS]


def dest_fields(n_blocks, folded):
    """[(name in publish_ref.layout, how to set it on a ModelWeights)]"""
    out = [(n, (n, None)) for n in ("emb_own", "emb_opp", "pos", "stem_w", "stem_b", "pre_w", "qkvg_w", "qn_w", "kn_w", "o_w")]
    for k in range(n_blocks):
        out += [("res%d_%s" % (k + 2, s), (f, k)) for s, f in (("w", "block_w"), ("b", "block_b"), ("g", "block_gamma"), ("beta", "block_beta"))]
    out += [(n, ("heads." + n, None)) for n, _ in PR.HEADS]
    if folded:
        out += [("stem_frag", ("stem_frag", None)), ("stem_pmap", ("stem_pmap", None))]
    return out


def weights_struct(env, n_blocks, folded, address, biases=(0.0, 0.0, 0.0)):
    w = env["abi"].ModelWeights()
    for name, (field, k) in dest_fields(n_blocks, folded):
        if k is not None:
            getattr(w, field)[k] = address(name)
        elif field.startswith("heads."):
            setattr(w.heads, field[6:], address(name))
        else:
            setattr(w, field, address(name))
    w.n_blocks, w.eps = n_blocks, 1e-5
    w.heads.p_gate_b, w.heads.p_out_b, w.heads.d_aux_b = biases
    w.heads.aux_scale = 42.0
    return w


class Call:
    """One az_nn_publish_dev call laid out in a slab: every source (every second one behind 1 to 3 floats of padding, so
    that it is 4-byte but not 16-byte aligned), every destination and the 16-byte scalar slot as fill pattern."""

    def __init__(self, env, sd, folded):
        torch, PB = env["torch"], env["PB"]
        self.n_blocks = PR.n_blocks_of(sd)
        self.ref = PR.layout(sd, folded)
        self.fields = source_fields(PB, self.n_blocks)
        inputs, self.shift = {}, {}
        for i, (_, _, key) in enumerate(self.fields):
            pad = (1, 0, 3, 0, 2, 0)[i % 6]
            inputs[key] = np.concatenate([np.full(pad, 7.0, np.float32), sd[key].astype(np.float32).ravel()])
            self.shift[key] = 4 * pad
        self.written = [n for n, _ in dest_fields(self.n_blocks, folded)]
        outs = {n: self.ref[n].nbytes for n in self.written}
        outs["scalars"] = 16
        self.slab = Slab(torch, inputs, outs)
        assert any((self.slab.ptr(k, s) % 16) == 4 for k, s in self.shift.items()) and all(self.slab.ptr(k, s) % 4 == 0 for k, s in self.shift.items())
        self.src = PB.PublishSrcC()
        self.src.n_blocks = self.n_blocks
        for field, k, key in self.fields:
            p = self.slab.ptr(key, self.shift[key])
            if k is None:
                setattr(self.src, field, p)
            else:
                getattr(self.src, field)[k] = p
        self.dst = weights_struct(env, self.n_blocks, folded, self.slab.ptr)
        self.scalars = self.slab.ptr("scalars")

    def image(self, env):
        env["torch"].cuda.synchronize()
        return self.slab.dev.cpu().numpy()

    def untouched(self, env):
        return np.array_equal(self.image(env), self.slab.host)


def stream(env):
    return C.c_void_p(env["torch"].cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------- 1. the launch in bytes

@pytest.mark.parametrize("folded", (True, False))
@pytest.mark.parametrize("n_blocks", (1, 3, 8))
def test_one_launch_writes_the_restatements_bytes(env, n_blocks, folded):
    L = env["L"]
    call = Call(env, numpy_sd(make_net(env, n_blocks, 100 + n_blocks, "cpu")), folded)
    images = []
    for _ in range(2):
        assert L.az_nn_publish_dev(C.byref(call.src), C.byref(call.dst), call.scalars, stream(env)) == 0
        images.append(call.image(env))
    image, slab = images[0], call.slab
    for name in call.written:
        got = image[slab.at[name]:slab.at[name] + slab.size[name]]
        assert got.tobytes() == call.ref[name].tobytes(), name
    at = slab.at["scalars"]
    assert image[at:at + 12].tobytes() == call.ref["scalars"].tobytes()
    assert (image[at + 12:at + 16] == FILL).all()                   # the slot's fourth float is not written
    assert slab.untouched_outside(image, call.written + ["scalars"])          # guards, sources, their padding
    assert np.array_equal(images[1], image)


# ---------------------------------------------------------------------------------------- 2. forwards

@pytest.fixture(scope="module")
def positions(env):
    """64 positions on the device -> (az_nn_positions, the tensors that keep them alive)"""
    torch = env["torch"]
    p1, p2, turn, sym, _ = R.positions(np.random.default_rng(4242), BATCH)
    both = p1 | p2
    assert (turn > 0).any() and (turn < 0).any() and (sym == 0).any() and (sym == 1).any()
    assert any(((int(b) >> (7 * c)) & 0x3F) == 0x3F for b in both for c in range(7)), "no full column"
    dev = [torch.from_numpy(p1.view(np.int64)).cuda(), torch.from_numpy(p2.view(np.int64)).cuda(), torch.from_numpy(turn).cuda(),
           torch.from_numpy(sym).cuda()]
    return env["abi"].Positions(*[t.data_ptr() for t in dev]), dev


def forward(env, model, positions):
    """(probs, wdl, moves_left) of the 64 positions from an az_nn_model, as uint32"""
    torch, L = env["torch"], env["L"]
    mask = torch.ones((BATCH, 7), dtype=torch.uint8, device="cuda")
    nb = int(L.az_nn_model_scratch_bytes(model, BATCH))
    scratch = torch.empty(nb, dtype=torch.uint8, device="cuda")
    outs = [torch.full(shape, float("nan"), device="cuda") for shape in ((BATCH, 7), (BATCH, 3), (BATCH,))]
    assert L.az_nn_model_forward_positions(model, C.byref(positions[0]), mask.data_ptr(), *[t.data_ptr() for t in outs], BATCH, None, None,
                                           scratch.data_ptr(), nb, stream(env)) == 0
    torch.cuda.synchronize()
    res = [t.cpu().numpy() for t in outs]
    assert all(np.isfinite(r).all() for r in res)
    return [r.view(np.uint32) for r in res]


def buffer_bytes(fast):
    """name -> the bytes of every buffer of a twin, in memory order"""
    import torch
    out = {}
    for name, t in fast.named_buffers():
        if t.dim() == 4 and not t.is_contiguous():          # a channels_last OIHW weight: its memory is [o][ky][kx][c]
            t = t.permute(0, 2, 3, 1)
        out[name] = t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()
    return out


def against_ref(fast, ref):
    """The first buffer of a twin that differs from publish_ref.layout, or None."""
    got = buffer_bytes(fast)
    for name, want in ref.items():
        if name != "scalars" and got[name] != want.tobytes():
            return name
    if b"".join(got[n] for n in ("p_gate_b", "p_out_b", "d_aux_b")) != ref["scalars"].tobytes():
        return "scalars"
    return None


def test_exact_inputs_equal_a_fresh_twin(env, positions):
    torch, FN = env["torch"], env["FN"]
    fast = FN.FastConnect4Net.from_module(make_net(env, 3, 21))          # an existing twin, of other weights
    net = make_net(env, 3, 22)
    ex = exact_state({})
    with torch.no_grad():
        for key in ("hidden.0.weight", "hidden.0.bias", "piece_emb.weight", "pos_emb.weight"):
            dict(net.named_parameters())[key].copy_(torch.from_numpy(ex[key]))
    keys = list(fast.state_dict())
    fast.publish_from(net)
    fresh = FN.FastConnect4Net.from_module(net)
    a, b = buffer_bytes(fast), buffer_bytes(fresh)
    assert list(a) == list(b) == keys == list(fast.state_dict())        # the slot is no buffer
    for name in a:
        assert a[name] == b[name], name
    assert fast._heads_w.p_gate_b == fresh._heads_w.p_gate_b and fast._heads_w.p_out_b == fresh._heads_w.p_out_b
    assert fast._heads_w.d_aux_b == fresh._heads_w.d_aux_b and fast.p_gate_b_host == fresh.p_gate_b_host
    for x, y in zip(forward(env, fast.native_model(), positions), forward(env, fresh.native_model(), positions)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("n_blocks", (1, 3, 8))
def test_the_live_model_computes_the_new_weights(env, positions, n_blocks):
    torch, L, FN = env["torch"], env["L"], env["FN"]
    net = make_net(env, n_blocks, 30 + n_blocks)
    fast = FN.FastConnect4Net.from_module(net)
    handle = fast.native_model()
    before = forward(env, handle, positions)
    addresses = {n: t.data_ptr() for n, t in fast.named_buffers()}
    perturb(env, net, 77)
    biases = fast.publish_from(net)
    after = forward(env, handle, positions)
    # a new model over buffers uploaded from the restatement, with the published biases
    sd = numpy_sd(net)
    ref = PR.layout(sd)
    up = {n: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for n, v in ref.items()}
    w = weights_struct(env, n_blocks, True, lambda n: up[n].data_ptr(), biases)
    other = C.c_void_p()
    assert L.az_nn_model_create(C.byref(w), C.byref(other)) == 0
    try:
        want = forward(env, other, positions)
    finally:
        L.az_nn_model_destroy(other)
    for x, y in zip(after, want):
        assert np.array_equal(x, y)
    assert not np.array_equal(after[0], before[0]) and not np.array_equal(after[1], before[1])
    assert {n: t.data_ptr() for n, t in fast.named_buffers()} == addresses
    assert fast.native_model() is handle and against_ref(fast, ref) is None
    out = (C.c_float * 3)()
    assert L.az_nn_model_head_biases(handle, C.byref(out)) == 0
    module = np.array([sd[k].reshape(-1)[0] for k in BIAS_KEYS], np.float32)
    assert np.array(list(out), np.float32).tobytes() == module.tobytes() == np.array(biases, np.float32).tobytes()
    hw = fast._heads_w
    assert np.array([hw.p_gate_b, hw.p_out_b, hw.d_aux_b, fast.p_gate_b_host], np.float32).tobytes() == module.tobytes() + module[:1].tobytes()
    assert hw.aux_scale == 42.0
    # setting and reading the biases back on the host
    assert L.az_nn_model_set_head_biases(handle, 0.5, -0.25, 2.0) == 0 and L.az_nn_model_head_biases(handle, C.byref(out)) == 0
    assert list(out) == [0.5, -0.25, 2.0]
    assert L.az_nn_model_set_head_biases(handle, *biases) == 0


# ---------------------------------------------------------------------------------------- 3. the learner

def test_a_learner_publishes_what_it_trained(env):
    torch, L, LN, FN = env["torch"], env["L"], env["LN"], env["FN"]
    net = LH.module(env)
    fast = FN.FastConnect4Net.from_module(net)
    learner = LN.NativeLearner(net, 64)
    config = env["TL"].LossConfig(**LH.KNOBS)
    before = numpy_sd(net)
    for batch in H.loaders(env)["cuda"][:2]:
        learner.step(batch, config)
    biases = learner.publish(fast)
    sd = numpy_sd(net)
    assert any(sd[k].tobytes() != before[k].tobytes() for k in BIAS_KEYS) and sd["hidden.0.weight"].tobytes() != before["hidden.0.weight"].tobytes()
    assert against_ref(fast, PR.layout(sd)) is None
    assert np.array(biases, np.float32).tobytes() == PR.layout(sd)["scalars"].tobytes()
    # before az_learn_bind
    cfg = LN.LearnConfigC(64, 3, 0, 1e-5, 1e-5, 1e-5, 5.0, 0.0, 0.0, 0.0, 0.0, 0)
    raw = C.c_void_p()
    assert L.az_learn_create(C.byref(cfg), C.byref(raw)) == 0
    try:
        image = buffer_bytes(fast)
        assert L.az_learn_publish(raw, fast.native_model(), fast.publish_slot.data_ptr(), stream(env)) == AZ_ERR_ARG
        assert b"az_learn_bind" in L.az_last_error()
        torch.cuda.synchronize()
        assert buffer_bytes(fast) == image
    finally:
        L.az_learn_destroy(raw)
    learner.close()


# ---------------------------------------------------------------------------------------- 4. FusedSearch.publish_weights

def test_fused_search_publishes_in_place(env):
    W = env["W"]
    net = make_net(env, 3, 51)
    rng = np.random.default_rng(9)
    B = 128
    boards, turns = S.random_openings(rng, B, 9)
    boards[:32] = boards[0]; turns[:32] = turns[0]              # transpositions across trees: the table gets hits

    def wrapper():
        w = W.BatchedMCTS(B, 1.4, 400, 0.0, 24, noise_epsilon=0.0, fpu_reduction=0.2, use_symmetry=False, mlh_slope=0.1)
        w.seed(7)
        return w, w._fused_runner(net, True)

    def result(w):
        return w.get_visits_count().copy(), np.array(w.mcts.get_all_root_stats()).copy()

    w1, fs1 = wrapper()
    fs1.enable_table(14)
    w1.batch_playout(net, boards, turns, vl_batch=4, fused=True)            # the old weights: fills the table
    old = result(w1)
    w2, fs2 = wrapper()
    fs2._sync_fast_net()                                                    # a twin of the old weights, no table
    fast1, fast2 = fs1.fast, fs2.fast
    model1 = fast1.native_model()
    assert fs1.table_stats()["inserts"] > 0
    refreshed = []
    original = fs1.refresh_table
    fs1.refresh_table = lambda: (refreshed.append(1), original())[1]
    perturb(env, net, 78)
    assert fs1.publish_weights() == "published" and fs2.publish_weights() == "published"
    assert fs1.fast is fast1 and fast1.native_model() is model1 and refreshed == [1]
    version = fs1._fast_version
    fs1._sync_fast_net()
    assert fs1.fast is fast1 and fs1._fast_version == version               # no rebuild
    assert against_ref(fast1, PR.layout(numpy_sd(net))) is None and against_ref(fast2, PR.layout(numpy_sd(net))) is None
    for i in range(B):
        w1.mcts.reset_env(i)
    w1.batch_playout(net, boards, turns, vl_batch=4, fused=True)
    w2.batch_playout(net, boards, turns, vl_batch=4, fused=True)
    assert fs1.fast is fast1 and fs2.fast is fast2
    (c1, s1), (c2, s2) = result(w1), result(w2)
    assert np.array_equal(c1, c2) and np.array_equal(bits(s1), bits(s2))
    assert not np.array_equal(bits(s1), bits(old[1]))                       # and the new weights are what searched
    # a wrapper without a twin
    w3, fs3 = wrapper()
    assert fs3.fast is None and fs3.publish_weights() == "rebuilt" and fs3.fast is not None


# ---------------------------------------------------------------------------------------- 5. argument errors

def test_argument_errors_write_nothing(env):
    L, LN = env["L"], env["LN"]
    call = Call(env, numpy_sd(make_net(env, 3, 61, "cpu")), True)
    src, dst, sc, s = call.src, call.dst, call.scalars, stream(env)

    def blocks(struct, field, k, value):
        arr = type(getattr(struct, field))(*getattr(struct, field))
        arr[k] = value
        return H.swap(struct, **{field: arr})

    def heads(struct, **kw):
        return H.swap(struct, heads=H.swap(struct.heads, **kw))

    dev = lambda a, b, c: L.az_nn_publish_dev(None if a is None else C.byref(a), None if b is None else C.byref(b), c, s)   # noqa: E731
    cases = {
        "null src": dev(None, dst, sc), "null dst": dev(src, None, sc), "null scalars": dev(src, dst, None),
        "null source": dev(H.swap(src, pos_emb=None), dst, sc), "null block source": dev(blocks(src, "block_conv_weight", 2, None), dst, sc),
        "null last source": dev(H.swap(src, aux_out_bias=None), dst, sc),
        "null destination": dev(src, H.swap(dst, o_w=None), sc), "null block destination": dev(src, blocks(dst, "block_beta", 1, None), sc),
        "null head destination": dev(src, heads(dst, d_val_b=None), sc), "null qkvg_w": dev(src, H.swap(dst, qkvg_w=None), sc),
        "n_blocks 0": dev(H.swap(src, n_blocks=0), H.swap(dst, n_blocks=0), sc),
        "n_blocks 9": dev(H.swap(src, n_blocks=9), H.swap(dst, n_blocks=9), sc),
        "n_blocks differ": dev(H.swap(src, n_blocks=2), dst, sc), "n_blocks differ the other way": dev(src, H.swap(dst, n_blocks=2), sc),
        "only stem_frag": dev(src, H.swap(dst, stem_pmap=None), sc), "only stem_pmap": dev(src, H.swap(dst, stem_frag=None), sc),
        "source at 2 bytes": dev(H.swap(src, qkv_weight=src.qkv_weight + 2), dst, sc),
        "scalar source at 2 bytes": dev(H.swap(src, policy_out_bias=src.policy_out_bias + 2), dst, sc),
        "qkvg_w at 2 bytes": dev(src, H.swap(dst, qkvg_w=dst.qkvg_w + 2), sc), "qkvg_w at 8 bytes": dev(src, H.swap(dst, qkvg_w=dst.qkvg_w + 8), sc),
        "block_w at 8 bytes": dev(src, blocks(dst, "block_w", 0, dst.block_w[0] + 8), sc),
        "stem_frag at 8 bytes": dev(src, H.swap(dst, stem_frag=dst.stem_frag + 8), sc),
        "emb_own at 1 byte": dev(src, H.swap(dst, emb_own=dst.emb_own + 1), sc), "d_val_b at 1 byte": dev(src, heads(dst, d_val_b=dst.heads.d_val_b + 1), sc),
        "stem_pmap at 2 bytes": dev(src, H.swap(dst, stem_pmap=dst.stem_pmap + 2), sc), "scalars at 2 bytes": dev(src, dst, sc + 2),
    }
    # the model entry point: a hash evaluator, a null model, a model of another depth
    hash_model, model = C.c_void_p(), C.c_void_p()
    assert L.az_nn_model_create_hash(0, C.byref(hash_model)) == 0 and L.az_nn_model_create(C.byref(dst), C.byref(model)) == 0
    out = (C.c_float * 3)()
    learner = LN.NativeLearner(LH.module(env), 64)
    try:
        cases["hash model"] = L.az_nn_model_publish(hash_model, C.byref(src), sc, s)
        cases["hash model's biases"] = L.az_nn_model_head_biases(hash_model, C.byref(out))
        cases["hash model's biases set"] = L.az_nn_model_set_head_biases(hash_model, 0.0, 0.0, 0.0)
        cases["null model"] = L.az_nn_model_publish(None, C.byref(src), sc, s)
        cases["model of 3 blocks, source of 2"] = L.az_nn_model_publish(model, C.byref(H.swap(src, n_blocks=2)), sc, s)
        cases["model, null source struct"] = L.az_nn_model_publish(model, None, sc, s)
        cases["model, null scalars"] = L.az_nn_model_publish(model, C.byref(src), None, s)
        # the learner's: a learner of 3 blocks and a model of 2, null arguments
        shallow = C.c_void_p()
        assert L.az_nn_model_create(C.byref(H.swap(dst, n_blocks=2)), C.byref(shallow)) == 0
        try:
            cases["learner of 3 blocks, model of 2"] = L.az_learn_publish(learner._handle, shallow, sc, s)
        finally:
            L.az_nn_model_destroy(shallow)
        cases["learner, hash model"] = L.az_learn_publish(learner._handle, hash_model, sc, s)
        cases["learner, null model"] = L.az_learn_publish(learner._handle, None, sc, s)
        cases["null learner"] = L.az_learn_publish(None, model, sc, s)
        cases["learner, null scalars"] = L.az_learn_publish(learner._handle, model, None, s)
        cases["learner, scalars at 2 bytes"] = L.az_learn_publish(learner._handle, model, sc + 2, s)
        assert {k: v for k, v in cases.items() if v != AZ_ERR_ARG} == {}
        assert call.untouched(env)
        # and the same structs, unchanged, are accepted: the refusals above were the changes'
        assert L.az_nn_model_publish(model, C.byref(src), sc, s) == 0
        assert not call.untouched(env)
    finally:
        L.az_nn_model_destroy(hash_model)
        L.az_nn_model_destroy(model)
        learner.close()
    # what the Python entry point refuses
    PB, FN = env["PB"], env["FN"]
    fast = FN.FastConnect4Net.from_module(make_net(env, 3, 62))
    with pytest.raises(ValueError, match="blocks"):
        PB.publish(fast, make_net(env, 1, 63))
    with pytest.raises(ValueError, match="CUDA"):
        PB.publish(fast, make_net(env, 3, 63, "cpu"))
    with pytest.raises(ValueError, match="float32"):
        PB.publish(fast, make_net(env, 3, 63).double())
    odd = make_net(env, 3, 63)
    odd.orbit_map[5] = 3
    with pytest.raises(ValueError, match="orbit_map"):
        PB.publish(fast, odd)
    with pytest.raises(ValueError, match="all-HIP"):
        PB.publish(FN.FastConnect4Net(make_net(env, 3, 63, "cpu").state_dict(), "cpu"), make_net(env, 3, 63))
