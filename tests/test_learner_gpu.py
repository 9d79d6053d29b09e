"""The native learner on the device (az_learn_* in include/az_train.h, csrc/learn_driver.hip, src/learner.py).

1. k_learn_keep in bytes: after one `step` on 5 rows the keep tensors, read through az_learn_outputs, equal the numpy
   restatement of the contract (tests/learner_ref.py) byte for byte at rates (0.2, 0.2, 0.2, 0.2) and (0.5, 0, 0.1, 0); a
   tensor at rate 0 and every row past the batch still hold the pattern the test put there; the same (seed, call) gives
   the same bytes, the next call others.
2. dropout 0: `NativeLearner.train_step` over three 64-row batches leaves the 6-tuple, every parameter, both moments and
   every step counter byte for byte as `adopt_all` + `train_step(route="kernel")` + `ClipAdamW` leave them on a twin.
3. dropout 0.2: one native `step` on 7 rows under max_workgroups = 3 against the functional chain run by hand with the
   keeps the learner drew: every gradient, the three losses and the gradient norm in bytes.
4. the values of 2 against the float64 net on the CPU: policy, value and aux loss and the gradient norm may deviate by
   train_ref_common's bound - 4 x what the unadopted float32 twin deviates, or 1e-6 - as test_train_heads_gpu.py holds
   `adopt_all`.
5. az_learn_dev_epoch over a ring of 200 rows, 150 indices, B = 64 (128, 128 and 44 rows) against per-batch `step` over
   the same `ReplayBatches`; with drop_last two batches; sums and the batch count.
6. two native batches, then `opt.clip_step(5)` on the Python route, against a twin that did all three in Python.
7. a LambdaLR that halves per `train_step` is seen by the next call; az_learn_dev_eval's confusion is `training_loss`'s on
   the module's own eval forward.
8. every AZ_ERR_ARG case leaves the bound tensors, between guard regions, as they were; a good step writes parameters,
   gradients and moments only."""
import ctypes as C

import numpy as np
import pytest

import learner_harness as LH
import learner_ref as LR
import train_gpu_harness as H
import train_ref_common as R
from train_gpu_harness import AZ_ERR_ARG, FILL, Slab, loaders

pytestmark = pytest.mark.gpu

SEED = 0x5EED1234ABCD


@pytest.fixture(scope="module")
def env():
    return LH.load_env()


def config(env):
    return env["TL"].LossConfig(**LH.KNOBS)


def rows(batch, n):
    return tuple(t[:n] for t in batch)


def put_pattern(env, learner, n):
    """Every keep tensor of n rows becomes the fill pattern, written through the addresses az_learn_outputs returned."""
    torch = env["torch"]
    blocks, attn, policy, pool = learner.keeps(n)
    for t in blocks + [attn, policy, pool]:
        t.view(torch.uint8).fill_(FILL)
    torch.cuda.synchronize()


def read_keeps(learner, n):
    blocks, attn, policy, pool = learner.keeps(n)
    return dict(blocks=[b.cpu().numpy() for b in blocks], attn=attn.cpu().numpy().view(np.uint64), policy=policy.cpu().numpy(),
                pool=pool.cpu().numpy())


def same_bytes(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---------------------------------------------------------------------------------------- 1. the keep kernel in bytes

@pytest.mark.parametrize("rates", ((0.2, 0.2, 0.2, 0.2), (0.5, 0.0, 0.1, 0.0)))
def test_keeps_are_the_restatement_in_bytes(env, rates):
    LN = env["LN"]
    n, cap = 5, 8
    batch = rows(loaders(env)["cuda"][0], n)
    learner = LN.NativeLearner(LH.module(env, dropout=rates), cap, seed=SEED)
    assert learner.rates == rates and learner.n_blocks == 3
    put_pattern(env, learner, cap)
    learner.step(batch, config(env))
    got, want = read_keeps(learner, cap), LR.keeps(SEED, 0, n, 3, rates)
    for name in ("attn", "policy", "pool"):
        if want[name] is None:
            assert (got[name].view(np.uint8) == FILL).all(), name + " at rate 0 was written"
        else:
            assert same_bytes(got[name][:n], want[name]), name
            assert (got[name][n:].view(np.uint8) == FILL).all(), name + " past the batch was written"
    for k in range(3):
        if want["blocks"] is None:
            assert (got["blocks"][k].view(np.uint8) == FILL).all()
        else:
            assert same_bytes(got["blocks"][k][:n], want["blocks"][k]), "block %d" % k
            assert (got["blocks"][k][n:].view(np.uint8) == FILL).all()
    if rates[1] > 0:
        assert not (got["attn"][:n] >> np.uint64(42)).any()
    # the same (seed, call) on another handle: the same bytes; the next call: the restatement's next
    other = LN.NativeLearner(LH.module(env, dropout=rates), cap, seed=SEED)
    other.step(batch, config(env))
    again = read_keeps(other, n)
    other.step(batch, config(env))
    later, want1 = read_keeps(other, n), LR.keeps(SEED, 1, n, 3, rates)
    assert same_bytes(again["policy"], want["policy"]) and same_bytes(again["blocks"][2], want["blocks"][2])
    assert same_bytes(later["policy"], want1["policy"]) and same_bytes(later["blocks"][0], want1["blocks"][0])
    assert not same_bytes(later["policy"], again["policy"])
    if rates[1] > 0:
        assert same_bytes(again["attn"], want["attn"]) and same_bytes(later["attn"], want1["attn"])
    other.draw_keeps(n, 0)                                      # the launch alone, numbered as the first batch was
    alone = read_keeps(other, n)
    assert same_bytes(alone["policy"], want["policy"]) and all(same_bytes(a, w) for a, w in zip(alone["blocks"], want["blocks"]))
    learner.close()
    other.close()


# ---------------------------------------------------------------------------------------- 2. and 4. three batches, dropout 0

@pytest.fixture(scope="module")
def three_batches(env):
    """The Python route (twin A) and the native learner (twin B) over the same three 64-row batches, once."""
    TL, LN = env["TL"], env["LN"]
    a = LH.python_twin(env)
    values_a = TL.train_step(a, loaders(env)["cuda"], lambda b: b, n_epochs=1, route="kernel", **LH.KNOBS)
    b = LH.module(env)
    learner = LN.NativeLearner(b, 64)
    values_b = learner.train_step(loaders(env)["cuda"], n_epochs=1, **LH.KNOBS)
    out = dict(python=(values_a, LH.trained_state(a)), native=(values_b, LH.trained_state(b)))
    learner.close()
    return out


def test_native_equals_the_python_route_in_bytes(env, three_batches):
    (values_a, state_a), (values_b, state_b) = three_batches["python"], three_batches["native"]
    print("python", values_a)
    print("native", values_b)
    assert LH.first_difference(state_a, state_b) is None
    assert values_a == values_b
    assert all(float(state_b["t.%d" % i]) == 3.0 for i in range(40))


@pytest.fixture(scope="module")
def baselines(env):
    return H.baselines(env, stem_bias=True)


def test_native_against_float64(env, three_batches, baselines):
    values, twin_values, exact_values = three_batches["native"][0], baselines["twin"], baselines["exact"]
    figures = []
    for i, what in ((0, "policy loss"), (1, "value loss"), (2, "aux loss"), (4, "grad norm")):
        exact = exact_values[i]
        dev, own = (abs(v[i] - exact) / abs(exact) for v in (values, twin_values))
        print("train_step native %-11s exact %.9g  native %.3e  twin %.3e  bound %.3e" % (what, exact, dev, own, R.bound(own)))
        figures.append((what, dev, own))
    for what, dev, own in figures:
        assert dev <= R.bound(own), (what, dev, own)


# ---------------------------------------------------------------------------------------- 3. dropout, against the chain by hand

def test_native_step_with_dropout_equals_the_chain_by_hand(env):
    torch, LN, TS, TB, TA, TH, TL = (env[k] for k in ("torch", "LN", "TS", "TB", "TA", "TH", "TL"))
    n, cap_wg, rates = 7, 3, (0.2, 0.2, 0.2, 0.2)
    batch = rows(loaders(env)["cuda"][1], n)
    net = LH.module(env, dropout=rates)
    learner = LN.NativeLearner(net, 8, seed=SEED + 1, max_workgroups=cap_wg)
    learner.step(batch, config(env))
    blocks, attn, policy, pool = (([b.clone() for b in k] if isinstance(k, list) else k.clone()) for k in learner.keeps(n))
    got_grads = {k: p.grad.clone() for k, p in net.named_parameters()}
    got_losses, got_norm = learner.losses.clone(), learner.grad_norm.clone()

    twin = LH.module(env, dropout=rates)                     # the same seed: the parameters before the step
    env["O"].adopt(twin.opt)
    layers = list(twin.hidden.children())
    conv, attn_mod = layers[0], layers[-1].attn
    x = TS.stem(batch[0], twin.piece_emb.weight, twin.pos_emb.weight, conv.weight, conv.bias, route="kernel", max_workgroups=cap_wg)
    for k, b in enumerate(layers[2:-1]):
        x = TB.residual_block(x, b.norm.weight, b.norm.bias, b.conv.weight, b.conv.bias, keep=blocks[k], eps=b.norm.eps, route="kernel",
                              max_workgroups=cap_wg)
    tokens = TA.gated_attention(x, attn_mod.prenorm.weight, attn_mod.qkv_proj.weight, attn_mod.gate_proj.weight, attn_mod.o_proj.weight,
                                attn_mod.q_norm.weight, attn_mod.k_norm.weight, keep_bits=attn, keep_scale=learner.keep_scale,
                                eps=attn_mod.prenorm.eps, route="kernel", max_workgroups=cap_wg)
    log_p, value, steps = TH.heads(tokens, batch[6], *(TH._resolve(twin, path) for _, path, _ in TH.PARAMS), keep_policy=policy,
                                   keep_pool=pool, eps=twin.policy_head.norm.eps, route="kernel", max_workgroups=cap_wg)
    loss = TL.training_loss(log_p, value, steps, batch, twin.aux_target_offset, config(env), "kernel")
    loss.total.backward()
    norm = twin.opt.clip_step(5)
    for k, p in twin.named_parameters():
        assert torch.equal(p.grad, got_grads[k]), k
    want_losses = torch.stack([loss.policy.detach(), loss.value.detach(), loss.aux.detach(), loss.entropy])
    assert got_losses.cpu().numpy().tobytes() == want_losses.cpu().numpy().tobytes()
    assert got_norm.cpu().numpy().tobytes() == norm.reshape(1).cpu().numpy().tobytes()
    assert LH.first_difference(LH.trained_state(twin), LH.trained_state(net)) is None
    learner.close()


# ---------------------------------------------------------------------------------------- 5. az_learn_dev_epoch

def test_epoch_equals_the_steps(env):
    torch, LN = env["torch"], env["LN"]
    buf = LH.ring(env, 200)
    gen = torch.Generator().manual_seed(5)
    idx = torch.randint(0, 200, (150,), generator=gen)
    order = torch.randperm(150, generator=gen)
    batches = buf.batches(idx, 64, order=order)
    assert len(batches) == 3 and [b[0].shape[0] for b in batches] == [128, 128, 44]
    nets = [LH.module(env), LH.module(env)]
    by_step, by_epoch = (LN.NativeLearner(net, 128, seed=SEED) for net in nets)
    by_step.reset_sums()
    for b in batches:
        by_step.step(b, config(env))
    assert by_epoch.epoch(batches, config(env)) == (3, 44)
    assert LH.first_difference(LH.trained_state(nets[0]), LH.trained_state(nets[1])) is None
    for name in ("sums", "batches", "entropy", "losses", "counts", "grad_norm"):
        assert torch.equal(getattr(by_step, name), getattr(by_epoch, name)), name
    assert int(by_epoch.batches) == 3 and by_epoch.calls == 3
    # the whole train_step, eval forward on the handle's own last batch included
    values = [ln.train_step(batches, n_epochs=1, **LH.KNOBS) for ln in (by_epoch,)]
    assert int(by_epoch.batches) == 3 and all(np.isfinite(values[0]))
    short = buf.batches(idx, 64, order=order, drop_last=True)
    assert by_epoch.epoch(short, config(env)) == (2, 128) and int(by_epoch.batches) == 5
    with pytest.raises(ValueError, match="max_rows"):
        by_epoch.epoch(buf.batches(idx, 65, order=order), config(env))
    by_step.close()
    by_epoch.close()


# ---------------------------------------------------------------------------------------- 6. the optimiser changes hands

def test_the_python_route_takes_over(env):
    LN, TH = env["LN"], env["TH"]
    batches = loaders(env)["cuda"]
    twin = LH.python_twin(env)
    for b in batches:
        LH.python_batch(env, twin, b, config(env))
    net = LH.module(env)
    learner = LN.NativeLearner(net, 64)
    for b in batches[:2]:
        learner.step(b, config(env))
    assert TH.adopt_all(net) == (3, 1, 1, 1)
    LH.python_batch(env, net, batches[2], config(env))
    assert LH.first_difference(LH.trained_state(twin), LH.trained_state(net)) is None
    state = net.opt.state_dict()["state"]
    assert len(state) == 40 and all(float(state[i]["step"]) == 3.0 for i in range(40))
    # and back: the learner follows the optimiser's counters
    learner.step(batches[0], config(env))
    LH.python_batch(env, twin, batches[0], config(env))
    assert LH.first_difference(LH.trained_state(twin), LH.trained_state(net)) is None
    learner.close()


# ---------------------------------------------------------------------------------------- 7. scheduler and eval

def test_scheduler_and_eval(env):
    torch, LN, TL, TH = env["torch"], env["LN"], env["TL"], env["TH"]
    batches = loaders(env)["cuda"]

    def halving(net):
        net.scheduler = torch.optim.lr_scheduler.LambdaLR(net.opt, lambda e: 0.5 ** e)
        return net
    twin = halving(LH.python_twin(env))
    python_values = [TL.train_step(twin, batches, lambda b: b, n_epochs=1, route="kernel", **LH.KNOBS) for _ in range(2)]
    net = halving(LH.module(env))
    learner = LN.NativeLearner(net, 64)
    native_values = [learner.train_step(batches, n_epochs=1, **LH.KNOBS) for _ in range(2)]
    assert native_values == python_values
    assert LH.first_difference(LH.trained_state(twin), LH.trained_state(net)) is None
    assert [g["lr"] for g in net.opt.param_groups] == [g["lr"] for g in twin.opt.param_groups] and net.opt.param_groups[0]["lr"] == 1e-3 / 4
    flat = LH.module(env)
    steady = LN.NativeLearner(flat, 64)
    for _ in range(2):
        steady.train_step(batches, n_epochs=1, **LH.KNOBS)
    assert LH.first_difference(LH.trained_state(flat), LH.trained_state(net)) is not None
    # az_learn_dev_eval against the module's own eval forward
    got = learner.evaluate(batches[1], config(env))
    got = [t.clone() for t in (got.policy, got.value, got.aux, got.entropy, got.confusion)]
    assert TH.adopt_all(net) == (3, 1, 1, 1)
    net.eval()
    with torch.no_grad():
        want = TL.training_loss(*net(batches[1][0], action_mask=batches[1][6]), batches[1], net.aux_target_offset, config(env), "kernel")
    for g, w in zip(got, (want.policy, want.value, want.aux, want.entropy, want.confusion)):
        assert torch.equal(g, w)
    assert int(got[4].sum()) == 64
    learner.close()
    steady.close()


# ---------------------------------------------------------------------------------------- 8. argument errors

def test_argument_errors_enqueue_and_write_nothing(env):
    torch, L, abi, LN, O = env["torch"], env["L"], env["abi"], env["LN"], env["O"]
    net = LH.module(env, "cpu")
    conv, blocks, attn_block, eps_block, eps_attn, eps_heads = LN._layout(net)
    role_of = {id(t): r for t, r in LN._roles(net, conv, blocks, attn_block)}
    flat = [p for g in net.opt.param_groups for p in g["params"]]
    n = len(flat)
    assert n == 40 and sorted(role_of.values()) == list(range(4 + 12)) + list(range(36, 60))
    roles = [role_of[id(p)] for p in flat]
    groups = [gi for gi, g in enumerate(net.opt.param_groups) for _ in g["params"]]
    n_rows = 5
    batch = [t[:n_rows].numpy() for t in loaders(env)["cpu"][0]]
    inputs = {"p%d" % i: p.detach().numpy() for i, p in enumerate(flat)}
    inputs.update({"m%d" % i: np.zeros(p.numel(), np.float32) for i, p in enumerate(flat)})
    inputs.update({"v%d" % i: np.zeros(p.numel(), np.float32) for i, p in enumerate(flat)})
    inputs.update({"b%d" % i: b for i, b in enumerate(batch)})
    slab = Slab(torch, inputs, {"g%d" % i: 4 * p.numel() for i, p in enumerate(flat)})
    arr = C.c_void_p * n
    ptrs = {k: [slab.ptr("%s%d" % (k, i)) for i in range(n)] for k in "pgmv"}
    batch_c = abi.ReplayBatchC(*(slab.ptr("b%d" % i) for i in range(8)))
    cfg = env["TL"].config_c(config(env), 42)
    step = (C.c_int64 * n)(*([1] * n))
    hp = (C.c_double * 80)()
    for gi, g in enumerate(net.opt.param_groups):
        hp[5 * gi:5 * gi + 5] = (g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"])

    def learn_config(**kw):
        base = dict(max_rows=8, n_blocks=3, max_workgroups=0, eps_block=eps_block, eps_attn=eps_attn, eps_heads=eps_heads, max_norm=5.0,
                    p_block=0.0, p_attn=0.0, p_policy=0.0, p_pool=0.0, seed=1)
        return LN.LearnConfigC(**dict(base, **kw))

    def bind(handle, roles=roles, **shift):
        q = {k: list(v) for k, v in ptrs.items()}
        for k, (i, by) in shift.items():
            q[k][i] += by
        return L.az_learn_bind(handle, n, (C.c_int32 * n)(*roles), (C.c_int32 * n)(*groups), len(net.opt.param_groups),
                               arr(*q["p"]), arr(*q["g"]), arr(*q["m"]), arr(*q["v"]))

    def dev_step(handle, b=batch_c, rows=n_rows):
        return L.az_learn_dev_step(handle, None if b is None else C.byref(b), rows, C.byref(cfg), step, hp, 0,
                                   abi._stream())
    handle = C.c_void_p()
    for bad in (dict(n_blocks=0), dict(n_blocks=9), dict(p_block=-0.1), dict(p_attn=1.0), dict(p_pool=float("nan")), dict(max_rows=0),
                dict(eps_heads=0.0)):
        assert L.az_learn_create(C.byref(learn_config(**bad)), C.byref(handle)) == AZ_ERR_ARG and not handle.value, bad
    assert L.az_learn_create(C.byref(learn_config()), C.byref(handle)) == 0
    try:
        assert dev_step(handle) == AZ_ERR_ARG                                   # a step before bind
        conv_w = roles.index(LN.ROLE_BLOCK + 2)                                 # a tensor its unit wants 16-byte aligned
        twice = list(roles)
        twice[1] = twice[0]                                                     # one role twice, so another is missing
        assert bind(handle, roles=twice) == AZ_ERR_ARG
        assert bind(handle, roles=roles[:-1] + [LN.ROLE_BLOCK + 12]) == AZ_ERR_ARG      # a fourth block's role
        assert bind(handle, g=(conv_w, 4)) == AZ_ERR_ARG
        assert bind(handle, g=(0, 2)) == AZ_ERR_ARG
        assert bind(handle, m=(3, 2)) == AZ_ERR_ARG
        assert bind(handle, p=(conv_w, 8)) == AZ_ERR_ARG
        assert L.az_learn_bind(handle, n - 1, (C.c_int32 * n)(*roles), (C.c_int32 * n)(*groups), 5, arr(*ptrs["p"]), arr(*ptrs["g"]),
                               arr(*ptrs["m"]), arr(*ptrs["v"])) == AZ_ERR_ARG
        assert dev_step(handle) == AZ_ERR_ARG                                   # still unbound
        assert bind(handle) == 0
        assert dev_step(handle, rows=9) == AZ_ERR_ARG                           # N > max_rows
        assert dev_step(handle, rows=0) == AZ_ERR_ARG
        assert dev_step(handle, b=None) == AZ_ERR_ARG
        assert dev_step(handle, b=H.swap(batch_c, prob=None)) == AZ_ERR_ARG
        assert dev_step(handle, b=H.swap(batch_c, state=batch_c.state + 4)) == AZ_ERR_ARG
        assert L.az_learn_dev_eval(handle, None, n_rows, C.byref(cfg), abi._stream()) == AZ_ERR_ARG
        step[7] = 0
        assert dev_step(handle) == AZ_ERR_ARG
        step[7] = 1
        assert L.az_learn_outputs(handle, None) == AZ_ERR_ARG
        torch.cuda.synchronize()
        assert np.array_equal(slab.dev.cpu().numpy(), slab.host), "a refused call wrote something"
        assert dev_step(handle) == 0
        torch.cuda.synchronize()
        image = slab.dev.cpu().numpy()
        written = [k + str(i) for k in "pgmv" for i in range(n)]
        assert slab.untouched_outside(image, written)
        for i in range(n):                                                     # every gradient was written whole
            a, b = slab.at["g%d" % i], slab.size["g%d" % i]
            assert not (image[a:a + b].reshape(-1, 4) == FILL).all(1).any(), i
        a, b = slab.at["p%d" % conv_w], slab.size["p%d" % conv_w]
        assert not np.array_equal(image[a:a + b], slab.host[a:a + b])           # and the step was taken
    finally:
        L.az_learn_destroy(handle)
