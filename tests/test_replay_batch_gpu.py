"""Augmented training batches out of the replay ring on the device (k_replay_batch and k_replay_indices:
az_replay_dev_batch / az_replay_dev_sample_indices in include/az_mcts.h, `ReplayTensors.batches`,
`SampledReplayTensors.sample` and `ReplayBatches` in src/replay.py).

1. the kernel against what the reference's `get` + `augment` returned (fixture G16), both games, whole and split
   batches, with and without `order`;
2. at scale: rings filled by a real `NativeSelfPlay(...).export` (refill, noise, symmetry on), B = 512 and 4096,
   thousands of random indices with duplicates: the kernel route equals the torch route bit for bit;
3. indices outside the ring give zero rows, leave their neighbours intact and write nothing outside the batch
   (guard regions around every output tensor);
4. the C ABI alone through ctypes, with each AZ_ERR_ARG case;
5. az_replay_dev_sample_indices: deterministic per (seed, call), different across calls, in range, uniform by the
   chi-square rule of tests/test_devrng_gpu.py - and that rule rejects a biased index array;
6. step / export / batch interleaved on one stream with no wait of the test's in between: every batch equals the
   torch route on a clone of the ring taken at the same point in stream order;
7. reference-shaped consumer lines give the same on both routes; `sample` end to end on the device.

All row comparisons are bit for bit.  The reference itself is never imported here: the golden file stands for it.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from test_replay_batch_cpu import (GAMES, GEOMETRY, TENSORS, batch_arrays, check_shapes, differences, golden_batch,
                                   golden_buffer, reassembled)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
AZ_ERR_ARG = 1


@pytest.fixture(scope="module")
def env():
    sys.path.insert(0, ROOT)
    import torch  # noqa: F401  (before the engine library: one HIP runtime per process)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import torch
    from src import fused, hash_eval, replay, selfplay
    return dict(torch=torch, F=fused, H=hash_eval, SP=selfplay, RP=replay, L=fused.lib())


def hash_net(env, game):
    return env["H"].HashEvaluator("cuda") if game == "Connect4" else env["H"].OthelloHashEvaluator("cuda")


def one_batch(buf, idx, route):
    (batch,) = list(buf.batches(idx, len(idx), route=route))
    return batch


# ---------------------------------------------------------------------------------------- 1. the fixture

@pytest.mark.parametrize("key", sorted(GAMES))
def test_kernel_equals_the_reference_batch(env, key):
    RP = env["RP"]
    game = GAMES[key]
    S = GEOMETRY[game][3]
    buf = golden_buffer(RP, key, "cuda")
    idx, expected = golden_batch(key)
    n = len(idx)
    loader = buf.batches(idx, n)
    assert loader.route == "kernel"
    whole = list(loader)
    assert len(whole) == 1
    check_shapes(RP, game, whole[0], n)
    assert all(x.is_cuda and x.is_contiguous() for x in whole[0])
    assert differences(batch_arrays(whole[0]), expected) == []
    order = np.random.default_rng(8).permutation(n)
    permuted = {t: np.concatenate([expected[t][s * n:(s + 1) * n][order] for s in range(S)]) for t in TENSORS}
    for size in (1, 7, 31, n):
        parts = list(buf.batches(idx, size, route="kernel"))
        assert len(parts) == (n + size - 1) // size
        assert differences(reassembled(parts, S), expected) == []
        assert differences(reassembled(list(buf.batches(idx, size, order=order, route="kernel")), S), permuted) == []
        kept = list(buf.batches(idx, size, order=order, route="kernel", drop_last=True))
        m = (n // size) * size
        assert len(kept) == n // size
        cut = {t: np.concatenate([permuted[t][s * n:s * n + m] for s in range(S)]) for t in TENSORS}
        assert differences(reassembled(kept, S), cut) == []
    # two passes over one loader hand out fresh tensors with the same content
    again = next(iter(loader))
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(again, whole[0]))
    assert differences(batch_arrays(again), expected) == []


# ---------------------------------------------------------------------------------------- 2. at scale

def played_ring(env, game, n_games, plies, every, capacity, cls=None):
    SP, RP = env["SP"], env["RP"]
    sp = SP.NativeSelfPlay(hash_net(env, game), n_games, n_playout=16, vl_batch=4, seed=33, temp_decay_moves=10, record=True,
                           td_steps=3, refill=True, game=game)
    buf = (cls or RP.ReplayTensors)(game, capacity, "cuda")
    for _ in range(plies // every):
        sp.step(every)
        sp.export(buf)
    return sp, buf


def consumer_lines(batch):
    """What the reference's training step derives first from a batch (written here, not imported)."""
    state, prob = batch[0], batch[1]
    policy_mask = prob.sum(1) > 0
    turn = state[:, 2, 0, 0]
    return policy_mask.cpu().numpy(), np.ascontiguousarray(turn.cpu().numpy())


@pytest.mark.parametrize("game,n_games,plies,every,capacity,at_least", [
    ("Connect4", 2048, 40, 10, 30011, 20000), ("Othello", 256, 140, 20, 9001, 5000)])
def test_kernel_route_equals_torch_route_at_scale(env, game, n_games, plies, every, capacity, at_least):
    torch = env["torch"]
    _sp, buf = played_ring(env, game, n_games, plies, every, capacity)
    assert len(buf) >= at_least, len(buf)
    S = GEOMETRY[game][3]
    gen = torch.Generator(device="cuda")
    gen.manual_seed(77)
    n = 8192 + 300                                                       # a short last batch at both sizes
    idx = torch.randint(0, len(buf), (n,), device="cuda", generator=gen)
    idx[1000:1100] = idx[0]                                              # a run of duplicates on top of the chance ones
    assert len(torch.unique(idx)) < n - 99
    order = torch.randperm(n, device="cuda", generator=gen)
    for size in (512, 4096):
        for o in (None, order):
            fast = list(buf.batches(idx, size, order=o, route="kernel"))
            slow = list(buf.batches(idx, size, order=o, route="torch"))
            assert len(fast) == len(slow) == (n + size - 1) // size
            with_policy = []
            for a, b in zip(fast, slow):
                check_shapes(env["RP"], game, a, a[2].shape[0] // S)
                assert differences(batch_arrays(a), batch_arrays(b)) == []
                pa, ta = consumer_lines(a)
                pb, tb = consumer_lines(b)
                assert np.array_equal(pa, pb) and np.array_equal(ta.view(np.uint32), tb.view(np.uint32))
                assert set(np.unique(ta).tolist()) <= {-1.0, 1.0}
                with_policy.append(pa)
            with_policy = np.concatenate(with_policy)
            assert with_policy.any() and not with_policy.all()           # positions and end states
    print("batches at scale:", game, len(buf), "rows in the ring,", n, "sampled")


# ---------------------------------------------------------------------------------------- 3. rows outside the ring

@pytest.mark.parametrize("key", sorted(GAMES))
def test_rows_outside_the_ring_are_zero_and_nothing_else_is_touched(env, key):
    torch, SP, RP, L, F = env["torch"], env["SP"], env["RP"], env["L"], env["F"]
    game = GAMES[key]
    A, R, Cc, S = GEOMETRY[game]
    buf = golden_buffer(RP, key, "cuda")
    cap = buf.current_capacity
    good, _ = golden_batch(key)
    idx = good[:24].copy()
    outside = {1: -1, 4: cap, 5: cap + 5, 11: 2 ** 62, 12: -2 ** 63, 23: -cap}
    for at, v in outside.items():
        idx[at] = v
    B = len(idx)
    GUARD = 256
    shapes = dict(state=(np.float32, (3, R, Cc)), prob=(np.float32, (A,)), winner=(np.int8, (1,)), steps_to_end=(np.int16, (1,)),
                  aux_target=(np.int16, (1,)), root_wdl=(np.float32, (3,)), valid_mask=(np.uint8, (A,)), future_root_wdl=(np.float32, (3,)))
    slabs, nbytes = {}, {}
    for t, (dtype, tail) in shapes.items():
        nbytes[t] = S * B * int(np.prod(tail)) * np.dtype(dtype).itemsize
        slabs[t] = torch.full((GUARD + nbytes[t] + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        assert (slabs[t].data_ptr() + GUARD) % 16 == 0
    out = SP.ReplayBatchC(*(slabs[t].data_ptr() + GUARD for t in TENSORS))
    d_idx = torch.from_numpy(idx).cuda()
    F.check(L.az_replay_dev_batch(0 if game == "Connect4" else 1, C.byref(RP.replay_tensors_c(buf, game, "cuda")), d_idx.data_ptr(),
                                  None, 0, B, C.byref(out), F._stream()))
    torch.cuda.synchronize()
    inside = np.array([i for i in range(B) if i not in outside])
    expected = batch_arrays(one_batch(buf, idx[inside], "torch"))
    for t, (dtype, tail) in shapes.items():
        raw = slabs[t].cpu().numpy()
        assert (raw[:GUARD] == 0xA5).all() and (raw[GUARD + nbytes[t]:] == 0xA5).all(), t
        got = raw[GUARD:GUARD + nbytes[t]].view(dtype).reshape((S, B) + tail)
        for at in outside:
            assert not np.ascontiguousarray(got[:, at]).view(np.uint8).any(), (t, at)
        want = expected[t].reshape((S, len(inside)) + tail)
        assert np.array_equal(np.ascontiguousarray(got[:, inside]).view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), t
    # through the Python route: the same zero rows
    batch = batch_arrays(one_batch(buf, idx, "kernel"))
    for t, (dtype, tail) in shapes.items():
        got = batch[t].reshape((S, B) + tail)
        assert all(not np.ascontiguousarray(got[:, at]).view(np.uint8).any() for at in outside), t


# ---------------------------------------------------------------------------------------- 4. the C ABI alone

class RawTensors(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TENSORS] + [("capacity", C.c_int64)]


class RawBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in TENSORS]


def test_c_abi_alone_via_ctypes(env):
    torch, RP = env["torch"], env["RP"]
    L = C.CDLL(os.path.join(PKG, "lib", "libaz_mcts.so"))
    L.az_last_error.restype = C.c_char_p
    vp, i64, u64 = C.c_void_p, C.c_int64, C.c_uint64
    L.az_game_num_augment.argtypes = [C.c_int]
    L.az_replay_dev_batch.argtypes = [C.c_int, C.POINTER(RawTensors), vp, vp, i64, i64, C.POINTER(RawBatch), vp]
    L.az_replay_dev_sample_indices.argtypes = [u64, u64, i64, vp, i64, vp]
    assert (L.az_game_num_augment(0), L.az_game_num_augment(1), L.az_game_num_augment(2), L.az_game_num_augment(-1)) == (2, 4, -1, -1)
    for key, game_id in (("c4", 0), ("ot", 1)):
        game = GAMES[key]
        A, R, Cc, S = GEOMETRY[game]
        buf = golden_buffer(RP, key, "cuda")
        idx, expected = golden_batch(key)
        n = len(idx)
        order = np.random.default_rng(1).permutation(n)
        d_idx, d_order = torch.from_numpy(idx).cuda(), torch.from_numpy(order).cuda()
        src = RawTensors(*(getattr(buf, t).data_ptr() for t in TENSORS), buf.current_capacity)

        def fresh(rows):
            ts = (torch.zeros((rows, 3, R, Cc), device="cuda"), torch.zeros((rows, A), device="cuda"),
                  torch.zeros((rows, 1), dtype=torch.int8, device="cuda"), torch.zeros((rows, 1), dtype=torch.int16, device="cuda"),
                  torch.zeros((rows, 1), dtype=torch.int16, device="cuda"), torch.zeros((rows, 3), device="cuda"),
                  torch.zeros((rows, A), dtype=torch.bool, device="cuda"), torch.zeros((rows, 3), device="cuda"))
            return ts, RawBatch(*(t.data_ptr() for t in ts))
        torch.cuda.synchronize()
        ts, out = fresh(S * n)
        assert L.az_replay_dev_batch(game_id, C.byref(src), d_idx.data_ptr(), None, 0, n, C.byref(out), None) == 0, L.az_last_error()
        torch.cuda.synchronize()
        assert differences(batch_arrays(ts), expected) == []
        # a window [first, first + B) of a permutation
        first, B = 5, 17
        ts, out = fresh(S * B)
        assert L.az_replay_dev_batch(game_id, C.byref(src), d_idx.data_ptr(), d_order.data_ptr(), first, B, C.byref(out), None) == 0
        torch.cuda.synchronize()
        pick = order[first:first + B]
        want = {t: np.concatenate([expected[t][s * n:(s + 1) * n][pick] for s in range(S)]) for t in TENSORS}
        assert differences(batch_arrays(ts), want) == []

        # the error cases: AZ_ERR_ARG with a message, nothing enqueued
        before = batch_arrays(ts)

        def refused(word, game_id=game_id, src=src, idx_p=d_idx.data_ptr(), first=0, B=B, out=out):
            rc = L.az_replay_dev_batch(game_id, None if src is None else C.byref(src), idx_p, None, first, B,
                                       None if out is None else C.byref(out), None)
            return rc == AZ_ERR_ARG and word in L.az_last_error()
        assert refused(b"unknown game", game_id=2) and refused(b"unknown game", game_id=-1)
        assert refused(b"B must be positive", B=0) and refused(b"B must be positive", B=-4)
        assert refused(b"first", first=-1)
        for cap in (0, -5):
            assert refused(b"capacity", src=RawTensors(*(getattr(buf, t).data_ptr() for t in TENSORS), cap))
        assert refused(b"null", src=None) and refused(b"null", out=None) and refused(b"null", idx_p=None)
        for missing in TENSORS:
            assert refused(b"null", src=RawTensors(*(None if t == missing else getattr(buf, t).data_ptr() for t in TENSORS),
                                                   buf.current_capacity)), missing
            assert refused(b"null", out=RawBatch(*(None if t == missing else x.data_ptr() for t, x in zip(TENSORS, ts)))), missing
            assert refused(b"aligned", out=RawBatch(*(x.data_ptr() + (8 if t == missing else 0) for t, x in zip(TENSORS, ts)))), missing
            assert refused(b"aligned", src=RawTensors(*(getattr(buf, t).data_ptr() + (4 if t == missing else 0) for t in TENSORS),
                                                      buf.current_capacity)), missing
        torch.cuda.synchronize()
        assert differences(batch_arrays(ts), before) == []

    d = torch.zeros(64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    assert L.az_replay_dev_sample_indices(1, 0, 10, d.data_ptr(), 64, None) == 0, L.az_last_error()
    assert L.az_replay_dev_sample_indices(1, 0, 10, None, 0, None) == 0, L.az_last_error()
    for args, word in (((1, 0, 0, d.data_ptr(), 64), b"n_valid"), ((1, 0, -3, d.data_ptr(), 64), b"n_valid"),
                       ((1, 0, 10, d.data_ptr(), -1), b"n must not"), ((1, 0, 10, None, 64), b"null")):
        assert L.az_replay_dev_sample_indices(*args, None) == AZ_ERR_ARG and word in L.az_last_error(), args
    torch.cuda.synchronize()
    got = d.cpu().numpy()
    assert got.min() >= 0 and got.max() < 10 and len(np.unique(got)) > 5


# ---------------------------------------------------------------------------------------- 5. the index draw

def device_indices(env, seed, call, n_valid, n):
    torch, L, F = env["torch"], env["L"], env["F"]
    out = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    F.check(L.az_replay_dev_sample_indices(seed, call, n_valid, out.data_ptr(), n, F._stream()))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def index_problems(idx, n_valid, buckets):
    """The chi-square rule of tests/test_devrng_gpu.py (`uniform_problems`: p < 1e-4 rejects) over `buckets` equal
    ranges of [0, n_valid) (n_valid a multiple of `buckets`, or buckets == n_valid)."""
    from scipy import stats
    if idx.min() < 0 or idx.max() >= n_valid:
        return ["indices outside [0, %d)" % n_valid]
    assert n_valid % buckets == 0
    cnt = np.bincount(idx // (n_valid // buckets), minlength=buckets).astype(np.float64)
    p = stats.chisquare(cnt).pvalue
    return ["indices not uniform over %d buckets of [0, %d) (chi-square p = %.2e)" % (buckets, n_valid, p)] if p < 1e-4 else []


def test_sampled_indices_are_seeded_in_range_and_uniform(env):
    a = device_indices(env, 5, 0, 500000, 12500)
    assert np.array_equal(a, device_indices(env, 5, 0, 500000, 12500))
    assert np.array_equal(a[:777], device_indices(env, 5, 0, 500000, 777))          # keyed by the element, not by n
    for other in (device_indices(env, 5, 1, 500000, 12500), device_indices(env, 6, 0, 500000, 12500)):
        assert (other == a).mean() < 0.01
    assert len(np.unique(a)) > 12000
    assert not device_indices(env, 3, 9, 1, 4096).any()
    problems = []
    for seed, call, n_valid, n, buckets in ((11, 0, 7, 200000, 7), (11, 1, 7, 200000, 7), (12, 0, 500000, 400000, 1000),
                                            (12, 3, 500000, 400000, 50), (13, 2, 64, 200000, 64), (14, 0, 3 * 2 ** 20, 400000, 48)):
        idx = device_indices(env, seed, call, n_valid, n)
        assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() < n_valid
        problems += ["seed %d call %d: %s" % (seed, call, p) for p in index_problems(idx, n_valid, buckets)]
    # consecutive elements and consecutive calls are unrelated
    x, y = device_indices(env, 21, 0, 1 << 20, 200000).astype(np.float64), device_indices(env, 21, 1, 1 << 20, 200000).astype(np.float64)
    for u, v, what in ((x[:-1], x[1:], "neighbouring elements"), (x, y, "consecutive calls")):
        r = np.corrcoef(u, v)[0, 1]
        if abs(r) > 4.5 / np.sqrt(len(u)):
            problems.append("%s: correlation %.5f" % (what, r))
    assert not problems, "\n".join(problems)


def test_the_index_check_rejects_a_biased_draw():
    """Power of the rule, on host-made arrays: a modulo-biased draw, a draw that favours one index, a range error."""
    rng = np.random.default_rng(0)
    assert not index_problems(rng.integers(0, 500000, 400000), 500000, 1000)
    assert not index_problems(rng.integers(0, 7, 200000), 7, 7)
    assert index_problems(rng.integers(0, 2 ** 20, 400000) % 500000, 500000, 1000)      # modulo folding: the lowest indices half again as likely
    favoured = rng.integers(0, 7, 200000)
    favoured[rng.random(200000) < 0.02] = 3
    assert index_problems(favoured, 7, 7)
    assert index_problems(rng.integers(0, 8, 1000), 7, 7) == ["indices outside [0, 7)"]


# ---------------------------------------------------------------------------------------- 6. interleaving

def test_batches_between_steps_and_exports_on_one_stream(env):
    torch, SP, RP = env["torch"], env["SP"], env["RP"]
    game = "Connect4"
    sp = SP.NativeSelfPlay(hash_net(env, game), 512, n_playout=16, vl_batch=4, seed=6, temp_decay_moves=10, record=True,
                           td_steps=2, refill=True, game=game)
    buf = RP.ReplayTensors(game, 4001, "cuda")
    sp.step(12)
    sp.export(buf)
    taken = []
    gen = torch.Generator(device="cuda")
    gen.manual_seed(60)
    for chunk in (5, 7, 9, 6, 8, 11):
        # step, export, a clone of the ring and a batch, all enqueued on the current stream; this test waits for nothing
        sp.step(chunk)
        sp.export(buf)
        assert len(buf) > 0
        idx = torch.randint(0, len(buf), (700,), device="cuda", generator=gen)
        loader = buf.batches(idx, 512)
        snap = RP.ReplayTensors(game, 4001, "cuda")
        for t in TENSORS:
            getattr(snap, t).copy_(getattr(buf, t))
        snap._ptr = buf._ptr
        taken.append((idx, snap, list(loader)))
    assert buf._ptr > 2 * 4001, "the ring was meant to be overwritten between batches"
    rings = [batch_arrays([getattr(s, t) for t in TENSORS]) for _i, s, _b in taken]
    assert all(differences(a, b) for a, b in zip(rings, rings[1:])), "every export changed the ring"
    for idx, snap, got in taken:
        want = list(snap.batches(idx, 512, route="torch"))
        assert len(got) == len(want) == 2
        for a, b in zip(got, want):
            assert differences(batch_arrays(a), batch_arrays(b)) == []


# ---------------------------------------------------------------------------------------- 7. sample, end to end

@pytest.mark.parametrize("key", sorted(GAMES))
def test_sample_on_the_device_end_to_end(env, key):
    torch, RP = env["torch"], env["RP"]
    game = GAMES[key]
    S = GEOMETRY[game][3]
    buf = golden_buffer(RP, key, "cuda", cls=RP.SampledReplayTensors)
    buf.aux_target[:, 0] = torch.arange(len(buf), dtype=torch.int16, device="cuda")       # tag every ring row with its index
    loader = buf.sample(50, seed=4)
    assert loader.route == "kernel" and loader.indices.is_cuda and loader.indices.numel() == len(buf)
    twin = golden_buffer(RP, key, "cuda", cls=RP.SampledReplayTensors)
    assert torch.equal(twin.sample(50, seed=4).indices, loader.indices)
    assert not torch.equal(twin.sample(50, seed=4).indices, loader.indices) and twin.sample_calls == 2
    sampled = np.sort(loader.indices.cpu().numpy())
    assert sampled.min() >= 0 and sampled.max() < len(buf)
    epochs = []
    for _ in range(2):
        seen = []
        for batch in loader:
            rows = batch[4][:len(batch[4]) // S, 0].long()
            assert differences(batch_arrays(batch), batch_arrays(one_batch(buf, rows, "torch"))) == []
            seen.append(rows.cpu().numpy())
        seen = np.concatenate(seen)
        assert np.array_equal(np.sort(seen), sampled)
        epochs.append(seen)
    assert not np.array_equal(epochs[0], epochs[1])
    full = buf.sample(50, full_batches=True, seed=4)
    assert len(full) == len(buf) // 50 and all(b[0].shape[0] == S * 50 for b in full)
    assert RP.augmented(batch) is batch
