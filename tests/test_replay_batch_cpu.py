"""Augmented training batches out of the replay tensors, the parts that need no GPU (`ReplayTensors.batches`,
`SampledReplayTensors.sample`, `ReplayBatches`, `augmented` in src/replay.py) against what the reference's own
`get` + `augment` and `sample` gave (fixture G16, tests/golden/make_golden_batch.py), bit for bit; and the Python
mirror of az_replay_batch against the size the header asserts.

The reference itself is never imported here: the golden file stands for it."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from test_oracle_golden import load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
TENSORS = ("state", "prob", "winner", "steps_to_end", "aux_target", "root_wdl", "valid_mask", "future_root_wdl")
GAMES = {"c4": "Connect4", "ot": "Othello"}
GEOMETRY = {"Connect4": (7, 6, 7, 2), "Othello": (65, 8, 8, 4)}          # actions, rows, columns, symmetries


@pytest.fixture(scope="module")
def RP():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src import replay
    return replay


def raw_bytes(a):
    """Any array as its bytes: floats compare as their bit patterns, booleans as 0 / 1."""
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def golden_buffer(RP, key, device="cpu", cls=None):
    """A buffer (ReplayTensors unless `cls`) holding fixture G15's tensors of game `key`."""
    import torch
    g = load("g15_replay_buffer")
    buf = (cls or RP.ReplayTensors)(GAMES[key], int(g[f"{key}_capacity"][0]), device)
    for t in TENSORS:
        getattr(buf, t).copy_(torch.from_numpy(g[f"{key}_{t}"]))
    buf._ptr = int(g[f"{key}_ptr"][0])
    return buf


def golden_batch(key):
    g = load("g16_training_batch")
    return g[f"{key}_idx"], {t: g[f"{key}_{t}"] for t in TENSORS}


def batch_arrays(batch):
    assert len(batch) == len(TENSORS)
    return {t: x.cpu().numpy() for t, x in zip(TENSORS, batch)}


def differences(got, expected):
    """Names of the tensors that differ in dtype, shape or any byte."""
    return [t for t in TENSORS if got[t].dtype != expected[t].dtype or got[t].shape != expected[t].shape or
            not np.array_equal(raw_bytes(got[t]), raw_bytes(expected[t]))]


def reassembled(batches, S):
    """Batches of one pass -> the arrays of ONE batch over all their samples: every batch is S blocks of its own
    size, block s of the whole is the batches' blocks s one after the other."""
    parts = [batch_arrays(b) for b in batches]
    out = {}
    for t in TENSORS:
        blocks = []
        for s in range(S):
            for p in parts:
                n = p[t].shape[0] // S
                assert n * S == p[t].shape[0]
                blocks.append(p[t][s * n:(s + 1) * n])
        out[t] = np.concatenate(blocks)
    return out


def check_shapes(RP, game, batch, n):
    import torch
    A, R, Cc, S = GEOMETRY[game]
    want = [(torch.float32, (S * n, 3, R, Cc)), (torch.float32, (S * n, A)), (torch.int8, (S * n, 1)), (torch.int16, (S * n, 1)),
            (torch.int16, (S * n, 1)), (torch.float32, (S * n, 3)), (torch.bool, (S * n, A)), (torch.float32, (S * n, 3))]
    assert [(x.dtype, tuple(x.shape)) for x in batch] == want


# ------------------------------------------------------------------------------------------ 1. rows

@pytest.mark.parametrize("key", sorted(GAMES))
def test_torch_route_equals_the_reference_batch(RP, key):
    game = GAMES[key]
    buf = golden_buffer(RP, key)
    idx, expected = golden_batch(key)
    S = GEOMETRY[game][3]
    whole = list(buf.batches(idx, len(idx), route="torch"))
    assert len(whole) == 1
    check_shapes(RP, game, whole[0], len(idx))
    assert differences(batch_arrays(whole[0]), expected) == []
    # the default route on the CPU is the torch route
    assert differences(batch_arrays(next(iter(buf.batches(idx, len(idx))))), expected) == []
    # the comparison notices one flipped byte anywhere
    rng = np.random.default_rng(16)
    got = batch_arrays(whole[0])
    for t in TENSORS:
        broken = {k: v.copy() for k, v in expected.items()}
        flat = broken[t].view(np.uint8).reshape(-1)
        flat[int(rng.integers(0, flat.size))] ^= 1
        assert differences(got, broken) == [t]
    for size in (7, 10, 31):
        loader = buf.batches(idx, size, route="torch")
        parts = list(loader)
        short = len(idx) % size
        assert short and len(parts) == len(loader) == len(idx) // size + 1
        for p in parts[:-1]:
            check_shapes(RP, game, p, size)
        check_shapes(RP, game, parts[-1], short)
        assert differences(reassembled(parts, S), expected) == []
        dropped = buf.batches(idx, size, route="torch", drop_last=True)
        kept = list(dropped)
        assert len(kept) == len(dropped) == len(idx) // size
        n = len(kept) * size
        cut = {t: np.concatenate([expected[t][s * len(idx):s * len(idx) + n] for s in range(S)]) for t in TENSORS}
        assert differences(reassembled(kept, S), cut) == []


@pytest.mark.parametrize("key", sorted(GAMES))
def test_order_names_positions_of_the_sample(RP, key):
    game = GAMES[key]
    buf = golden_buffer(RP, key)
    idx, expected = golden_batch(key)
    S, n = GEOMETRY[game][3], len(idx)
    order = np.random.default_rng(3).permutation(n)
    got = reassembled(list(buf.batches(idx, 9, order=order, route="torch")), S)
    want = {t: np.concatenate([expected[t][s * n:(s + 1) * n][order] for s in range(S)]) for t in TENSORS}
    assert differences(got, want) == []
    with pytest.raises(ValueError):
        buf.batches(idx, 9, order=order[:-1], route="torch")
    with pytest.raises(ValueError):
        buf.batches(idx, 9, order=np.arange(1, n + 1), route="torch")
    with pytest.raises(ValueError):
        buf.batches(idx, 0, route="torch")
    with pytest.raises(ValueError):
        buf.batches(idx, 9, route="kernel")                             # no GPU under this buffer
    with pytest.raises(ValueError):
        buf.batches(idx, 9, route="eager")


def test_the_fixture_holds_the_rows_it_promises():
    g15, g16 = load("g15_replay_buffer"), load("g16_training_batch")
    for key, n in (("c4", 64), ("ot", 48)):
        idx = g16[f"{key}_idx"]
        cap = int(g15[f"{key}_capacity"][0])
        prob, mask = g15[f"{key}_prob"][idx], g15[f"{key}_valid_mask"][idx]
        assert len(idx) == n and 0 in idx and cap - 1 in idx and len(np.unique(idx)) < n
        assert ((prob == 0).all(1) & mask.all(1)).sum() >= 2
        turn = g15[f"{key}_state"][idx, 2, 0, 0]
        assert (turn > 0).any() and (turn < 0).any()
        assert (g15[f"{key}_future_root_wdl"][idx] != 0).any()
        if key == "ot":
            assert (mask[:, 64] & ~mask.all(1)).any()


def test_augmented_is_the_identity(RP):
    batch = tuple(object() for _ in range(8))
    assert RP.augmented(batch) is batch


# ------------------------------------------------------------------------------------------ 2. sample sizes

def test_sample_sizes_equal_the_reference(RP):
    g = load("g16_training_batch")
    cases, sizes = g["sample_cases"], g["sample_sizes"]
    assert len(cases) == len(sizes) >= 40
    assert {0.25, 0.025} == set(cases[:, 2].tolist()) and {0, 1} == set(cases[:, 4].astype(int).tolist())
    for (length, capacity, ratio, batch, full), (n_rows, n_batches) in zip(cases.tolist(), sizes.tolist()):
        length, capacity, batch, full = int(length), int(capacity), int(batch), bool(int(full))
        assert RP.sample_size(length, batch, full, ratio) == n_rows, (length, ratio, batch, full)
        buf = RP.SampledReplayTensors("Connect4", capacity, "cpu")
        buf._ptr = length
        loader = buf.sample(batch, full_batches=full, replay_ratio=ratio, seed=5)
        assert (loader.indices.numel(), len(loader)) == (n_rows, n_batches), (length, capacity, ratio, batch, full)
        lo, hi = int(loader.indices.min()), int(loader.indices.max())
        assert 0 <= lo and hi < length


def test_sample_is_seeded_and_counts_its_calls(RP):
    import torch
    a, b = golden_buffer(RP, "c4", cls=RP.SampledReplayTensors), golden_buffer(RP, "c4", cls=RP.SampledReplayTensors)
    first_a, first_b = a.sample(32, seed=9), b.sample(32, seed=9)
    assert first_a.indices.dtype == torch.int64 and first_a.indices.numel() == len(a) == 389
    assert torch.equal(first_a.indices, first_b.indices)
    second = a.sample(32, seed=9)
    assert a.sample_calls == 2 and not torch.equal(second.indices, first_a.indices)
    assert not torch.equal(b.sample(32, seed=10).indices, second.indices)
    assert len(np.unique(first_a.indices.numpy())) > 200                # a draw, not a constant
    with pytest.raises(ValueError):
        a.sample(0, full_batches=True)
    with pytest.raises(ValueError):
        a.sample(-3, full_batches=True)
    with pytest.raises(AssertionError):
        RP.SampledReplayTensors("Connect4", 50, "cpu").sample(8)       # nothing stored yet


# ------------------------------------------------------------------------------------------ 3. epochs

@pytest.mark.parametrize("key", sorted(GAMES))
def test_epochs_cover_the_sample_once_each_in_different_orders(RP, key):
    import torch
    game = GAMES[key]
    buf = golden_buffer(RP, key, cls=RP.SampledReplayTensors)
    buf.aux_target[:, 0] = torch.arange(len(buf), dtype=torch.int16)     # tag every ring row with its index
    loader = buf.sample(50, seed=2)
    n, S = loader.indices.numel(), GEOMETRY[game][3]
    assert n == len(buf) and len(loader) == (n + 49) // 50
    sampled = np.sort(loader.indices.numpy())
    epochs = []
    for _ in range(2):
        seen = []
        for batch in loader:
            rows = batch[4][:, 0].numpy()
            m = len(rows) // S
            for s in range(1, S):                                        # symmetry-major blocks of the same samples
                assert np.array_equal(rows[:m], rows[s * m:(s + 1) * m])
            seen.append(rows[:m])
        seen = np.concatenate(seen)
        assert len(seen) == n and np.array_equal(np.sort(seen), sampled)   # every sampled position exactly once
        epochs.append(seen)
    assert not np.array_equal(epochs[0], epochs[1])
    full = buf.sample(50, full_batches=True, seed=2)
    assert len(full) == full.indices.numel() // 50 and all(b[0].shape[0] == S * 50 for b in full)


# ------------------------------------------------------------------------------------------ 4. the header

def test_batch_struct_mirror_has_the_size_the_header_asserts(RP):
    hdr = open(os.path.join(ROOT, "include", "az_mcts.h")).read()
    m = re.search(r"#define\s+AZ_REPLAY_BATCH_BYTES\s+(\d+)", hdr)
    assert m and "sizeof(az_replay_batch) == AZ_REPLAY_BATCH_BYTES" in hdr
    assert C.sizeof(RP.ReplayBatchC) == int(m.group(1)) == 8 * C.sizeof(C.c_void_p)
    body = re.search(r"typedef struct az_replay_batch \{(.*?)\} az_replay_batch;", hdr, re.S).group(1)
    assert re.findall(r"\b(\w+);", body) == [f[0] for f in RP.ReplayBatchC._fields_] == list(TENSORS)
    for name in ("az_game_num_augment", "az_replay_dev_batch", "az_replay_dev_sample_indices"):
        assert re.search(r"\bint\s+%s\(" % name, hdr), name
