"""The host route into the replay-buffer tensors (`ReplayTensors.store_games` in src/replay.py) against the
reference's own `ReplayBuffer.store` (fixture G15, tests/golden/make_golden_replay.py), and the Python mirror of
az_replay_tensors against the size the header asserts.  No GPU."""
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
COLUMNS = ("state", "prob", "z", "steps", "aux", "root_wdl", "mask", "fut")
GOLDEN_CASES = {"c4": ("Connect4", ("g11_selfplay_plain_search", "g10_selfplay_numpy_rng")),
                "ot": ("Othello", ("g12_selfplay_othello",))}


@pytest.fixture(scope="module")
def SP():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    ge.build()
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src import selfplay
    return selfplay


@pytest.fixture(scope="module")
def RP(SP):
    from src import replay
    return replay


def fixture_games(name):
    """The games of a self-play fixture as drain() would return them - (winner, play_data, slot) - in the order
    (length, index): their (finishing ply, slot) order, since all start together without refill."""
    g = load(name)
    cols = [c for c in COLUMNS if f"g0_{c}" in g.files]
    games = []
    i = 0
    while f"g{i}_state" in g.files:
        arrs = [g[f"g{i}_{c}"] for c in cols]
        play = tuple(tuple(a[t] for a in arrs) for t in range(len(arrs[0])))
        games.append((int(g[f"g{i}_winner"][0]), play, i))
        i += 1
    return sorted(games, key=lambda t: (len(t[1]), t[2]))


def raw_bytes(a):
    """Any array as its bytes: floats compare as their bit patterns, booleans as 0 / 1."""
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1)


def buffer_arrays(buf):
    return {t: getattr(buf, t).cpu().numpy() for t in TENSORS}


def differences(got, expected):
    """Names of the tensors that differ in dtype, shape or any byte of any ring slot."""
    bad = []
    for t in TENSORS:
        a, b = got[t], expected[t]
        if a.dtype != b.dtype or a.shape != b.shape or not np.array_equal(raw_bytes(a), raw_bytes(b)):
            bad.append(t)
    return bad


def golden(key):
    g = load("g15_replay_buffer")
    return {t: g[f"{key}_{t}"] for t in TENSORS}, int(g[f"{key}_ptr"][0]), int(g[f"{key}_capacity"][0])


def naive_store(RP, game, capacity, games):
    """Row by row, one assignment per tuple and column: the ring rule spelled out."""
    buf = RP.ReplayTensors(game, capacity, "cpu")
    arr = buffer_arrays(buf)
    ptr = 0
    for _w, play, _s in games:
        for tup in play:
            i = ptr % capacity
            ptr += 1
            arr["state"][i] = tup[0]
            arr["prob"][i] = tup[1]
            arr["winner"][i] = int(tup[2])
            arr["steps_to_end"][i] = int(tup[3])
            arr["aux_target"][i] = int(tup[4])
            arr["root_wdl"][i] = tup[5]
            arr["valid_mask"][i] = tup[6]
            arr["future_root_wdl"][i] = tup[7] if len(tup) > 7 else 0
    return arr, ptr


@pytest.mark.parametrize("key", sorted(GOLDEN_CASES))
def test_store_games_equals_the_reference_buffer(RP, key):
    """1 + 6: every tensor, every ring slot, `_ptr`; and the comparison notices one flipped byte anywhere."""
    game, names = GOLDEN_CASES[key]
    expected, ptr, cap = golden(key)
    buf = RP.ReplayTensors(game, cap, "cpu")
    rows = sum(buf.store_games(fixture_games(n)) for n in names)
    assert rows == ptr > cap
    got = buffer_arrays(buf)
    assert differences(got, expected) == []
    assert buf._ptr == ptr and len(buf) == cap
    rng = np.random.default_rng(15)
    for t in TENSORS:
        broken = {k: v.copy() for k, v in expected.items()}
        flat = broken[t].view(np.uint8).reshape(-1)
        at = int(rng.integers(0, flat.size))
        flat[at] ^= 1
        assert differences(got, broken) == [t], (t, at)


def test_fresh_tensors_have_the_reference_layout(RP):
    import torch
    for game, (A, R, Cc) in (("Connect4", (7, 6, 7)), ("Othello", (65, 8, 8))):
        b = RP.ReplayTensors(game, 50, "cpu")
        want = dict(state=(torch.int8, (50, 3, R, Cc)), prob=(torch.float32, (50, A)), winner=(torch.int8, (50, 1)),
                    steps_to_end=(torch.int16, (50, 1)), aux_target=(torch.int16, (50, 1)), root_wdl=(torch.float32, (50, 3)),
                    valid_mask=(torch.bool, (50, A)), future_root_wdl=(torch.float32, (50, 3)))
        for t in TENSORS:
            x = getattr(b, t)
            assert (x.dtype, tuple(x.shape)) == want[t] and x.is_contiguous(), t
            assert bool((x == (1 if t == "valid_mask" else 0)).all()), t
        assert b._ptr == 0 and b.current_capacity == 50 and len(b) == 0
        out = b.get(torch.tensor([3, 4]))
        assert len(out) == 8 and out[0].dtype == torch.float32 and out[0].shape == (2, 3, R, Cc)
        assert not hasattr(b, "sample") and not hasattr(b, "save") and not hasattr(b, "replay_ratio")


def test_td_steps_zero_leaves_the_future_column_zero(RP):
    games = fixture_games("g11_selfplay_plain_search")                  # recorded with td_steps = 0: seven columns
    assert all(len(t) == 7 for _w, play, _s in games for t in play)
    buf = RP.ReplayTensors("Connect4", 97, "cpu")
    buf.future_root_wdl.fill_(7.0)                                       # whatever was there before
    buf.store_games(games)
    assert buf._ptr > 97 and not buf.future_root_wdl.any()


@pytest.mark.parametrize("game,name,capacity", [("Connect4", "g10_selfplay_numpy_rng", 61), ("Connect4", "g10_selfplay_numpy_rng", 19),
                                                ("Othello", "g12_selfplay_othello", 50)])
def test_more_rows_than_capacity_equals_one_by_one(RP, game, name, capacity):
    """One call with several times the ring's rows (capacity 19 and 50: less than ONE game's rows) against the
    same games stored one at a time, and against row-by-row assignment."""
    games = fixture_games(name)
    assert sum(len(p) for _w, p, _s in games) > 3 * capacity
    at_once = RP.ReplayTensors(game, capacity, "cpu")
    at_once.store_games(games)
    singly = RP.ReplayTensors(game, capacity, "cpu")
    for g in games:
        singly.store_games([g])
    naive, ptr = naive_store(RP, game, capacity, games)
    assert differences(buffer_arrays(at_once), naive) == [] and differences(buffer_arrays(singly), naive) == []
    assert at_once._ptr == singly._ptr == ptr


def test_tensor_struct_mirror_has_the_size_the_header_asserts(SP, RP):
    hdr = open(os.path.join(ROOT, "include", "az_mcts.h")).read()
    m = re.search(r"#define\s+AZ_REPLAY_TENSORS_BYTES\s+(\d+)", hdr)
    assert m and "sizeof(az_replay_tensors) == AZ_REPLAY_TENSORS_BYTES" in hdr
    assert C.sizeof(SP.ReplayTensorsC) == int(m.group(1)) == 8 * C.sizeof(C.c_void_p) + 8
    body = re.search(r"typedef struct az_replay_tensors \{(.*?)\} az_replay_tensors;", hdr, re.S).group(1)
    declared = re.findall(r"\b(\w+);", body)
    assert declared == [f[0] for f in SP.ReplayTensorsC._fields_] == list(TENSORS) + ["capacity"]
    assert tuple(RP.ReplayTensors.TENSORS) == TENSORS
    body = re.search(r"typedef struct az_selfplay_export_info \{(.*?)\} az_selfplay_export_info;", hdr, re.S).group(1)
    assert re.findall(r"\*?(\w+)[,;]", body) == [f[0] for f in SP.SelfPlayExportInfo._fields_]
