#!/usr/bin/env python3
"""Output bytes of every entry point of nn_conv.hip on fixed inputs: record them, or check a build against a record.

    python tools/record_conv_golden.py                    record tests/golden/g14_conv_block_bytes.npz with THIS tree's build
    python tools/record_conv_golden.py --check            run the same cases and compare with the record, byte for byte
    (--fixture PATH: another file)

The record is an oracle only when it comes from ANOTHER build than the one under test: it was made by running this script
in a checkout of the parent commit (the script copied into it), and tests/test_conv_slots_gpu.py holds every later build
to it.  Nothing here builds anything: the library of the tree the script lies in is loaded as it is.

Cases (every one for each entry point that include/az_nn.h declares for nn_conv.hip: az_nn_conv_block with c_in 64 and
the residual, c_in 64 without it, c_in 32; az_nn_stem_conv_block_positions; az_nn_stem_embed; az_nn_stem_embed_positions):

    group free   (no AZ_NN_CONV_GRID)  batch 1, 3, 4, 5      dead waves; a partial tile; one tile; one full + one partial
                                       batch 13, batch_dev 9  rows 9.. of y keep their NaN canary
                                       the three stem forms, gather list 9 of 13 with one index outside the rows
    group grid2  (AZ_NN_CONV_GRID=2)   batch 13              two tiles per workgroup, both raw buffers, the last tile partial
    group grid1  (AZ_NN_CONV_GRID=1)   batch 13              four tiles in one workgroup

AZ_NN_CONV_GRID is read once per process, so a capped group runs in a child process.  All inputs come from the seed
stored in the record (numpy only: no device arithmetic goes into an input), and the record keeps a SHA-256 of every
case's inputs, so a failure of the generator cannot pass for one of the kernels.  Outputs are kept whole for batch <= 5
and as SHA-256 digests for batch 13 (the file stays well under 1 MB).
"""
import argparse
import ctypes as C
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
FIXTURE = os.path.join(ROOT, "tests", "golden", "g14_conv_block_bytes.npz")
SEED = 1814
CELLS = 42
ENTRIES = ("conv64_res", "conv64_nores", "conv32", "stem_conv", "stem_embed", "stem_embed_positions")
STEM_ENTRIES = ENTRIES[3:]
GROUPS = {"free": None, "grid2": "2", "grid1": "1"}
WHOLE_UP_TO = 5                                     # outputs of larger batches are stored as digests


def case_names(group):
    if group == "free":
        names = ["free/%s/b%d" % (e, b) for b in (1, 3, 4, 5) for e in ENTRIES]
        names += ["free/%s/b13n9" % e for e in ENTRIES]
        names += ["free/%s/b13g9" % e for e in STEM_ENTRIES]
        return names
    return ["%s/%s/b13" % (group, e) for e in ENTRIES]


def all_case_names():
    return [n for g in GROUPS for n in case_names(g)]


def _bf16(a):
    """float32 -> bf16 bits (truncated: any bit pattern will do for an input)"""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _wins(bb):
    for d in (1, 7, 6, 8):
        m = bb & (bb >> d)
        if m & (m >> (2 * d)):
            return True
    return False


def positions(rng, n):
    """n random legal positions of all ages (games stop at a win; bit = 7 * column + height), both sides to move, both
    symmetry ids, and the relative feature planes (n, 3, 6, 7) that show them (row 0 on top, columns mirrored under id 1)"""
    p1, p2 = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
    turn, sym = np.zeros(n, dtype=np.int32), rng.integers(0, 2, n).astype(np.int32)
    feat = np.zeros((n, 3, 6, 7), dtype=np.float32)
    for k in range(n):
        bb, height, ply = [0, 0], [0] * 7, 0
        for ply in range(int(rng.integers(0, 43))):
            cols = [c for c in range(7) if height[c] < 6]
            if not cols:
                break
            c = cols[int(rng.integers(0, len(cols)))]
            bb[ply & 1] |= 1 << (7 * c + height[c])
            height[c] += 1
            if _wins(bb[ply & 1]):
                ply += 1
                break
        else:
            ply = sum(height)
        ply = sum(height)
        p1[k], p2[k] = bb[0], bb[1]
        turn[k] = 1 if ply % 2 == 0 else -1
        own, opp = (bb[0], bb[1]) if turn[k] > 0 else (bb[1], bb[0])
        for r in range(6):
            for c in range(7):
                bit = (6 - c if sym[k] else c) * 7 + (5 - r)
                feat[k, 0, r, c] = (own >> bit) & 1
                feat[k, 1, r, c] = (opp >> bit) & 1
        feat[k, 2] = 1.0
    return p1, p2, turn, sym, feat


def make_inputs(name):
    """every host array of one case, from SEED and the case's name alone"""
    group, entry, shape = name.split("/")
    batch = int(shape[1:].split("n")[0].split("g")[0])
    rng = np.random.default_rng([SEED, sum(name.encode()), len(name), batch])
    cin = 32 if entry in ("conv32", "stem_embed", "stem_embed_positions") else 64
    d = {"w": _bf16(rng.standard_normal((64, 3, 3, cin)) * 0.06), "bias": _bf16(rng.standard_normal(64) * 0.1)}
    if cin == 64:
        d["gamma"] = _bf16(1.0 + 0.3 * rng.standard_normal(64))
        d["beta"] = _bf16(0.2 * rng.standard_normal(64))
    if entry.startswith("conv"):
        x = rng.standard_normal((batch, CELLS, cin)).astype(np.float32)
        for b in range(batch):
            if b % 5 == 2:
                x[b] = 0.0                                      # an all-zero sample: variance 0
            if b % 4 == 1:
                x[b, 7, 3], x[b, 40, cin - 1] = 3e18, -2e17     # entries of large magnitude
        d["x"] = _bf16(x)
    else:
        d["p1"], d["p2"], d["turn"], d["sym"], d["features"] = positions(rng, batch)
        if entry == "stem_conv":
            d["frag"] = _bf16(rng.standard_normal((2, 4, 64, 8)) * 0.25)
            pmap = np.zeros((48, 68), dtype=np.float32)
            pmap[:CELLS, :64] = rng.standard_normal((CELLS, 64))
            d["pmap"] = pmap
        else:
            d["emb_own"], d["emb_opp"] = _bf16(rng.standard_normal(32)), _bf16(rng.standard_normal(32))
            d["pos"] = _bf16(rng.standard_normal((CELLS, 32)))
    if "n" in shape or "g" in shape:
        d["live"] = np.array([9], dtype=np.int64)
    if "g" in shape:
        rows = rng.permutation(batch).astype(np.int32)
        rows[4] = batch + 3                                     # outside the rows: shows row 0
        rows[9:] = 2 ** 31 - 1                                  # behind the list: never read
        d["rows"] = rows
    return d


def digest(arrays):
    h = hashlib.sha256()
    for k in sorted(arrays):
        h.update(k.encode())
        h.update(np.ascontiguousarray(arrays[k]).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


def run_case(torch, L, Positions, name):
    """(digest of the inputs, y as uint16 (batch, 42, 64)) of one case on the current device"""
    entry = name.split("/")[1]
    host = make_inputs(name)
    dev = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int16) if v.dtype == np.uint16 else v).cuda()
           for k, v in host.items()}
    ptr = lambda k: dev[k].data_ptr() if k in dev else None
    batch = len(host["x"]) if "x" in host else len(host["p1"])
    y = torch.full((batch, CELLS, 64), float("nan"), dtype=torch.bfloat16, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if entry.startswith("conv"):
        cin = 32 if entry == "conv32" else 64
        rc = L.az_nn_conv_block(ptr("x"), cin, ptr("w"), ptr("bias"), ptr("gamma"), ptr("beta"), 1 if entry == "conv64_res" else 0,
                                y.data_ptr(), batch, 1e-5, ptr("live"), s)
    else:
        pos = Positions(ptr("p1"), ptr("p2"), ptr("turn"), ptr("sym"))
        if entry == "stem_conv":
            rc = L.az_nn_stem_conv_block_positions(C.byref(pos), ptr("frag"), ptr("pmap"), ptr("w"), ptr("bias"), ptr("gamma"),
                                                   ptr("beta"), y.data_ptr(), batch, 1e-5, ptr("rows"), ptr("live"), s)
        elif entry == "stem_embed":
            rc = L.az_nn_stem_embed(ptr("features"), ptr("emb_own"), ptr("emb_opp"), ptr("pos"), ptr("w"), ptr("bias"),
                                    y.data_ptr(), batch, ptr("rows"), ptr("live"), s)
        else:
            rc = L.az_nn_stem_embed_positions(C.byref(pos), ptr("emb_own"), ptr("emb_opp"), ptr("pos"), ptr("w"), ptr("bias"),
                                              y.data_ptr(), batch, ptr("rows"), ptr("live"), s)
    assert rc == 0, (name, rc)
    torch.cuda.synchronize()
    return digest(host), y.view(torch.int16).cpu().numpy().view(np.uint16)


def run_group(group):
    """name -> (input digest, output) for the cases of one group, IN THIS PROCESS (whose AZ_NN_CONV_GRID must be the group's)"""
    assert os.environ.get("AZ_NN_CONV_GRID") == GROUPS[group], "group %s needs AZ_NN_CONV_GRID=%s" % (group, GROUPS[group])
    import torch  # (before the engine library: one HIP runtime per process)
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    from src.fast_net import Positions, glue
    L = glue()
    assert L is not None, "no library in " + PKG
    return {n: run_case(torch, L, Positions, n) for n in case_names(group)}


def run_group_in_child(group, timeout=300):
    env = {k: v for k, v in os.environ.items() if k != "AZ_NN_CONV_GRID"}
    if GROUPS[group] is not None:
        env["AZ_NN_CONV_GRID"] = GROUPS[group]
    with tempfile.TemporaryDirectory() as tmp:
        raw = os.path.join(tmp, "raw.npz")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--group", group, "--raw", raw], env=env,
                           capture_output=True, text=True, timeout=timeout)
        assert r.returncode == 0, r.stderr[-3000:]
        with np.load(raw) as z:
            return {n: (z["in/" + n], z["out/" + n]) for n in case_names(group)}


def stored(out):
    """what the record keeps of an output: the array itself up to WHOLE_UP_TO samples, else its SHA-256"""
    return out if len(out) <= WHOLE_UP_TO else digest({"y": out})


def compare(results, fixture):
    """the names of the cases whose inputs or outputs are not the record's"""
    bad = []
    with np.load(fixture) as z:
        assert int(z["seed"]) == SEED
        for n in all_case_names():
            if n not in results:
                continue
            ins, out = results[n]
            if not np.array_equal(z["in/" + n], ins):
                bad.append(n + " (inputs)")
            elif not np.array_equal(z["out/" + n], stored(out)):
                bad.append(n)
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--fixture", default=FIXTURE)
    ap.add_argument("--group", choices=list(GROUPS))
    ap.add_argument("--raw")
    a = ap.parse_args()
    if a.group:                                                     # the child of run_group_in_child
        res = run_group(a.group)
        np.savez(a.raw, **{"in/" + n: v[0] for n, v in res.items()}, **{"out/" + n: v[1] for n, v in res.items()})
        return 0
    results = {}
    for g in GROUPS:
        results.update(run_group_in_child(g))
    if a.check:
        bad = compare(results, a.fixture)
        print("%d cases against %s: %s" % (len(results), a.fixture, "all equal" if not bad else "DIFFERENT: " + ", ".join(bad)))
        return 1 if bad else 0
    os.makedirs(os.path.dirname(os.path.abspath(a.fixture)), exist_ok=True)
    np.savez_compressed(a.fixture, seed=np.int64(SEED), **{"in/" + n: v[0] for n, v in results.items()},
                        **{"out/" + n: stored(v[1]) for n, v in results.items()})
    print("recorded %d cases from %s to %s (%d bytes)" % (len(results), PKG, a.fixture, os.path.getsize(a.fixture)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
