#!/usr/bin/env python3
"""Output bytes of the attention / heads kernels (nn_attn.hip, nn_attn_heads.hip, nn_heads.hip) and of the model object
on fixed inputs: record them, or check a build against a record.

    python tools/record_attn_golden.py                    record tests/golden/g19_attn_bytes.npz with THIS tree's build
    python tools/record_attn_golden.py --check            run the same cases and compare with the record, byte for byte
    (--fixture PATH: another file)

The record is an oracle only when it comes from ANOTHER build than the one under test: it was made by running this script
in a checkout of the commit before the kernels' earlier forms were removed (EXPERIMENTS.md E20; the script copied into
it), and tests/test_attn_bytes_gpu.py holds every later build to it.  At that commit az_nn_debug bit 8 selected the earlier
forms at launch time; record mode runs every case with the bit clear and with it set and refuses to write unless the two
agree, so the record is the bytes of both.  (The bit is unused since: there the second run repeats the first.)  Nothing
here builds anything: the library of the tree the script lies in is loaded as it is.

Cases (name = entry/weights/inputs/grid cap/mask/q-norm; every one with soft and with sharp q-norm weights unless noted):

    heads   az_nn_attn_heads   w1 plain    b1 12 13 25 192 193 401 in one workgroup (cap 1), b777 b4099 free; mask, none
                               w1 compact  (batch, live, cap) 9/5/0  401/260/1  401/260/1 stray  9/9/0 stray  9/5/0 stray:
                                           shuffled output rows, NaN in every sample past `live`, stray = indices -1, B,
                                           B + 7, 2^31 - 1, -2^31 in the list
                               w2 extreme  b1 2 3 25 with cap 0 and 1, mask and none; b205 (12 x 17 + 1) cap 1;
                                           b40 live 25 compact
    block   az_nn_attn_block   w1 plain b1 3 50; w2 extreme b1 2 3 25
    pair    az_nn_heads        w1 plain b1 2 3 9, soft only
    heads, block               w2 plain b25, soft only, eps 1e-40 and 0: below FLT_MIN, the rsqrtf() instantiation.  At eps 0
                               NaN is expected (1 / sqrt(0) x 0 in the padding tokens): every NaN is stored and compared
                               as the one quiet NaN
                               (with these inputs all 275 values of the heads case are NaN: it pins no more than
                               that; the block case's digest carries the arithmetic)
    model   az_nn_model_forward on the planes of g7_network, az_nn_model_forward_positions on 3000 positions; w1, soft

w1 = tests/golden/g7_checkpoint_weights; w2 = every parameter drawn here (matrices N(0, 1 / fan_in), norm weights 1 +
N(0, 0.25^2), the rest N(0, 0.1^2)); sharp = q-norm weight x 40: scores outside the bound, the max-subtracting softmax.
plain = N(0, 1.5^2); extreme = about one token row in eight exactly zero and one in eight +-1e18 x [0.5, 1), a whole
zero sample.  Every output array is prefilled with NaN, and the prefill is part of the compared bytes.

All inputs come from the seed stored in the record (numpy only: no device arithmetic and no torch generator goes into an
input or a weight), and the record keeps a SHA-256 of every case's inputs - the weights as the twin holds them on the
device included - so a failure of the generator cannot pass for one of the kernels.  Outputs are kept whole up to 16 KB
and as SHA-256 digests above (the file stays well under 1 MB).
"""
import argparse
import ctypes as C
import functools
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "alphazero-al_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "g19_attn_bytes.npz")
SEED = 1919
CELLS, C_DIM = 42, 64
WHOLE_UP_TO = 16 * 1024                             # bytes: larger outputs are stored as digests
BIT8 = 1 << 8                                       # az_nn_debug: the earlier forms, at the recorded commit


def _cases():
    """name -> dict(entry, w, kind, B, cap, mask, sharp, live, stray, eps)"""
    out = {}

    def add(entry, w, kind, B, cap=0, mask=True, sharps=(False, True), live=None, stray=False, eps=1e-5):
        for sharp in sharps:
            shape = "b%d" % B + ("" if live is None else "l%d" % live) + ("s" if stray else "")
            name = "/".join([entry, w, kind, shape, "cap%d" % cap, "mask" if mask else "nomask", "sharp" if sharp else "soft"])
            if eps != 1e-5:
                name += "/eps%g" % eps
            out[name] = dict(entry=entry, w=w, kind=kind, B=B, cap=cap, mask=mask, sharp=sharp, live=live, stray=stray, eps=eps)

    for B in (1, 12, 13, 25, 192, 193, 401, 777, 4099):
        for mask in (True, False):
            add("heads", "w1", "plain", B, cap=1 if B <= 401 else 0, mask=mask)
    for B, live, cap, stray in ((9, 5, 0, False), (401, 260, 1, False), (401, 260, 1, True), (9, 9, 0, True), (9, 5, 0, True)):
        add("heads", "w1", "plain", B, cap=cap, live=live, stray=stray)
    for B in (1, 2, 3, 25):
        for cap in (0, 1):
            for mask in (True, False):
                add("heads", "w2", "extreme", B, cap=cap, mask=mask)
    add("heads", "w2", "extreme", 12 * 17 + 1, cap=1)
    add("heads", "w2", "extreme", 40, live=25)
    for B in (1, 3, 50):
        add("block", "w1", "plain", B, mask=False)
    for B in (1, 2, 3, 25):
        add("block", "w2", "extreme", B, mask=False)
    for B in (1, 2, 3, 9):
        add("pair", "w1", "plain", B, sharps=(False,))
    for eps in (1e-40, 0.0):
        add("heads", "w2", "plain", 25, sharps=(False,), eps=eps)
        add("block", "w2", "plain", 25, mask=False, sharps=(False,), eps=eps)
    add("model", "w1", "planes", 0, sharps=(False,))
    add("model", "w1", "positions", 3000, sharps=(False,))
    return out


CASES = _cases()


def all_case_names():
    return list(CASES)


def _bf16(a):
    """float32 -> bf16 bits (truncated: any bit pattern will do for an input)"""
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


@functools.lru_cache(maxsize=2)
def _activations(kind, B, live, stray):
    """x (B, 42, 64) bf16 bits, mask (B, 7) uint8 with column 3 open, and for a compact case the row list and its count.
    One draw per (kind, B, live, stray): the cases that differ in weights, cap or mask only share it."""
    rng = _rng(kind == "extreme", B, live or 0, stray)
    x = (rng.standard_normal((B, CELLS, C_DIM)) * 1.5).astype(np.float32)
    if kind == "extreme":
        tag = rng.integers(0, 8, (B, CELLS))
        tag[0, 0], tag[0, 1], tag[0, 40], tag[0, 41] = 0, 1, 1, 0       # both kinds in the first and the last token tile
        big = ((rng.random(x.shape) * 0.5 + 0.5) * 1e18 * np.where(rng.random(x.shape) < 0.5, -1.0, 1.0)).astype(np.float32)
        x = np.where((tag == 1)[..., None], big, x)
        x = np.where((tag == 0)[..., None], np.float32(0.0), x)
        if B > 1:
            x[1] = 0.0
    d = {"x": _bf16(x)}
    mask = rng.random((B, 7)) > 0.25
    mask[:, 3] = True
    d["mask"] = mask.astype(np.uint8)
    if live is not None:
        d["x"][live:] = 0x7FC0                                          # NaN past the device-side count
        rows = rng.permutation(B).astype(np.int32)
        if stray:
            bad = np.array([-1, B, B + 7, 2 ** 31 - 1, -2 ** 31], dtype=np.int64).astype(np.int32)
            at = np.arange(0, live, max(1, live // len(bad)))[:len(bad)]
            rows[at] = bad[:len(at)]
        d["rows"], d["n_rows"] = rows, np.array([live], dtype=np.int64)
    return d


def listed_rows(name):
    """compact case: bool (B,), the output rows its list names inside the batch, and how many strays the list holds"""
    c = CASES[name]
    d = _activations(c["kind"], c["B"], c["live"], c["stray"])
    named = d["rows"][:c["live"]].astype(np.int64)
    inside = (named >= 0) & (named < c["B"])
    listed = np.zeros(c["B"], dtype=bool)
    listed[named[inside]] = True
    return listed, int((~inside).sum())


def _model_inputs(kind):
    if kind == "planes":            # about 3000 feature planes from the positions of g7_network
        g = np.load(os.path.join(GOLDEN, "g7_network.npz"))
        boards, turns = g["boards"], g["turns"]
        planes = np.stack([(boards == turns[:, None, None]), (boards == -turns[:, None, None]),
                           np.ones_like(boards) * turns[:, None, None]], 1).astype(np.float32)
        reps = -(-3000 // len(planes))
        return {"features": np.ascontiguousarray(np.concatenate([planes] * reps)),
                "mask": np.ascontiguousarray(np.concatenate([(boards[:, 0, :] == 0)] * reps).astype(np.uint8))}
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from test_stem_conv_gpu import _positions
    p1, p2, turn, sym, mask = _positions(np.random.default_rng(31), 3000)
    return {"p1": p1.view(np.int64), "p2": p2.view(np.int64), "turn": turn, "sym": sym, "mask": mask}


def digest(arrays):
    h = hashlib.sha256()
    for k in sorted(arrays):
        h.update(k.encode())
        h.update(np.ascontiguousarray(arrays[k]).tobytes())
    return np.frombuffer(h.digest(), dtype=np.uint8).copy()


class Runner:
    """the library, the two weight sets as device twins (soft and sharp), and run(name)"""

    def __init__(self):
        import torch  # (before the engine library: one HIP runtime per process)
        if PKG not in sys.path:
            sys.path.insert(0, PKG)
        from src import az_net
        from src.fast_net import FastConnect4Net, Positions, glue
        self.torch, self.Positions, self.L = torch, Positions, glue()
        assert self.L is not None, "no library in " + PKG
        self.twins, self.wdigest = {}, {}
        for w in ("w1", "w2"):
            net = az_net.Connect4Net(device="cuda").eval()
            if w == "w1":
                wts = np.load(os.path.join(GOLDEN, "g7_checkpoint_weights.npz"))
                az_net.load_reference_weights(net, {k: wts[k] for k in wts.files})
            else:
                rng = _rng(2)
                with torch.no_grad():
                    for pname, p in net.named_parameters():
                        v = rng.standard_normal(tuple(p.shape)).astype(np.float32)
                        if p.dim() >= 2:
                            v = v / np.float32(p[0].numel()) ** np.float32(0.5)
                        elif "norm" in pname and pname.endswith("weight"):
                            v = np.float32(1.0) + np.float32(0.25) * v
                        else:
                            v = np.float32(0.1) * v
                        p.copy_(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)))
            for sharp in (False, True):
                fast = FastConnect4Net.from_module(net)
                if sharp:
                    fast.qn_w = (fast.qn_w.float() * 40.0).to(fast.qn_w.dtype).contiguous()
                self.twins[w, sharp] = fast
                self.wdigest[w, sharp] = digest({k: (b.view(torch.int16) if b.dtype == torch.bfloat16 else b).cpu().numpy()
                                                 for k, b in fast.named_buffers()})

    def _launch(self, c, fast, dev, out):
        L, ptr = self.L, lambda k: dev[k].data_ptr() if k in dev else None
        s = C.c_void_p(self.torch.cuda.current_stream().cuda_stream)
        att = (ptr("x"), fast.pre_w.data_ptr(), fast.qkvg_w.data_ptr(), fast.qn_w.data_ptr(),
               fast.kn_w.data_ptr(), fast.o_w.data_ptr())
        o3 = [t.data_ptr() for t in out]
        if c["entry"] == "heads":
            return L.az_nn_attn_heads(*att, C.byref(fast._heads_w), ptr("mask"), *o3, c["B"], c["eps"], ptr("rows"), ptr("n_rows"), s)
        if c["entry"] == "block":
            return L.az_nn_attn_block(*att, o3[0], c["B"], c["eps"], None, s)
        if c["entry"] == "pair":
            return L.az_nn_heads(ptr("x"), C.byref(fast._heads_w), ptr("mask"), *o3, c["B"], c["eps"], None, None, s)
        model, B = fast.native_model(), len(dev["mask"])
        nb = int(L.az_nn_model_scratch_bytes(model, B))
        scratch = self.torch.empty(nb, dtype=self.torch.uint8, device="cuda")
        if c["kind"] == "planes":
            return L.az_nn_model_forward(model, ptr("features"), ptr("mask"), *o3, B, None, None, scratch.data_ptr(), nb, s)
        pos = self.Positions(ptr("p1"), ptr("p2"), ptr("turn"), ptr("sym"))
        return L.az_nn_model_forward_positions(model, C.byref(pos), ptr("mask"), *o3, B, None, None, scratch.data_ptr(), nb, s)

    def run(self, name, flags=0):
        """(digest of the inputs, output) of one case: uint32 (B, 11) = probs | wdl | moves left, or uint16 (B, 42, 64) = y"""
        torch, c = self.torch, CASES[name]
        host = dict(_model_inputs(c["kind"]) if c["entry"] == "model" else _activations(c["kind"], c["B"], c["live"], c["stray"]))
        if not c["mask"]:
            del host["mask"]
        fast = self.twins[c["w"], c["sharp"]]
        dev = {k: torch.from_numpy(v.view(np.int16) if v.dtype == np.uint16 else v).cuda() for k, v in host.items()}
        B = len(host["mask"]) if c["entry"] == "model" else c["B"]
        if c["entry"] == "block":
            out = [torch.full((B, CELLS, C_DIM), float("nan"), dtype=torch.bfloat16, device="cuda")]
        else:
            out = [torch.full(shape, float("nan"), device="cuda") for shape in ((B, 7), (B, 3), (B, 1))]
        before = self.L.az_nn_debug_flags()
        self.L.az_nn_debug(flags | (c["cap"] & 0xfff) << 16)            # bits 16-27: a cap on az_nn_attn_heads' grid
        try:
            rc = self._launch(c, fast, dev, out)
            torch.cuda.synchronize()
        finally:
            self.L.az_nn_debug(before)
        assert rc == 0, (name, rc)
        if c["entry"] == "block":
            res = out[0].view(torch.int16).cpu().numpy().view(np.uint16)
            if c["eps"] == 0.0:
                res[(res & 0x7FFF) > 0x7F80] = 0x7FC0
        else:
            res = torch.cat(out, 1).contiguous().view(torch.int32).cpu().numpy().view(np.uint32)
            if c["eps"] == 0.0:
                res[np.isnan(res.view(np.float32))] = 0x7FC00000
        host["weights"] = self.wdigest[c["w"], c["sharp"]]
        host["case"] = np.frombuffer(name.encode(), dtype=np.uint8)
        return digest(host), res


def stored(out):
    """what the record keeps of an output: the array itself up to WHOLE_UP_TO bytes, else its SHA-256"""
    return out if out.nbytes <= WHOLE_UP_TO else digest({"y": out})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--fixture", default=FIXTURE)
    a = ap.parse_args()
    R = Runner()
    results = {n: R.run(n) for n in CASES}
    if a.check:
        bad = []
        with np.load(a.fixture) as z:
            assert int(z["seed"]) == SEED
            for n, (ins, out) in results.items():
                if not np.array_equal(z["in/" + n], ins):
                    bad.append(n + " (inputs)")
                elif not np.array_equal(z["out/" + n], stored(out)):
                    bad.append(n)
        print("%d cases against %s: %s" % (len(results), a.fixture, "all equal" if not bad else "DIFFERENT: " + ", ".join(bad)))
        return 1 if bad else 0
    differ = [n for n in CASES if not np.array_equal(R.run(n, BIT8)[1], results[n][1])]
    if differ:
        print("NOT recorded: az_nn_debug bit 8 changes the bytes of " + ", ".join(differ))
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.fixture)), exist_ok=True)
    np.savez_compressed(a.fixture, seed=np.int64(SEED), w2=R.wdigest["w2", False],
                        **{"in/" + n: v[0] for n, v in results.items()}, **{"out/" + n: stored(v[1]) for n, v in results.items()})
    print("recorded %d cases from %s to %s (%d bytes)" % (len(results), PKG, a.fixture, os.path.getsize(a.fixture)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
