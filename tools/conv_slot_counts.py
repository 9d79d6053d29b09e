#!/usr/bin/env python3
"""Static instruction counts of the kernels of nn_conv.hip, from the compiler's assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fPIC -I include -I alphazero-al_amd/csrc \\
          -S --cuda-device-only alphazero-al_amd/csrc/nn_conv.hip -o nn_conv.s
    python tools/conv_slot_counts.py nn_conv.s [label]

Per kernel: the resource lines of the .s trailer (VGPRs, spilled SGPRs / VGPRs, scratch bytes, occupancy), then the
instructions of the TILE LOOP by class - the loop whose blocks (by the compiler's block comments) hold the MFMAs -
for the whole loop and for the stretches between its barriers (text order: P0 + P1 | staging + matrix phase + woven
epilogue | P3, for a loop the compiler did not rotate).  The counts are static: a block behind a debug bit or the phase
stamps counts as much as one that always runs, and nothing here knows how often a block executes.
"""
import re
import sys

CLASSES = ("vector", "mfma", "transc", "scalar+branch", "lds", "global", "nop/wait")
TRANSC = ("v_exp_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_log_", "v_sin_", "v_cos_")


def classify(op):
    if op == "s_barrier":
        return None
    if op.startswith("v_mfma") or op.startswith("v_smfma"):
        return "mfma"
    if op.startswith(TRANSC):
        return "transc"
    if op.startswith("v_"):
        return "vector"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "global"
    if op in ("s_nop", "s_waitcnt") or op.startswith("s_waitcnt"):
        return "nop/wait"
    if op.startswith("s_"):
        return "scalar+branch"
    return None


def kernels(text):
    """name -> list of (loop, mnemonic) in text order; loop is the header (BBn_m) of the loop the compiler's block
    comment puts the instruction's basic block in, or None"""
    out, cur, name, loop = {}, None, None, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, cur, loop = m.group(1), [], None
            continue
        if cur is None:
            continue
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)", line)
        if m:
            h = re.search(r"(?:Header=|Parent Loop )(BB\d+_\d+)", m.group(2))
            loop = h.group(1) if h else (m.group(1) if "Loop Header" in m.group(2) else None)
            continue
        body = line.split(";")[0].strip()
        if not body or body.startswith("."):
            continue
        op = body.split(None, 1)[0]
        cur.append((loop, op))
        if op == "s_endpgm":
            out[name], cur = cur, None
    return out


def tile_loop(items):
    """the instructions of the loop that holds the matrix instructions"""
    per = {}
    for loop, op in items:
        if loop and op.startswith("v_mfma"):
            per[loop] = per.get(loop, 0) + 1
    if not per:
        return None
    head = max(per, key=per.get)
    return [it for it in items if it[0] == head]


def count(items):
    c = dict.fromkeys(CLASSES, 0)
    for _, op in items:
        k = classify(op)
        if k:
            c[k] += 1
    return c


def resources(text):
    res = {}
    for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name:
            continue
        get = lambda k: re.search(r"\.%s:\s+(\d+)" % k, blk)
        res[name.group(1)] = {k: int(get(k).group(1)) for k in ("vgpr_count", "sgpr_spill_count", "vgpr_spill_count", "private_segment_fixed_size") if get(k)}
    occ = re.findall(r"^; Occupancy: (\d+)", text, re.M)
    return res, occ


def main():
    text = open(sys.argv[1]).read()
    label = sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]
    res, occ = resources(text)
    print("== %s" % label)
    for n, (name, items) in enumerate(kernels(text).items()):
        r = res.get(name, {})
        print("%s\n  VGPRs %s, spilled SGPRs %s, spilled VGPRs %s, scratch %s B, occupancy %s" % (
            name, r.get("vgpr_count"), r.get("sgpr_spill_count"), r.get("vgpr_spill_count"),
            r.get("private_segment_fixed_size"), occ[n] if n < len(occ) else "?"))
        loop = tile_loop(items)
        if loop is None:
            continue
        print("  %-28s" % "tile loop" + " ".join("%s %4d" % (k, v) for k, v in count(loop).items()))
        seg, k = [], 0
        for it in loop + [(None, "s_barrier")]:
            if it[1] == "s_barrier":
                print("  %-28s" % ("  stretch %d (to a barrier)" % k) + " ".join("%s %4d" % (a, b) for a, b in count(seg).items()))
                seg, k = [], k + 1
            else:
                seg.append(it)


if __name__ == "__main__":
    main()
