#!/usr/bin/env python3
"""Idle time around the evaluator's convolution launches, from one rocprofv3 --kernel-trace run of bench.py.

    python tools/conv_chain_gaps.py TRACE_DIR_OR_CSV [OUT.csv]

Finds every evaluator forward in the per-dispatch trace - k_stem_conv_block, k_conv_block x (n_blocks - 1), k_attn_heads
in a row on one queue, or k_conv_chain, k_attn_heads - and prints (and writes to OUT.csv) the medians of each kernel's
duration, of the end-to-start gaps between them, and of the span from the first start to the last end against the sum
of the durations.  All figures in us.  Reads files only: nothing is run.
"""
import csv
import glob
import os
import statistics
import sys


def short(name):
    for k in ("k_stem_conv_block", "k_conv_chain", "k_conv_block", "k_attn_heads"):
        if k in name:
            return k
    return None


def load(path):
    if os.path.isdir(path):
        hits = sorted(glob.glob(os.path.join(path, "**", "*kernel_trace.csv"), recursive=True))
        if not hits:
            sys.exit(f"no *kernel_trace.csv under {path}")
        path = hits[0]
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], r.get("Queue_Id", "")))
    rows.sort()
    return rows


def forwards(rows):
    """lists of (short name, start, end): a stem (or chain) launch up to the next k_attn_heads, with nothing else between"""
    out, cur = [], None
    for s, e, name, _q in rows:
        k = short(name)
        if k in ("k_stem_conv_block", "k_conv_chain"):
            cur = [(k, s, e)]
        elif cur is not None and k == "k_conv_block":
            cur.append((k, s, e))
        elif cur is not None and k == "k_attn_heads":
            cur.append((k, s, e))
            out.append(cur)
            cur = None
        else:
            cur = None
    return out


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    fw = forwards(load(sys.argv[1]))
    if not fw:
        sys.exit("no evaluator forward found in the trace")
    # the most common shape of a forward (the lead-in may run other routes)
    shape = statistics.mode(tuple(k for k, _, _ in f) for f in fw)
    fw = [f for f in fw if tuple(k for k, _, _ in f) == shape]
    med = lambda v: statistics.median(v) / 1000.0
    lines = [("forwards", len(fw))]
    for i, k in enumerate(shape):
        lines.append((f"dur_{i}_{k}_us", round(med([f[i][2] - f[i][1] for f in fw]), 3)))
    for i in range(len(shape) - 1):
        lines.append((f"gap_{i}_{shape[i]}_to_{shape[i + 1]}_us", round(med([f[i + 1][1] - f[i][2] for f in fw]), 3)))
    span = [f[-1][2] - f[0][1] for f in fw]
    tot = [sum(e - s for _, s, e in f) for f in fw]
    lines.append(("span_first_start_to_last_end_us", round(med(span), 3)))
    lines.append(("sum_of_durations_us", round(med(tot), 3)))
    lines.append(("span_excess_us", round(med([a - b for a, b in zip(span, tot)]), 3)))
    # the conv part alone: first conv start to last conv end (what one k_conv_chain launch replaces)
    nconv = len(shape) - 1
    lines.append(("conv_span_us", round(med([f[nconv - 1][2] - f[0][1] for f in fw]), 3)))
    for k, v in lines:
        print(f"{k},{v}")
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            f.write("figure,median\n")
            for k, v in lines:
                f.write(f"{k},{v}\n")


if __name__ == "__main__":
    main()
