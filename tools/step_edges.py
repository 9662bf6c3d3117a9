#!/usr/bin/env python
"""The two edges of a headline step in a rocprofv3 --kernel-trace CSV of `python bench.py --gpus 1 --steps K --warmup W`:
what runs between the fork of the extraction lanes and the first stem kernel (head), and between the end of the first lane's
trunk and the start of the step's search (tail).  Those are the stretches in which no chip-filling trunk kernel is queued.

    python tools/step_edges.py <kernel_trace.csv> [--step -2]      (index into the trace's searches; -2 = the last but one)
"""
import argparse
import collections
import csv


def short(n):
    if n.startswith("void "):
        n = n[5:]
    return n.split("(")[0][:64]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--step", type=int, default=-2)
    a = ap.parse_args()
    rows = list(csv.DictReader(open(a.csv)))
    for r in rows:
        r["t0"], r["t1"], r["name"] = int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])
    rows.sort(key=lambda r: r["t0"])
    searches = [i for i, r in enumerate(rows) if "sim_topk_ring_kernel" in r["name"]]
    si = searches[a.step]
    prev = searches[searches.index(si) - 1]
    search = rows[si]
    # the previous step ends with the last kernel of the caller's stream behind its search: the lanes fork behind it
    caller = search["Stream_Id"]
    step = [r for r in rows[prev + 1:si + 1]]
    stems = [r for r in step if "conv_stem_direct_h_kernel" in r["name"]]
    first_stem = min(stems, key=lambda r: r["t0"])
    before = [r for r in step if r["Stream_Id"] == caller and r["t1"] <= first_stem["t0"]]
    fork = max(r["t1"] for r in before) if before else rows[prev]["t1"]
    # a lane's trunk ends with the kernel in front of its VLAD kernel
    by_stream = collections.defaultdict(list)
    for r in step:
        by_stream[r["Stream_Id"]].append(r)
    trunk_ends = []
    for s, rs in sorted(by_stream.items()):
        for j, r in enumerate(rs):
            if "vlad_mfma_kernel" in r["name"] and j > 0:
                trunk_ends.append((rs[j - 1]["t1"], s, rs[j - 1]["name"]))
    first_done = min(trunk_ends)
    last_done = max(trunk_ends)

    def show(title, lo, hi):
        print("%s: %.3f ms" % (title, (hi - lo) / 1e6))
        inside = [r for r in step if r["t1"] > lo and r["t0"] < hi]
        busy = collections.defaultdict(int)
        for r in inside:
            busy[r["name"]] += min(r["t1"], hi) - max(r["t0"], lo)
        for r in inside:
            print("    stream %s  %+9.3f .. %+9.3f ms  (%7.3f)  %s" % (r["Stream_Id"], (r["t0"] - lo) / 1e6, (r["t1"] - lo) / 1e6,
                                                                   (r["t1"] - r["t0"]) / 1e6, r["name"]))
        print("  kernel time inside the span, summed over the streams:")
        for k, v in sorted(busy.items(), key=lambda kv: -kv[1]):
            print("    %8.3f ms  %s" % (v / 1e6, k))

    print("step: search %d of %d in the trace; previous search to this search: %.3f ms" %
          (searches.index(si), len(searches), (search["t0"] - rows[prev]["t0"]) / 1e6))
    print("streams:", ", ".join("%s (queue %s)" % (s, rs[0]["Queue_Id"]) for s, rs in sorted(by_stream.items())))
    show("head: fork (last kernel of the caller's stream) -> first conv_stem_direct_h_kernel", fork, first_stem["t0"])
    print("lanes' trunks end (ms before the search starts): " +
          ", ".join("stream %s %.3f (%s)" % (s, (search["t0"] - t) / 1e6, n) for t, s, n in sorted(trunk_ends)))
    show("tail: first lane's last trunk kernel -> sim_topk_ring_kernel", first_done[0], search["t0"])
    print("tail behind the LAST lane's trunk: %.3f ms" % ((search["t0"] - last_done[0]) / 1e6))


if __name__ == "__main__":
    main()
