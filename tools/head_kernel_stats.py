#!/usr/bin/env python
"""The kernels of an extraction pass outside the trunk in a rocprofv3 --kernel-trace CSV of
`tools/extract_leg.py --copy-peak` (NetVLAD, 256 frames of 480 x 640, crop 376): ms per pass over the last
`--iters` passes and the bytes each must move over that time, as a fraction of the run's own streaming-copy rate.

    python tools/head_kernel_stats.py <kernel_trace.csv> --copy-gbs <hbm_copy_GBs printed by the run> [--iters 8]
"""
import argparse
import collections
import csv

B, DIN, DOUT, S, P, C = 256, 32768, 4096, 8, 196, 512
MB = 1e6
V = B * DIN * 4                      # one VLAD row set as float32, or as fp16 pairs: the same bytes
PART = S * B * DOUT * 4
OUT = B * DOUT * 4
# bytes each kernel must move (reads + writes), parent and fused forms
BYTES = {
    "preprocess_tile_kernel": B * 376 * 376 * 3 + B * 3 * 224 * 224 * 4,
    "vlad_mfma_kernel": B * P * C * 4 + V,
    "pca_pairs_rows_kernel": 2 * V,
    "pca product (wino_gemm_h2_kernel)": S * DOUT * (DIN // S) * 4 + V + PART,
    "pca_epilogue_pairs_kernel": PART + OUT,
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("csv")
    ap.add_argument("--copy-gbs", type=float, required=True)
    ap.add_argument("--iters", type=int, default=8)
    a = ap.parse_args()
    rows = list(csv.DictReader(open(a.csv)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    idx = [i for i, r in enumerate(rows) if "preprocess_tile" in r["Kernel_Name"]]
    sel = rows[idx[-a.iters]:]
    t = collections.defaultdict(list)
    head = False                       # behind the VLAD kernel of a pass: the pair product is the projection's, not the trunk's
    for r in sel:
        n = r["Kernel_Name"]
        ms = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        if "preprocess_tile" in n:
            head = False
        for k in BYTES:
            if k in n:
                t[k].append(ms)
        if "vlad_mfma" in n:
            head = True
        elif head and "wino_gemm_h2_kernel" in n:
            t["pca product (wino_gemm_h2_kernel)"].append(ms)
    print("last %d passes of %d frames; copy rate of this run %.0f GB/s" % (a.iters, B, a.copy_gbs))
    print("%-36s %9s %9s %9s %10s %9s" % ("kernel", "ms/pass", "min", "max", "MB moved", "of copy"))
    tot = 0.0
    for k, b in BYTES.items():
        if not t[k]:
            print("%-36s %9s" % (k, "not run"))
            continue
        per = sum(t[k]) / a.iters
        tot += per
        print("%-36s %9.4f %9.4f %9.4f %10.0f %9.3f" % (k, per, min(t[k]), max(t[k]), b / MB, b / (per * 1e-3) / 1e9 / a.copy_gbs))
    print("%-36s %9.4f" % ("sum", tot))


if __name__ == "__main__":
    main()
