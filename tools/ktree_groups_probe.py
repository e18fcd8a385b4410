#!/usr/bin/env python3
"""Times the weighting tree over given groups on the GPU box:

  kernel_ms   the four kernels of g2g_msa_divergence_groups together (the member-pair kernel, the per-column group counts, the gap
              walk of one lane per (member, other group), the sums per group pair), HIP events on the context's stream (context option
              KTREE_TIMING -> KTREE_GROUPS_KERNEL_MS), median of 10 warm runs with min and max
  call_ms     g2g_msa_divergence_groups as a caller sees it: reordering the members on the host, device allocation, upload, the
              kernels, download of the group distances and counts; wall clock, median of the same runs
  tree_ms     g2g_ktree_from_msa_groups: the same plus the download of the member distances, every group's own tree and weights, the
              tree over the groups and the final weights; wall clock, median of 3

Inputs: the 256 x 5206 start MSA tests/golden/msa/prog256x1024.npz in 16 groups of 16 and in 128 pairs (consecutive members), and
tools/ktree_probe.py's seeded synthetic 4096 x 5000 star in 64 groups of 64 and in 2048 pairs.  member_steps = columns x the sum of
ni x nj over the group pairs is what the reference's triple loop walks; lane_steps = columns x members x (groups - 1) is what the
gap kernel walks.  A few group pairs of every input are recomputed with the restatement (tests/ktreegrouplib.py) and compared.
Usage: python tools/ktree_groups_probe.py [--out profiles/NAME.json] [--inputs msa16,msa2,star64,star2]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def probe(ctx, name, codes, size, reps=10, check=4):
    import ktreegrouplib as kg
    from ktreelib import elem
    from prrn_aln_amd import guide
    from prrn_aln_amd.refine import KTree
    ln, many = codes.shape
    groups = [np.arange(s, s + size, dtype=np.int32) for s in range(0, many, size)]
    num = len(groups)
    kernel, call = [], []
    for k in range(reps + 2):                                           # two warm-up runs: code object load, first allocation
        t0 = time.perf_counter()
        dist, counts = guide.msa_divergence_groups(ctx, codes, groups)
        dt = (time.perf_counter() - t0) * 1e3
        if k >= 2:
            call.append(dt)
            kernel.append(float(ctx.get_option("KTREE_GROUPS_KERNEL_MS")))
    tree = []
    for _ in range(3):
        t0 = time.perf_counter()
        t, w = KTree.from_msa_groups(ctx, codes, groups)
        tree.append((time.perf_counter() - t0) * 1e3)
    rng = np.random.default_rng(num)
    same = True
    for _ in range(check):
        l = int(rng.integers(1, num))
        k = int(rng.integers(0, l))
        same = same and tuple(counts[elem(k, l)]) == kg.group_counts(codes, groups[k], groups[l])
    km = statistics.median(kernel)
    pairs = num * (num - 1) // 2
    return {"input": name, "members": many, "columns": ln, "groups": num, "group_size": size, "group_pairs": pairs,
            "member_steps": ln * pairs * size * size, "lane_steps": ln * many * (num - 1),
            "kernel_ms": round(km, 4), "kernel_ms_min_max": [round(min(kernel), 4), round(max(kernel), 4)],
            "call_ms": round(statistics.median(call), 3), "call_ms_min_max": [round(min(call), 3), round(max(call), 3)],
            "tree_ms": round(statistics.median(tree), 3), "tree_ms_min_max": [round(min(tree), 3), round(max(tree), 3)],
            "runs": reps, "nan_pairs": int(np.isnan(dist).sum()), "sum_of_weights": float(np.sum(w)),
            "sampled_pairs_equal_the_restatement": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--inputs", default="msa16,msa2,star64,star2")
    a = ap.parse_args()
    from prrn_aln_amd import engine
    ctx = engine.Context()
    ctx.set_option("KTREE_TIMING", 1)
    rows, star, msa = [], None, None
    for s in a.inputs.split(","):
        size = int(s[3:] if s.startswith("msa") else s[4:])
        if s.startswith("msa"):
            if msa is None:
                msa = np.load(os.path.join(ROOT, "tests", "golden", "msa", "prog256x1024.npz"))["codes"]
            r = probe(ctx, "prog256x1024 start MSA", msa, size)
        else:
            if star is None:
                import ktree_probe
                star = ktree_probe.synthetic(4096, 5000, 4096)
            r = probe(ctx, "synthetic 4096 x 5000 star", star, size, check=2)
        print(json.dumps(r), flush=True)
        rows.append(r)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump({"tool": "tools/ktree_groups_probe.py", "timing": "kernel: HIP events, median of 10 warm runs in one process; call / tree: wall clock",
                   "rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
