#!/usr/bin/env python3
"""Times the weighting tree of an MSA (g2g_ktree_from_msa's two halves) on the GPU box:

  kernel_ms   g2g_msa_div_kernel alone, HIP events on the context's stream (context option KTREE_TIMING), median of 10 warm runs
  call_ms     g2g_msa_divergence as a caller sees it: device allocation, upload of the MSA, the kernel, download of the
              distances and counts (16 + 8 bytes per pair), wall clock, median of the same 10 runs
  tree_ms     g2g_ktree_from_dist (UPGMA + Kirchhoff weights, host, one core), wall clock, median of 5

Shapes: the 256 x 5206 start MSA of tests/golden/refine_prot256x1024_prog.json.gz (its tree is also checked against the fixture's),
and seeded synthetic families of 1024 x 5000 and 4096 x 5000 (members mutated from one ancestor at rates spread over 5 .. 60 %, a
fifth of the cells gaps in runs).  column_steps = pairs x columns is the work of the kernel; steps_per_ns follows from kernel_ms.
The reference's own time for the same loop (Ktree(msd) inside prrn5) is NOT reported: the trace (oracle/ref_trace.cc) carries no
clock, and it wraps Randiv's constructor, not Ktree's.
Usage: python tools/ktree_probe.py [--out profiles/NAME.json] [--shapes fixture,1024,4096]"""
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


def synthetic(many, ln, seed):
    rng = np.random.default_rng(seed)
    anc = rng.integers(2, 22, ln).astype(np.uint8)
    codes = np.repeat(anc[:, None], many, axis=1)
    rate = rng.uniform(0.05, 0.6, many)
    mut = rng.random((ln, many)) < rate[None, :]
    codes[mut] = rng.integers(2, 22, int(mut.sum())).astype(np.uint8)
    for m in range(many):                                               # gaps in runs of 1 .. 40 columns, about a fifth of the cells
        at = 0
        while at < ln:
            at += int(rng.integers(1, 160))
            run = int(rng.integers(1, 41))
            codes[at:at + run, m] = 1
            at += run
    return codes


def probe(ctx, name, codes, reps=10):
    from prrn_aln_amd import guide
    from prrn_aln_amd.refine import KTree
    ln, many = codes.shape
    kernel, call = [], []
    for k in range(reps + 2):                                           # two warm-up runs: code object load, first allocation
        t0 = time.perf_counter()
        dist, counts = guide.msa_divergence(ctx, codes)
        dt = (time.perf_counter() - t0) * 1e3
        if k >= 2:
            call.append(dt)
            kernel.append(float(ctx.get_option("KTREE_KERNEL_MS")))
    tree = []
    for _ in range(5):
        t0 = time.perf_counter()
        t = KTree.from_dist(dist)
        tree.append((time.perf_counter() - t0) * 1e3)
    pairs = many * (many - 1) // 2
    km = statistics.median(kernel)
    return {"shape": name, "members": many, "columns": ln, "pairs": pairs, "column_steps": pairs * ln,
            "kernel_ms": round(km, 4), "kernel_ms_min_max": [round(min(kernel), 4), round(max(kernel), 4)],
            "steps_per_ns": round(pairs * ln / (km * 1e6), 2), "call_ms": round(statistics.median(call), 3),
            "tree_ms": round(statistics.median(tree), 3), "tree_ms_min_max": [round(min(tree), 3), round(max(tree), 3)],
            "runs": reps, "nan_pairs": int(np.isnan(dist).sum())}, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shapes", default="fixture,1024,4096")
    a = ap.parse_args()
    from prrn_aln_amd import engine
    ctx = engine.Context()
    ctx.set_option("KTREE_TIMING", 1)
    rows = []
    for s in a.shapes.split(","):
        if s == "fixture":
            import refinelib
            path = [p for p in refinelib.fixtures() if "256x1024" in p][0]
            f, ref, _, codes = refinelib.load(path)
            r, t = probe(ctx, "refine_prot256x1024_prog start MSA", codes)
            r["tree_equals_fixture"] = (t.left, t.right, t.parent, t.vol, t.cur) == (ref.left, ref.right, ref.parent, ref.vol, ref.cur)
        else:
            r, _ = probe(ctx, "synthetic %s x 5000" % s, synthetic(int(s), 5000, int(s)))
        print(json.dumps(r), flush=True)
        rows.append(r)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump({"tool": "tools/ktree_probe.py", "timing": "kernel: HIP events, median of 10 warm runs in one process; call / tree: wall clock",
                   "rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
