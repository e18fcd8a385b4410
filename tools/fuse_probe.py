#!/usr/bin/env python3
"""Times g2g_refine_plan (what prrn's default run decides before it refines: fused groups, attack ranges, per-range groups) on the GPU
box, per MSA:

  kernel_ms    g2g_mayfuse_kernel alone, HIP events on the context's stream, summed over the call's launches (context option
               FUSE_TIMING leaves FUSE_KERNEL_MS)
  build_ms     the sons of every fuse test extracted and built: g2g_group_create on host threads + g2g_pwdm_create_batch
               (FUSE_BUILD_MS, wall clock)
  host_ms      collecting the rounds' candidates, the groups and the rearranged trees (FUSE_HOST_MS, wall clock)
  consreg_*    the grouped g2g_consreg inside the plan (CONSREG_TIMING: its builders, its kernel)
  call_ms      g2g_refine_plan as a caller sees it, wall clock
medians of --runs warm runs in one process after one warm-up run (code object load, first allocations), with min / max.

MSAs: tests/golden/msa/prog256x1024.npz (256 x 5206; its tree from g2g_ktree_from_msa: nothing fuses, one range) and a clustered
family from synth -- 16 diverged ancestors (make_family without indels), 16 members each with 2 % of their columns substituted --
that does fuse.  Parameters: the reference's localprm (u 3, v 10, thr 35, similarity matrix number 1 as the fixtures record it).
--reference FILE merges the line `tools/make_fuse_golden.py --time` printed (the reference's own consregss + grouped consreg +
per-range consregss, one CPU core).
Usage: python tools/fuse_probe.py [--out profiles/fuse_probe.json] [--runs 5] [--reference FILE]"""
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


def clustered_family(clusters=16, per=16, length=600, seed=7, within=0.02):
    from prrn_aln_amd import operator as op
    from prrn_aln_amd.synth import make_family
    anc = op.encode(list(make_family(clusters, length, seed, sub=0.25, indel=0.0).msa), op.PROTEIN)
    rng = np.random.default_rng(seed)
    cols = []
    for c in range(clusters):
        for m in range(per):
            s = anc[:, c].copy()
            hit = rng.random(len(s)) < within
            s[hit] = rng.integers(3, 23, int(hit.sum()))
            cols.append(s)
    return np.ascontiguousarray(np.stack(cols, 1), np.uint8)


def probe(ctx, name, codes, tree, prm, thr, runs):
    from prrn_aln_amd import guide
    keys = ("FUSE_KERNEL_MS", "FUSE_BUILD_MS", "FUSE_HOST_MS", "CONSREG_KERNEL_MS", "CONSREG_BUILD_MS")
    rows = {k: [] for k in keys}
    call = []
    plan = None
    for r in range(runs + 1):
        for k in keys:
            ctx.set_option(k, None)
        t0 = time.perf_counter()
        plan = guide.refine_plan(ctx, codes, tree, prm, thr)
        dt = (time.perf_counter() - t0) * 1e3
        if r >= 1:
            call.append(dt)
            for k in keys:
                rows[k].append(float(ctx.get_option(k) or 0.))
    med = statistics.median
    res = {"msa": name, "members": int(codes.shape[1]), "columns": int(codes.shape[0]), "thr": thr, "runs": runs,
           "whole_fused": bool(plan.whole.fused), "groups": len(plan.whole.groups), "ranges": plan.ranges.tolist(),
           "fused_inside": [bool(r.fused) for r in plan.relations], "groups_inside": [len(r.groups) for r in plan.relations],
           "tests": plan.stats.tests, "tests_fused": plan.stats.fused, "launches": plan.stats.launches}
    for k, label in zip(keys, ("kernel_ms", "build_ms", "host_ms", "consreg_kernel_ms", "consreg_build_ms")):
        res[label] = round(med(rows[k]), 3)
        res[label + "_min_max"] = [round(min(rows[k]), 3), round(max(rows[k]), 3)]
    res["call_ms"] = round(med(call), 3)
    res["call_ms_min_max"] = [round(min(call), 3), round(max(call), 3)]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reference", help="the JSON line of tools/make_fuse_golden.py --time")
    a = ap.parse_args()
    import fuselib as fl
    import consreglib as cl
    from prrn_aln_amd import engine
    from prrn_aln_amd.refine import KTree
    g = dict(fl.fixtures())["prot12_clusters"]
    prm, keep = cl.alp_of(g).to_c()
    ctx = engine.Context()
    ctx.set_option("FUSE_TIMING", 1)
    ctx.set_option("CONSREG_TIMING", 1)
    big = np.load(os.path.join(ROOT, "tests", "golden", "msa", "prog256x1024.npz"))["codes"]
    fam = clustered_family()
    rows = [probe(ctx, "prog256x1024", big, KTree.from_msa(ctx, big), prm, 35., a.runs),
            probe(ctx, "clustered16x16", fam, KTree.from_msa(ctx, fam), prm, 35., a.runs)]
    ctx.close()
    for r in rows:
        print(json.dumps(r), flush=True)
    ref = None
    if a.reference and os.path.exists(a.reference):
        ref = json.load(open(a.reference))["reference_preprrn_decisions_one_core"]
        for r in rows:
            if r["msa"] in ref:
                r["decisions_equal_reference"] = ref[r["msa"]]["groups"] == r["groups"] and ref[r["msa"]]["ranges"] == r["ranges"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump({"tool": "tools/fuse_probe.py",
                   "timing": "kernels: HIP events; the rest wall clock; medians of warm runs in one process after one warm-up run",
                   "rows": rows, "reference_preprrn_decisions_one_core": ref}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
