#!/usr/bin/env python3
"""Times the conserved-region search (g2g_consreg) on the GPU box, per MSA:

  build_ms     the sons of every division extracted and built: g2g_group_create on host threads + g2g_pwdm_create_batch (the device
               builders), wall clock inside the call (context option CONSREG_TIMING leaves CONSREG_BUILD_MS)
  kernel_ms    g2g_consreg_kernel alone, HIP events on the context's stream, summed over the call's chunks (CONSREG_KERNEL_MS)
  constwo_ms   g2g_constwo_batch as g2g_consreg sees it: packing, upload, kernel, download (CONSREG_CONSTWO_MS, wall clock)
  host_ms      cmnrng over the divisions and complerng (CONSREG_HOST_MS, wall clock)
  call_ms      g2g_consreg as a caller sees it, wall clock
each MSA twice: as a caller gets it (the loop over the divisions stops once the intersection is empty, like the reference's) and with
every division scored (context option CONSREG_NO_EARLY_STOP), which is the work the kernel was written for;
medians of --runs warm runs in one process after one warm-up run (code object load, first allocations), with min / max.

MSAs: tests/golden/msa/prog256x1024.npz (256 x 5206: 509 divisions; its tree from g2g_ktree_from_msa) and the 16-member fixture
tests/golden/consreg/prot16_pf.npz (its recorded tree).  Parameters: the reference's localprm (u 3, v 10, thr 35, similarity matrix
number 1 as the fixture records it), dissim = 1.  --reference FILE merges the line `tools/make_consreg_golden.py --time` printed (the
reference's own Ssrel::consreg on the same MSAs, one CPU core) and compares its ranges with the library's.
Usage: python tools/consreg_probe.py [--out profiles/consreg_probe.json] [--runs 5] [--reference FILE]"""
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


def probe(ctx, name, codes, tree, prm, thr, runs, all_divisions=False):
    from prrn_aln_amd import guide
    ctx.set_option("CONSREG_NO_EARLY_STOP", 1 if all_divisions else None)
    keys = ("CONSREG_BUILD_MS", "CONSREG_KERNEL_MS", "CONSREG_CONSTWO_MS", "CONSREG_HOST_MS")
    rows = {k: [] for k in keys}
    call = []
    out = None
    for r in range(runs + 1):
        t0 = time.perf_counter()
        out = guide.conserved_regions(ctx, codes, tree, prm, thr, None, True)
        dt = (time.perf_counter() - t0) * 1e3
        if r >= 1:
            call.append(dt)
            for k in keys:
                rows[k].append(float(ctx.get_option(k)))
    med = statistics.median
    res = {"msa": name, "members": int(codes.shape[1]), "columns": int(codes.shape[0]), "divisions": 2 * int(codes.shape[1]) - 3, "thr": thr,
           "every_division_scored": bool(all_divisions),
           "runs": runs, "dissim_ranges": out.tolist()}
    for k, label in zip(keys, ("build_ms", "kernel_ms", "constwo_ms", "host_ms")):
        res[label] = round(med(rows[k]), 3)
        res[label + "_min_max"] = [round(min(rows[k]), 3), round(max(rows[k]), 3)]
    res["call_ms"] = round(med(call), 3)
    res["call_ms_min_max"] = [round(min(call), 3), round(max(call), 3)]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--reference", help="the JSON line of tools/make_consreg_golden.py --time")
    a = ap.parse_args()
    import consreglib as cl
    from prrn_aln_amd import engine
    from prrn_aln_amd.refine import KTree
    g = dict(cl.fixtures())["prot16_pf"]
    alp = cl.alp_of(g)
    prm, keep = alp.to_c()
    ctx = engine.Context()
    ctx.set_option("CONSREG_TIMING", 1)
    big = np.load(os.path.join(ROOT, "tests", "golden", "msa", "prog256x1024.npz"))["codes"]

    class Small:
        left, right, parent = g["tree_left"], g["tree_right"], g["tree_parent"]
    tree = KTree.from_msa(ctx, big)
    rows = [probe(ctx, "prog256x1024", big, tree, prm, 35., a.runs), probe(ctx, "prog256x1024", big, tree, prm, 35., a.runs, True),
            probe(ctx, "prot16_pf", g["codes"], Small, prm, 35., a.runs), probe(ctx, "prot16_pf", g["codes"], Small, prm, 35., a.runs, True)]
    ctx.close()
    ref = None
    if a.reference and os.path.exists(a.reference):
        ref = json.load(open(a.reference))["reference_consreg_one_core"]
        for r in rows:
            if r["msa"] in ref:
                r["ranges_equal_reference"] = ref[r["msa"]]["dissim_ranges"] == r["dissim_ranges"]
    for r in rows:
        r["n_dissim_ranges"] = len(r.pop("dissim_ranges"))
        print(json.dumps(r), flush=True)
    if ref:
        for v in ref.values():
            v["n_dissim_ranges"] = len(v.pop("dissim_ranges"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump({"tool": "tools/consreg_probe.py",
                   "timing": "kernel: HIP events; the rest wall clock; medians of warm runs in one process after one warm-up run",
                   "rows": rows, "reference_consreg_one_core": ref}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
