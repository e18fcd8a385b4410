#!/usr/bin/env python3
"""What the progressive alignment of the bench family costs on the GPU, in one process on the GPU box:

  family   synth.make_family(256, 1024, 1), the unaligned sequences
  tree     guide.distance_matrix (alnScoreD of all pairs) + KTree.from_dist(with_weights=False)
  run      guide.progressive over it, after a warm-up call on eight of the sequences (code object load)

written to profiles/progressive_probe.json: waves, DPs per wave, ms per wave (wall clock between the ends of two waves, from the
merges' t_ms: groups, PwdMs, DPs and the interleaving of a wave), total ms of the call, DP cells (columns of the left son x columns
of the right son, summed over the merges: the rectangles, not the bands), the result's size, and the tree itself -- so that
tools/make_progressive_golden.py --time-bench can time the reference's own merges over the same tree on one core and write its
figure into the same file.  Whether the result equals tests/golden/msa/prog256x1024.npz is reported, not asserted: that MSA came from
prrn5's own guide forest, so equality is not expected.  No threshold is set: nobody has measured this before.
--checker: no GPU -- the tree from tests/kmerlib.py, the DPs by the CPU checker; for trying the tool on a small family.
Usage: python tools/progressive_probe.py [--out profiles/progressive_probe.json] [--members 256] [--length 1024] [--max-batch 0] [--checker]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "progressive_probe.json"))
    ap.add_argument("--members", type=int, default=256)
    ap.add_argument("--length", type=int, default=1024)
    ap.add_argument("--max-batch", type=int, default=0)
    ap.add_argument("--checker", action="store_true")
    a = ap.parse_args()
    from prrn_aln_amd import guide
    from prrn_aln_amd import operator as op
    from prrn_aln_amd.refine import KTree
    from prrn_aln_amd.synth import make_family
    fam = make_family(a.members, a.length, 1)
    seqs = [op.encode([s], op.PROTEIN).reshape(-1) for s in fam.seqs]
    alp = op.AlnParam()
    prm, sm = alp.to_c()
    kw = {}
    if a.checker:
        import kmerlib
        import proglib
        ctx = None
        t0 = time.perf_counter()
        dist = kmerlib.distance(seqs, op.PROTEIN, 3)[0]
        kw = dict(aligner=proglib.oracle_aligner())
    else:
        from prrn_aln_amd import engine
        ctx = engine.Context()
        few = seqs[:8]
        guide.progressive(ctx, few, KTree.from_dist(guide.distance_matrix(ctx, prm, few, sm), with_weights=False), prm)     # warm-up
        t0 = time.perf_counter()
        dist = guide.distance_matrix(ctx, prm, seqs, sm)
    tree = KTree.from_dist(dist, with_weights=False)
    tree_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    codes, order, merges, stats = guide.progressive(ctx, seqs, tree, prm, max_batch=a.max_batch, **kw)
    total_ms = (time.perf_counter() - t0) * 1e3
    if ctx is not None:
        ctx.close()
    n = len(seqs)
    for k in range(n):
        assert np.array_equal(codes[:, k][codes[:, k] > 1], seqs[order[k]]), "member %d is not sequence %d" % (k, order[k])
    ln = {i: len(s) for i, s in enumerate(seqs)}
    waves, cells = {}, 0
    for m in merges:
        ln[m["node"]] = m["len"]
        c = ln[m["left"]] * ln[m["right"]]
        cells += c
        w = waves.setdefault(m["wave"], {"dps": 0, "cells": 0, "end_ms": m["t_ms"], "modes": {}, "most_members": 0})
        w["dps"] += 1; w["cells"] += c
        w["modes"][str(m["mode"])] = w["modes"].get(str(m["mode"]), 0) + 1
        w["most_members"] = max(w["most_members"], m["na"] + m["nb"])
    rows, last = [], 0.
    for k in sorted(waves):
        w = waves[k]
        rows.append({"wave": k, "dps": w["dps"], "ms": round(w["end_ms"] - last, 2), "cells": w["cells"], "modes": w["modes"], "most_members": w["most_members"]})
        last = w["end_ms"]
    same = None
    gold = os.path.join(ROOT, "tests", "golden", "msa", "prog256x1024.npz")
    if (a.members, a.length) == (256, 1024) and os.path.exists(gold):
        back = np.empty_like(order); back[order] = np.arange(n, dtype=order.dtype)
        ref = np.load(gold)["codes"]
        same = bool(ref.shape == codes.shape and np.array_equal(ref, codes[:, back]))
        ref_columns = int(ref.shape[0])
    res = {"tool": "tools/progressive_probe.py", "family": "synth.make_family(%d, %d, 1)" % (a.members, a.length), "members": n, "length": a.length,
           "dps_on": "CPU checker" if a.checker else "GPU", "timing": "wall clock, one run in one process after a warm-up call",
           "guide_tree": "tests/kmerlib.py k = 3 + KTree.from_dist" if a.checker else "guide.distance_matrix + KTree.from_dist", "guide_tree_ms": round(tree_ms, 1),
           "max_batch": a.max_batch or 64, "merges": stats["merges"], "waves": stats["waves"], "largest_wave": stats["largest_wave"],
           "total_ms": round(total_ms, 1), "dp_cells": int(cells), "columns": int(codes.shape[0]),
           "wait_timeouts": stats["wait_timeouts"], "recovered_dps": stats["recovered_dps"], "per_wave": rows,
           "equals_prog256x1024": same, "tree": {"left": list(map(int, tree.left)), "right": list(map(int, tree.right)), "parent": list(map(int, tree.parent))}}
    if same is not None:
        res["prog256x1024_columns"] = ref_columns
    print(json.dumps({k: v for k, v in res.items() if k not in ("tree", "per_wave")}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
