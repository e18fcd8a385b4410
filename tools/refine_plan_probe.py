#!/usr/bin/env python3
"""What prrn's default refinement costs next to the exhaustive one, on one MSA in one process on the GPU box:

  refine           g2g_refine: the `-YH0` trajectory -- every member a leaf, the whole MSA one range
  refine_planned   g2g_refine_planned with the plan made on the device (g2g_refine_plan, the reference's localprm: u 3, v 10, thr 35,
                   similarity matrix number 1 as the fixtures record it): fused groups, one loop per unconserved range

per run: wall time of the call, DPs (divisions that were scored and looked at), DP cells (rows x columns of those DPs, recounted on
the host by replaying the accepted moves -- see cells_of; the replay must end in the call's MSA), accepted moves, batches, divisions
scored but thrown away behind an acceptance.  refine_planned's wall time includes making the plan (plan_s).  The two runs refine
different things -- the planned run leaves conserved columns and the inside of fused groups alone -- so the pair is reported as what
the default run costs next to the exhaustive one, not as a speed-up of one computation.  g2g_refine's figure is the yardstick.

MSA: the clustered family of tools/fuse_probe.py (16 diverged ancestors, 16 members each, 600 columns) with deletions put into it: a
gapless MSA has no division to re-align.  Per cluster 3 deletions shared by its members and per member 2 of its own, 1 .. 4 columns
each, then slid 1 .. 3 columns to the right in half of the rows so that the start alignment is wrong in places.
--checker: no GPU -- the plan by tests/fuselib.py and the DPs by the CPU checker; for trying the tool on a small family.
Usage: python tools/refine_plan_probe.py [--out profiles/refine_plan_probe.json] [--clusters 16] [--per 16] [--length 600] [--checker]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GAP = 1


def gapped_family(clusters, per, length, seed=7):
    from fuse_probe import clustered_family
    codes = clustered_family(clusters, per, length, seed)
    rng = np.random.default_rng(seed + 1)
    for c in range(clusters):
        for _ in range(3):
            p, n = int(rng.integers(5, length - 10)), int(rng.integers(1, 5))
            codes[p:p + n, c * per:(c + 1) * per] = GAP
    for m in range(codes.shape[1]):
        for _ in range(2):
            p, n = int(rng.integers(5, length - 10)), int(rng.integers(1, 5))
            codes[p:p + n, m] = GAP
        if rng.random() < 0.5:                                   # slide this row's gap runs to the right
            col = codes[:, m].copy()
            i = 0
            while i < length:
                if col[i] != GAP:
                    i += 1
                    continue
                j = i
                while j < length and col[j] == GAP:
                    j += 1
                k = int(rng.integers(1, 4))
                if j + k <= length and not (col[j:j + k] == GAP).any():
                    seg = col[j:j + k].copy()
                    col[i:i + k] = seg
                    col[i + k:j + k] = GAP
                i = j + k
            codes[:, m] = col
    keep = (codes != GAP).any(1)                                 # no all-gap column in the start MSA
    return np.ascontiguousarray(codes[keep])


def summary(name, seconds, start, final, steps, stats, cells):
    dps = [s for s in steps if not s["skipped"]]
    return {"run": name, "wall_s": round(seconds, 3), "divisions": len(steps), "dps": len(dps), "dp_cells": int(cells),
            "accepted": int(stats["accepted"]), "batches": int(stats["batches"]), "wasted": int(stats["divisions_wasted"]),
            "columns": [int(start.shape[0]), int(final.shape[0])], "wait_timeouts": int(stats["wait_timeouts"]), "recovered_dps": int(stats["recovered_dps"])}


def cells_of(start, steps, moves, sides_of_step):
    """(sum over the scored, looked-at divisions of (columns of side a) x (columns of side b), the MSA the moves end in): the trajectory
    is replayed on the host -- the sides of a division are read off the MSA as it stood, their all-gap columns dropped (what the loop
    builds), an accepted skeleton interleaves them.  sides_of_step(i) -> (members a, members b, (left, right) of the range in the
    start MSA or None for the whole MSA)"""
    M = start.copy()
    total = 0
    mv = iter(moves)
    shift = {}
    for i, s in enumerate(steps):
        if s["skipped"]:
            continue
        la, lb, rng = sides_of_step(i)
        l, r = (0, M.shape[0]) if rng is None else (rng[0], rng[1] + shift.get(rng, 0))
        sub = M[l:r]
        ra = int((sub[:, la] != GAP).any(1).sum())
        rb = int((sub[:, lb] != GAP).any(1).sum())
        total += ra * rb
        if s["accepted"]:
            br, ma, mb, skl = next(mv)
            a = sub[(sub[:, ma] != GAP).any(1)][:, ma]
            b = sub[(sub[:, mb] != GAP).any(1)][:, mb]
            rows = []
            for (m0, n0), (m1, n1) in zip(skl[:-1], skl[1:]):
                for t in range(max(m1 - m0, n1 - n0)):
                    row = np.full(M.shape[1], GAP, np.uint8)
                    if m1 > m0:
                        row[ma] = a[m0 + t]
                    if n1 > n0:
                        row[mb] = b[n0 + t]
                    rows.append(row)
            new = np.stack(rows)
            M = np.concatenate([M[:l], new, M[r:]])
            if rng is not None:
                shift[rng] = shift.get(rng, 0) + len(new) - (r - l)
    return total, M


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--clusters", type=int, default=16)
    ap.add_argument("--per", type=int, default=16)
    ap.add_argument("--length", type=int, default=600)
    ap.add_argument("--checker", action="store_true")
    a = ap.parse_args()
    import consreglib as cl
    import fuselib as fl
    import ktreelib as kl
    from prrn_aln_amd import guide, refine
    from prrn_aln_amd import operator as op
    codes = gapped_family(a.clusters, a.per, a.length)
    ln, many = codes.shape
    alp = op.AlnParam()
    prm, _sm = alp.to_c()
    alp_plan = cl.alp_of(dict(fl.fixtures())["prot12_clusters"])
    pprm, _psm = alp_plan.to_c()
    kw = {}
    if a.checker:
        import refinelib
        import refineplanlib as rp
        ctx = None
        t = kl.tree_from_dist(kl.divergence(codes)[0])
        tree = refine.KTree(t["left"], t["right"], t["parent"], t["vol"], t["cur"])
        tree5 = tuple(np.asarray(t[k]) for k in ("left", "right", "parent", "vol", "cur"))
        plan = rp.plan_object(fl.plan(codes, tree5, alp_plan, 35., np.asarray(tree.vol[:many])))
        kw = dict(scorer=refinelib.oracle_scorer())
    else:
        from prrn_aln_amd import engine
        ctx = engine.Context()
        tree = refine.KTree.from_msa(ctx, codes)
        few = codes[:, :4]
        few = np.ascontiguousarray(few[(few != GAP).any(1)])
        refine.refine_native(ctx, few, refine.KTree.from_msa(ctx, few), alp, maxitr=1)      # warm-up: code object load
        plan = None
    weight = np.asarray(tree.vol[:many], np.float64)
    # ---- the -YH0 trajectory
    t0 = time.perf_counter()
    f0, s0, st0 = refine.refine_native(ctx, codes, tree, alp, want_moves=True, **kw)
    w0 = time.perf_counter() - t0
    leaves = {}

    def below(tr, k):
        if k not in leaves:
            leaves[k] = [k] if tr.left[k] < 0 else below(tr, tr.left[k]) + below(tr, tr.right[k])
        return leaves[k]

    def sides0(i):
        ins = sorted(below(tree, s0[i]["branch"]))
        out = [m for m in range(many) if m not in set(ins)]
        return (ins, out, None) if len(out) < len(ins) else (out, ins, None)
    c0, m0 = cells_of(codes, s0, st0["moves"], sides0)
    assert np.array_equal(m0, f0), "the host replay of g2g_refine's moves does not end in its MSA"
    r0 = summary("refine", w0, codes, f0, s0, st0, c0)
    # ---- the default run
    t0 = time.perf_counter()
    if plan is None:
        plan = guide.refine_plan(ctx, codes, tree, pprm, 35., weight)
    w_plan = time.perf_counter() - t0
    f1, s1, rs1, st1 = refine.refine_planned(ctx, codes, tree, prm, 35., weight, plan, want_moves=True, **kw)
    w1 = time.perf_counter() - t0
    step_range = {}
    for r in rs1:
        for i in range(r["first_step"], r["first_step"] + r["nsteps"]):
            step_range[i] = r["range"]

    def sides1(i):
        r = step_range[i]
        rel = plan.relations[r]
        lv = {}

        def bl(k):
            if k not in lv:
                lv[k] = [k] if rel.left[k] < 0 else bl(int(rel.left[k])) + bl(int(rel.right[k]))
            return lv[k]
        ins = set(bl(s1[i]["branch"]))
        a_ = [int(m) for g in range(len(rel.groups)) if g in ins for m in rel.groups[g]]
        b_ = [int(m) for g in range(len(rel.groups)) if g not in ins for m in rel.groups[g]]
        return a_, b_, (int(plan.ranges[r][0]), int(plan.ranges[r][1]))
    c1, m1 = cells_of(codes, s1, st1["moves"], sides1)
    assert np.array_equal(m1, f1), "the host replay of g2g_refine_planned's moves does not end in its MSA"
    r1 = summary("refine_planned", w1, codes, f1, s1, st1, c1)
    r1.update(plan_s=round(w_plan, 3), whole_groups=len(plan.whole.groups), ranges=np.asarray(plan.ranges).tolist(),
              groups_per_range=[len(r.groups) for r in plan.relations], steps_per_range=[r["nsteps"] for r in rs1])
    if ctx is not None:
        ctx.close()
    res = {"tool": "tools/refine_plan_probe.py", "msa": "clustered%dx%d_gapped" % (a.clusters, a.per), "members": many, "columns": ln,
           "scoring": "CPU checker" if a.checker else "GPU", "timing": "wall clock of each call, one run each in one process after a warm-up call",
           "runs": [r0, r1]}
    print(json.dumps(res), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
