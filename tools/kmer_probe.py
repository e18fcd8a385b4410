#!/usr/bin/env python3
"""Times the k-mer composition distances (g2g_kmer_dist_batch) on the GPU box, with the DP distances of the same family beside them:

  profile_ms   g2g_kmer_profile_kernel alone (words, sort, run compaction: one workgroup per sequence), HIP events on the context's
               stream (context option KMER_TIMING), median of 10 warm runs
  pairs_ms     g2g_kmer_allpairs_kernel alone (all pairs), same events, same runs
  call_ms      g2g_kmer_dist_batch as a caller sees it: device allocation, upload, both kernels, download of 12 bytes per pair,
               the closed forms on the host; wall clock, median of the same runs
  alnscored_ms guide.distance_matrix (one banded alnScoreD DP per pair, wall clock, second of two runs) -- 256 family only

With --nalpha / --k / --seed the same shapes are timed again through g2g_kmer_dist_batch_spec (g2g_kmer_profile_spec_kernel): once
with the continuous seed of k over nalpha classes and once under every seed given; the full-alphabet default stays the first row of
each shape.  The classification is --classes, or the pattern a fixture of tests/golden/kmer_spec records for that nalpha.

Shapes: the bench family (make_family(256, 1024, 1), protein, k = 5 / Qpamd: the defaults) and a 4096-member family of 1024
residues (members mutated from one ancestor at rates spread over 5 .. 60 %, no indels; seeded numpy).  The counts of a sample of
pairs are checked against the Python restatement (tests/kmerlib.py) in the same run.
Usage: python tools/kmer_probe.py [--out profiles/NAME.json] [--shapes 256,4096] [--nalpha 14 --k 4 [--seed 1011,110101] [--classes PATTERN]]"""
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


def bench_family():
    from prrn_aln_amd import operator as op
    from prrn_aln_amd.synth import make_family
    fam = make_family(256, 1024, 1)
    return [op.encode([r.replace("-", "")], op.PROTEIN)[:, 0].copy() for r in fam.msa]


def synthetic(many, ln, seed):
    rng = np.random.default_rng(seed)
    anc = rng.integers(3, 23, ln).astype(np.uint8)
    rate = rng.uniform(0.05, 0.6, many)
    out = []
    for m in range(many):
        s = anc.copy()
        mut = rng.random(ln) < rate[m]
        s[mut] = rng.integers(3, 23, int(mut.sum())).astype(np.uint8)
        out.append(s)
    return out


def recorded_pattern(nalpha):
    import kmerspeclib as ks
    for _, g in ks.fixtures():
        c = ks.case(g)
        if c["molc"] == 1 and c["nalpha"] == nalpha:
            return c["classes"]
    raise SystemExit("no fixture of tests/golden/kmer_spec records a protein pattern for nalpha %d: give --classes" % nalpha)


def probe(ctx, name, seqs, reps=10, spec=None):
    """spec: None for g2g_kmer_dist_batch with the defaults, else (nalpha, k, classes, seed) for g2g_kmer_dist_batch_spec"""
    import kmerlib
    import kmerspeclib as ks
    from prrn_aln_amd import guide
    if spec is None:
        run = lambda: guide.kmer_distance(ctx, seqs, 1, want_counts=True)
        want_counts = lambda sq, a, b: kmerlib.counts_pairs(sq, 1, 0, a, b)
        words = lambda s: kmerlib.profile(s, 1, 5)[0]
        k, entry = 5, "g2g_kmer_dist_batch"
    else:
        nalpha, k, classes, seed = spec
        tab = ks.table(classes, 1)
        run = lambda: guide.kmer_distance_spec(ctx, seqs, 1, k, -1, nalpha, classes, seed, want_counts=True)
        want_counts = lambda sq, a, b: ks.counts_pairs(sq, 1, k, nalpha, classes, seed, a, b)
        words = lambda s: ks.profile(s, tab, nalpha, k, seed)[0]
        entry = "g2g_kmer_dist_batch_spec"
    prof, pairs, call = [], [], []
    for r in range(reps + 2):                                           # two warm-up runs: code object load, first allocation
        t0 = time.perf_counter()
        dist, counts = run()
        dt = (time.perf_counter() - t0) * 1e3
        if r >= 2:
            call.append(dt)
            prof.append(float(ctx.get_option("KMER_PROFILE_MS")))
            pairs.append(float(ctx.get_option("KMER_PAIRS_MS")))
    n = len(seqs)
    rng = np.random.default_rng(1)
    ia, ib = rng.integers(0, n, 200), rng.integers(0, n, 200)
    keep = ia < ib
    want = want_counts(seqs, ia[keep], ib[keep]) if n <= 256 else None
    if want is None:                                                    # (profiles of the sampled members only)
        ids = sorted(set(ia[keep]) | set(ib[keep]))
        at = {m: i for i, m in enumerate(ids)}
        want = want_counts([seqs[m] for m in ids], [at[a] for a in ia[keep]], [at[b] for b in ib[keep]])
    got = np.array([counts[kmerlib.elem(int(a), int(b))] for a, b in zip(ia[keep], ib[keep])])
    unq = np.array([len(words(s)) for s in seqs[:64]])
    med = statistics.median
    return {"shape": name, "members": n, "residues": int(np.median([len(s) for s in seqs])), "pairs": n * (n - 1) // 2,
            "entry": entry, "k": k or 5, "nalpha": spec[0] if spec else 20, "seed": (spec[3] if spec else None), "measure": "Qpamd", "distinct_words_median_of_64": int(np.median(unq)),
            "profile_ms": round(med(prof), 4), "profile_ms_min_max": [round(min(prof), 4), round(max(prof), 4)],
            "pairs_ms": round(med(pairs), 4), "pairs_ms_min_max": [round(min(pairs), 4), round(max(pairs), 4)],
            "call_ms": round(med(call), 3), "call_ms_min_max": [round(min(call), 3), round(max(call), 3)], "runs": reps,
            "sample_pairs_equal_restatement": bool(np.array_equal(got, want)), "sample_pairs": int(keep.sum()),
            "nan_pairs": int(np.isnan(dist).sum())}


def alnscored(ctx, seqs):
    from prrn_aln_amd import guide, operator as op
    alp = op.AlnParam()
    prm, keep = alp.to_c()
    ms = []
    for _ in range(2):
        t0 = time.perf_counter()
        guide.distance_matrix(ctx, prm, seqs, keep)
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(ms[1], 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--shapes", default="256,4096")
    ap.add_argument("--nalpha", type=int, default=0)
    ap.add_argument("--k", type=int, default=0)
    ap.add_argument("--seed", default="", help="comma-separated seed strings")
    ap.add_argument("--classes", default="", help="classification pattern; default: the one a kmer_spec fixture records for --nalpha")
    a = ap.parse_args()
    specs = []
    if a.nalpha or a.k or a.seed:
        nalpha = a.nalpha or 20
        classes = a.classes or (recorded_pattern(nalpha) if nalpha != 20 else None)
        specs = [(nalpha, a.k, classes, None)] + [(nalpha, a.k, classes, sd) for sd in a.seed.split(",") if sd]
    from prrn_aln_amd import engine
    ctx = engine.Context()
    ctx.set_option("KMER_TIMING", 1)
    rows = []
    for s in a.shapes.split(","):
        if s == "256":
            seqs, name = bench_family(), "bench family make_family(256, 1024, 1)"
        else:
            seqs, name = synthetic(int(s), 1024, int(s)), "synthetic %s x 1024" % s
        for spec in [None] + specs:
            r = probe(ctx, name, seqs, spec=spec)
            if s == "256" and spec is None:
                r["alnscored_distance_matrix_ms"] = alnscored(ctx, seqs)
            print(json.dumps(r), flush=True)
            rows.append(r)
    ctx.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump({"tool": "tools/kmer_probe.py",
                   "timing": "kernels: HIP events, median of 10 warm runs in one process; call / alnscored: wall clock", "rows": rows},
                  open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
