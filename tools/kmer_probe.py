#!/usr/bin/env python3
"""Times the k-mer composition distances (g2g_kmer_dist_batch) on the GPU box, with the DP distances of the same family beside them:

  profile_ms   g2g_kmer_profile_kernel alone (words, sort, run compaction: one workgroup per sequence), HIP events on the context's
               stream (context option KMER_TIMING), median of 10 warm runs
  pairs_ms     g2g_kmer_allpairs_kernel alone (all pairs), same events, same runs
  call_ms      g2g_kmer_dist_batch as a caller sees it: device allocation, upload, both kernels, download of 12 bytes per pair,
               the closed forms on the host; wall clock, median of the same runs
  alnscored_ms guide.distance_matrix (one banded alnScoreD DP per pair, wall clock, second of two runs) -- 256 family only

Shapes: the bench family (make_family(256, 1024, 1), protein, k = 5 / Qpamd: the defaults) and a 4096-member family of 1024
residues (members mutated from one ancestor at rates spread over 5 .. 60 %, no indels; seeded numpy).  The counts of a sample of
pairs are checked against the Python restatement (tests/kmerlib.py) in the same run.
Usage: python tools/kmer_probe.py [--out profiles/NAME.json] [--shapes 256,4096]"""
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


def probe(ctx, name, seqs, reps=10):
    import kmerlib
    from prrn_aln_amd import guide
    prof, pairs, call = [], [], []
    for r in range(reps + 2):                                           # two warm-up runs: code object load, first allocation
        t0 = time.perf_counter()
        dist, counts = guide.kmer_distance(ctx, seqs, 1, want_counts=True)
        dt = (time.perf_counter() - t0) * 1e3
        if r >= 2:
            call.append(dt)
            prof.append(float(ctx.get_option("KMER_PROFILE_MS")))
            pairs.append(float(ctx.get_option("KMER_PAIRS_MS")))
    n = len(seqs)
    rng = np.random.default_rng(1)
    ia, ib = rng.integers(0, n, 200), rng.integers(0, n, 200)
    keep = ia < ib
    want = kmerlib.counts_pairs(seqs, 1, 0, ia[keep], ib[keep]) if n <= 256 else None
    if want is None:                                                    # (profiles of the sampled members only)
        ids = sorted(set(ia[keep]) | set(ib[keep]))
        at = {m: i for i, m in enumerate(ids)}
        want = kmerlib.counts_pairs([seqs[m] for m in ids], 1, 0, [at[a] for a in ia[keep]], [at[b] for b in ib[keep]])
    got = np.array([counts[kmerlib.elem(int(a), int(b))] for a, b in zip(ia[keep], ib[keep])])
    unq = np.array([len(np.unique(kmerlib.profile(s, 1, 5)[0])) for s in seqs[:64]])
    med = statistics.median
    return {"shape": name, "members": n, "residues": int(np.median([len(s) for s in seqs])), "pairs": n * (n - 1) // 2,
            "k": 5, "measure": "Qpamd", "distinct_words_median_of_64": int(np.median(unq)),
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
    a = ap.parse_args()
    from prrn_aln_amd import engine
    ctx = engine.Context()
    ctx.set_option("KMER_TIMING", 1)
    rows = []
    for s in a.shapes.split(","):
        if s == "256":
            seqs = bench_family()
            r = probe(ctx, "bench family make_family(256, 1024, 1)", seqs)
            r["alnscored_distance_matrix_ms"] = alnscored(ctx, seqs)
        else:
            r = probe(ctx, "synthetic %s x 1024" % s, synthetic(int(s), 1024, int(s)))
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
