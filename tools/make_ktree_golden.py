#!/usr/bin/env python3
"""Generate tests/golden/ktree/*.json from the REAL reference: the weighting tree (Ssrel::calcweight: Ktree(msd) + calcpw) of the
edge-case MSAs of tests/test_ktree_host.py -- two members, three members, and families with duplicated members (zero distances:
heights of 0, res = fepsilon, the degenerate branch of Ktree::pairwt) -- as oracle/_ref/prrn5_trace writes it when Randiv is
constructed (the `T` lines, oracle/ref_trace.cc).  Data only: the MSA and topology / vol / cur of every node.
Usage: python tools/make_ktree_golden.py   (needs oracle/_ref, i.e. the reference's sources at build time)"""
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden", "ktree")
REF = os.path.join(ROOT, "oracle", "_ref")


def family(n_seq, length, seed, **kw):
    from prrn_aln_amd.synth import make_family
    return list(make_family(n_seq=n_seq, length=length, seed=seed, indel=0.05, max_indel=6, **kw).msa)


def cases():
    f6 = family(6, 60, 41)
    f4 = family(4, 50, 43)
    p2 = family(2, 60, 37)
    return [
        # prrn builds no weighting tree for two members (no Randiv is constructed: the trace holds no T line), so this one yields
        # no fixture; the nearest input it accepts is the same pair with its second member twice
        ("pair2", p2),
        ("pair2_refused_trio3_with_twin", [p2[0], p2[1], p2[1]]),
        ("trio3", family(3, 60, 39)),
        # members 1 and 2 repeat member 0, member 5 repeats member 4: zero distances inside and between two clusters
        ("dup8_two_clusters", [f6[0], f6[0], f6[0], f6[1], f6[2], f6[2], f6[3], f6[4]]),
        # every member twice
        ("dup8_all_twins", [r for r in f4 for _ in (0, 1)]),
    ]


def reference_tree(rows, molc=1):
    """the T lines of a traced run, or None if the reference refuses the input"""
    import refdump
    names = ["s%02d" % i for i in range(len(rows))]
    env = dict(os.environ, ALN_TAB=os.path.join(REF, "table"))
    with tempfile.TemporaryDirectory() as tmp:
        refdump.write_multi(os.path.join(tmp, "fam.msa"), names, list(rows), "fam")
        tr = os.path.join(tmp, "trace.txt")
        r = subprocess.run([os.path.join(REF, "prrn5_trace"), "-YH0", "-R1", "-I1", "-O4", "fam.msa"], cwd=tmp,
                           env=dict(env, G2G_TRACE=tr), capture_output=True, text=True)
        if r.returncode != 0 or not os.path.exists(tr):
            print("  reference refused: rc %d %s" % (r.returncode, r.stderr.strip()[:200]))
            return None
        T = [l.split() for l in open(tr) if l.startswith("T ")]
    T = T[:2 * len(rows) - 1]                                          # (the tree of the first Randiv: the start MSA's)
    if len(T) != 2 * len(rows) - 1:
        print("  no tree in the trace (%d T lines)" % len(T))
        return None
    assert [int(t[1]) for t in T] == list(range(len(T)))
    return {"left": [int(t[2]) for t in T], "right": [int(t[3]) for t in T], "parent": [int(t[4]) for t in T],
            "vol": [float(t[5]) for t in T], "cur": [float(t[6]) for t in T]}


def main():
    os.makedirs(GOLD, exist_ok=True)
    for name, rows in cases():
        print("%s: %d members x %d columns" % (name, len(rows), len(rows[0])))
        tree = reference_tree(rows)
        if tree is None:
            continue
        json.dump({"name": name, "molc": 1, "rows": rows, "tree": tree}, open(os.path.join(GOLD, name + ".json"), "w"))
        print("  root %d, cur of the leaves: %s" % (len(tree["left"]) - 1, " ".join("%.4g" % c for c in tree["cur"][:len(rows)])))


if __name__ == "__main__":
    main()
