"""Generate tests/golden/live/<case>.npz: what the REFERENCE computes (align2 score, the DP trace, stdskl's skeleton) for every
tree-branch division of the seeded families of tests/test_oracle_vs_reference.py.  Where oracle/_ref is not built, that test
builds the same divisions with the product's host builders and holds the oracle to these recorded outputs.

Run where oracle/_ref is built (make -f oracle/Makefile.ref); one subprocess per case: the reference keeps its parameters in
globals.  Data only."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

WORKER = r'''
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
import numpy as np
import refdump
from prrn_aln_amd.synth import make_family, tree_branches, tree_weights, drop_common_gaps, DNA, PROTEIN
molc, ls, nseq, length, seed, weighted = {args!r}
R = refdump.RefLib(molc=molc, ls=ls)
fam = make_family(nseq, length, seed, alphabet=(DNA if molc == 2 else PROTEIN), indel=0.02)
w = tree_weights(fam.tree, nseq) if weighted else None
out = {{}}
for j, b in enumerate(tree_branches(fam.tree)):
    o = [i for i in range(nseq) if i not in b]
    ra = drop_common_gaps([fam.msa[i] for i in b]); rb = drop_common_gaps([fam.msa[i] for i in o])
    ga = R.group([fam.names[i] for i in b], ra, [w[i] for i in b] if w else None)
    gb = R.group([fam.names[i] for i in o], rb, [w[i] for i in o] if w else None)
    d = R.align_dump(ga, gb)
    out["b%03d_scr" % j] = d["scr"][:1]
    out["b%03d_trace" % j] = d["vmf_trace"]
    out["b%03d_skl" % j] = d["align2_skl"]
    R.free(ga); R.free(gb)
np.savez_compressed({path!r}, **out)
'''


def main():
    import refdump
    from test_oracle_vs_reference import CASES, IDS
    if not refdump.available():
        raise SystemExit("oracle/_ref is not built (make -f oracle/Makefile.ref)")
    gold = os.path.join(ROOT, "tests", "golden", "live")
    os.makedirs(gold, exist_ok=True)
    for args, name in zip(CASES, IDS):
        path = os.path.join(gold, name + ".npz")
        subprocess.check_call([sys.executable, "-c", WORKER.format(root=ROOT, args=args, path=path)], stderr=subprocess.DEVNULL)
        print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
