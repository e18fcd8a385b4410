"""Live check of the oracle against the real reference (oracle/_ref) on seeded random families.
Where oracle/_ref is not built, the same divisions are built by the product's host builders and the oracle is held to the
reference's outputs recorded in tests/golden/live/ (tools/make_live_golden.py).  One subprocess per parameter set: the
reference keeps its parameters in globals."""
import os
import subprocess
import sys

import pytest

import refdump

WORKER = r'''
import sys, json
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
import numpy as np
import refdump, oraclelib
from prrn_aln_amd import _abi
from prrn_aln_amd.synth import make_family, tree_branches, tree_weights, drop_common_gaps, DNA, PROTEIN
molc, ls, nseq, length, seed, weighted = {args!r}
R = refdump.RefLib(molc=molc, ls=ls)
L = oraclelib.load()
fam = make_family(nseq, length, seed, alphabet=(DNA if molc == 2 else PROTEIN), indel=0.02)
w = tree_weights(fam.tree, nseq) if weighted else None
bad = []
modes = set()
for b in tree_branches(fam.tree):
    o = [i for i in range(nseq) if i not in b]
    ra = drop_common_gaps([fam.msa[i] for i in b]); rb = drop_common_gaps([fam.msa[i] for i in o])
    ga = R.group([fam.names[i] for i in b], ra, [w[i] for i in b] if w else None)
    gb = R.group([fam.names[i] for i in o], rb, [w[i] for i in o] if w else None)
    d = R.align_dump(ga, gb)
    modes.add(int(d["alnmode"][0]))
    h = _abi.problem_from_arrays(d)
    scr, cells, tr = oraclelib.forward(L, h)
    skl = oraclelib.stdskl(L, tr)
    if scr != d["scr"][0] or not np.array_equal(tr, d["vmf_trace"]) or not np.array_equal(skl, d["align2_skl"]):
        bad.append(len(b))
    R.free(ga); R.free(gb)
print(json.dumps({{"bad": bad, "modes": sorted(modes)}}))
'''

# the same divisions without the reference: inputs from the host builders (bit-identical to the reference's,
# tests/test_host_builders.py), outputs recorded from the reference
RECORDED = r'''
import sys, json
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/tests")
import numpy as np
import oraclelib
from prrn_aln_amd import operator as op
from prrn_aln_amd.synth import make_family, tree_branches, tree_weights, drop_common_gaps, DNA, PROTEIN
molc, ls, nseq, length, seed, weighted = {args!r}
L = oraclelib.load()
alp = op.AlnParam(molc=molc, max_code=25 if molc == 1 else 17, **({{"ls": ls}} if ls else {{}}))
g = np.load({gold!r})
fam = make_family(nseq, length, seed, alphabet=(DNA if molc == 2 else PROTEIN), indel=0.02)
w = tree_weights(fam.tree, nseq) if weighted else None
bad = []
modes = set()
branches = tree_branches(fam.tree)
assert len(g.files) == 3 * len(branches), (len(g.files), len(branches))
class H:
    def __init__(self, c): self.c = c
for j, b in enumerate(branches):
    o = [i for i in range(nseq) if i not in b]
    ra = drop_common_gaps([fam.msa[i] for i in b]); rb = drop_common_gaps([fam.msa[i] for i in o])
    pw = op.PwdM([op.mSeq(ra, alp, [w[i] for i in b] if w else None), op.mSeq(rb, alp, [w[i] for i in o] if w else None)], alp)
    modes.add(int(pw.problem.alnmode))
    scr, cells, tr = oraclelib.forward(L, H(pw.problem))
    skl = oraclelib.stdskl(L, tr)
    k = "b%03d_" % j
    if scr != g[k + "scr"][0] or not np.array_equal(tr, g[k + "trace"]) or not np.array_equal(skl, g[k + "skl"]):
        bad.append(len(b))
print(json.dumps({{"bad": bad, "modes": sorted(modes)}}))
'''

CASES = [
    (1, 0, 20, 90, 101, True),
    (1, 0, 9, 70, 102, False),
    (1, 3, 14, 80, 103, True),
    (2, 3, 12, 120, 104, True),
    (2, 0, 6, 100, 105, False),
]


IDS = ["prot20w", "prot9", "prot14_ls3", "dna12_ls3", "dna6"]


@pytest.mark.parametrize("args", CASES, ids=IDS)
def test_live(args):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if refdump.available():
        src = WORKER.format(root=root, args=args)
    else:
        gold = os.path.join(root, "tests", "golden", "live", IDS[CASES.index(args)] + ".npz")
        src = RECORDED.format(root=root, args=args, gold=gold)
    out = subprocess.check_output([sys.executable, "-c", src], stderr=subprocess.DEVNULL, timeout=600)
    import json
    r = json.loads(out.decode().strip().splitlines()[-1])
    assert r["bad"] == [], r
