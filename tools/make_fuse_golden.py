#!/usr/bin/env python3
"""Generate tests/golden/fuse/*.npz from the REAL reference (oracle/_ref): what IterMsa::preprrn decides before it refines
(src/prrn5.cc:794-823) on small MSAs, through the reference's own ConservedT::mayfuse, Ssrel::consregss and Ssrel::consreg
(src/consreg.cc:452-464, 692-711, 484-518), called in oracle/_ref/libprrn_ref.so through ctypes by their mangled names, one process
per case (the reference keeps its parameters in process globals).

Route: a zero-filled block is a default Ssrel; consreg builds its ss and ktree, and the tree is read out of the Ktree (with vol / cur).
mayfuse reads no member of its object: any block serves as `this`.  consregss takes sqs = {msd, scratch, scratch, 0}, the two scratch
mSeqs made by extseq(msd, NULL, ...).  For a column range sqs[0] is the slice read as its own group with the same weights: extseq
copies [left, right) only (src/seq.cc:1096-1118), so this is what restrange + consregss computes.  The grouped consreg is consreg
called with the Ssrel consregss returned as `this`.  Subset: {int** group; int* pool; int num; int elms} (src/sets.h:27-31).

Data only: codes, weights, u / v / thr, similarity matrix number 1, the tree; every fuse test of the whole-MSA walk in the reference's
order (two member lists, outcome, alnmode of the library's host-built pair); the fused subset and tree; the grouped consreg ranges
for dissim 0 and 1; per attack range its tests, fused subset and tree.

Before a case is saved
  - the tool's own post-order walk with mayfuse must reproduce consregss's groups (whole MSA and every range);
  - the restatement (tests/fuselib.py) must reproduce every outcome, subset, tree and range list;
  - the case must pin something: a test that fuses, a test that is refused, 1 < groups < leaves (the cases made to be all fused /
    none fused are exempt).
Usage: python tools/make_fuse_golden.py [case]            (needs oracle/_ref, i.e. the reference's sources at build time)
       python tools/make_fuse_golden.py --time [repeats]  the reference's consregss + grouped consreg + per-range consregss on
                                                          tests/golden/msa/prog256x1024.npz and on the largest fixture, wall clock on
                                                          one core, as one JSON line"""
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden", "fuse")
MAYFUSE = "_ZN10ConservedT7mayfuseEPP4mSeq"
CONSREGSS = "_ZN5Ssrel9consregssEPP4mSeq"
CPY_SEQ = 1
_AA = "ARNDCQEGHILKMFPSTWYV"
_NT = "ACGT"


def reference(molc):
    import make_consreg_golden as mc
    ref = mc.Ref(molc)
    ref.mayfuse = getattr(ref.L, MAYFUSE)
    ref.mayfuse.restype = C.c_bool
    ref.mayfuse.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    ref.consregss = getattr(ref.L, CONSREGSS)
    ref.consregss.restype = C.c_void_p
    ref.consregss.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
    return ref


def read_tree(ssrel_addr, n):
    """Ssrel::ktree (byte 8) -> Ktree::lead (byte 48) -> Knode[2 n - 1] (phyl.h:115-126, 80 bytes: left / right / parent, tid at byte
    24, vol at 48, cur at 56): (left, right, parent, vol, cur)"""
    kt = C.cast(ssrel_addr + 8, C.POINTER(C.c_void_p))[0]
    assert kt
    lead = C.cast(kt + 48, C.POINTER(C.c_void_p))[0]
    root = C.cast(kt + 56, C.POINTER(C.c_void_p))[0]
    nn = 2 * n - 1
    idx = np.full((3, nn), -1, np.int32)
    vc = np.zeros((2, nn))
    for k in range(nn):
        node = lead + 80 * k
        assert C.cast(node + 24, C.POINTER(C.c_int))[0] == k
        for f in range(3):
            p = C.cast(node + 8 * f, C.POINTER(C.c_void_p))[0]
            if p:
                assert (p - lead) % 80 == 0 and 0 <= (p - lead) // 80 < nn
                idx[f, k] = (p - lead) // 80
        vc[0, k] = C.cast(node + 48, C.POINTER(C.c_double))[0]
        vc[1, k] = C.cast(node + 56, C.POINTER(C.c_double))[0]
    assert (root - lead) // 80 == nn - 1 and idx[2, nn - 1] == -1
    return idx[0], idx[1], idx[2], vc[0], vc[1]


def read_subset(ssrel_addr):
    ss = C.cast(ssrel_addr, C.POINTER(C.c_void_p))[0]
    assert ss
    grp = C.cast(C.cast(ss, C.POINTER(C.c_void_p))[0], C.POINTER(C.c_void_p))
    num = C.cast(ss + 16, C.POINTER(C.c_int))[0]
    out = []
    for g in range(num):
        p = C.cast(grp[g], C.POINTER(C.c_int))
        lst = []
        while p[len(lst)] >= 0:
            lst.append(p[len(lst)])
        out.append(lst)
    return out


class Msa:
    """the reference's mSeq of some columns of the rows, with two scratch mSeqs for consregss / mayfuse"""

    def __init__(self, ref, rows, weight, left=0, right=None):
        self.ref = ref
        rows = [r[left:right] for r in rows]
        self.sd = ref.R.group(["m%d" % i for i in range(len(rows))], rows, weight)
        assert ref.L.ref_group_many(self.sd) == len(rows) and ref.L.ref_group_len(self.sd) == len(rows[0])
        self.scratch = [self.extract(list(range(len(rows)))) for _ in range(2)]

    def extract(self, lst):
        arr = (C.c_int * (len(lst) + 1))(*(list(lst) + [-1]))
        return self.ref.extseq(self.sd, None, arr, CPY_SEQ, 1.0)

    def may_fuse(self, l0, l1):
        sons = (C.c_void_p * 2)(self.extract(l0), self.extract(l1))
        this = (C.c_char * 256)()
        r = bool(self.ref.mayfuse(C.addressof(this), sons))
        for s in sons:
            self.ref.L.ref_group_free(s)
        return r

    def consregss(self, ssrel_addr):
        sqs = (C.c_void_p * 4)(self.sd, self.scratch[0], self.scratch[1], None)
        return self.ref.consregss(ssrel_addr, sqs)


def fuse_ref(msa, srl_addr, rel):
    """consregss of the reference on msa over the relation at srl_addr (= rel): (address or None, fused, relation, tests of the tool's own walk)"""
    import fuselib as fl
    tests = []

    def test(l0, l1):
        f = msa.may_fuse(l0, l1)
        tests.append((list(l0), list(l1), int(f)))
        return f
    own, leaf = fl.testssrel(rel[0], rel[1], rel[2], rel[3], test)
    trl = msa.consregss(srl_addr)
    if not trl:
        assert len(own) == len(rel[0]), "consregss fused nothing, the tool's walk did"
        return None, 0, rel, tests
    got = read_subset(trl)
    assert got == own, "the tool's own walk with mayfuse gives %s, consregss %s" % (own, got)
    return trl, 1, (got,) + read_tree(trl, len(got)), tests


def same_rel(a, b):
    return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4])) and all(np.array_equal(np.asarray(x).view(np.int64), np.asarray(y).view(np.int64)) for x, y in zip(a[4:6], b[4:6]))


def run(name, molc, rows, u=-1., v=-1., thr=35., weight=None, exempt=False, want_two_rounds=False, want_modes=(), save=True):
    import consreglib as cl
    import fuselib as fl
    from prrn_aln_amd import operator as op
    ref = reference(molc)
    simmtx = ref.matrix(1)
    codes = op.encode(rows, molc)
    ln, many = codes.shape
    ref.set_localprm(u, v, thr)
    uu, vv = float(np.float32(3. if u < 0 else u)), float(np.float32(10. if v < 0 else v))      # ALPRM holds floats
    whole = Msa(ref, rows, weight)
    ssrel = (C.c_char * 256)()
    ref.consreg(C.addressof(ssrel), whole.sd, 1)
    tree = read_tree(C.addressof(ssrel), many)
    g = dict(molc=np.array([molc], np.int32), max_code=np.array([25 if molc == 1 else 17], np.int32), u=np.array([uu]), v=np.array([vv]), simmtx=simmtx)
    alp = cl.alp_of(g)
    rel0 = ([[m] for m in range(many)],) + tree
    rrl, fused, srl, tests = fuse_ref(whole, C.addressof(ssrel), rel0)
    # the restatement: every outcome, the subset, the tree
    mine = []
    m_fused, m_rel, m_org = fl.consregss(codes, rel0, alp, weight, tests=mine)
    assert [(a, b, f) for a, b, f, _, _ in mine] == tests, "the restatement's tests differ: %s against %s" % ([(a, b, f) for a, b, f, _, _ in mine], tests)
    assert m_fused == fused and same_rel(m_rel, srl), "the restatement's relation differs"
    modes = [t[4] for t in mine]
    srl_addr = rrl if rrl else C.addressof(ssrel)
    united, ranges_rel = [[], []], []
    if len(srl[0]) >= 2:
        for dissim in (0, 1):
            united[dissim] = ref.ranges(ref.consreg(srl_addr, whole.sd, dissim))
            assert fl.consreg_groups(codes, srl, alp, thr, weight, bool(dissim)) == united[dissim], "the restatement's grouped consreg differs (dissim %d)" % dissim
        for l, r in united[1]:
            part = Msa(ref, rows, weight, l, r)
            trl, f, rel, t = fuse_ref(part, srl_addr, srl)
            pm = []
            mf, mr, mo = fl.consregss(codes, srl, alp, weight, l, r, tests=pm)
            assert [(a, b, x) for a, b, x, _, _ in pm] == t and mf == f and same_rel(mr, rel), "the restatement differs inside [%d, %d)" % (l, r)
            modes += [x[4] for x in pm]
            ranges_rel.append((f, rel, pm))
    n_fuse = sum(t[2] for t in tests)
    pins = (n_fuse >= 1 and n_fuse < len(tests) and 1 < len(srl[0]) < many) or exempt
    two = any(f for f, _, _ in ranges_rel)
    seen = {cl.MODE_NAME[m] + str(m) + ("+" if f else "-"): 0 for (_, _, f, _, m) in mine + [x for _, _, pm in ranges_rel for x in pm]}
    print("%-20s %2d x %3d: %2d tests, %2d fuse, %d groups, ranges %s, fused inside %s, modes %s, stops %s"
          % (name, many, ln, len(tests), n_fuse, len(srl[0]), united[1], [f for f, _, _ in ranges_rel], sorted(seen), [c for _, _, _, c, _ in mine]))
    assert pins, "%s pins nothing" % name
    assert two or not want_two_rounds, "%s: nothing fuses inside a range" % name
    for w in want_modes:
        assert w in seen, "%s: no test %s" % (name, w)
    if not save:
        return
    cat = lambda xs, dt: (np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs]) if xs else np.zeros(0, dt))
    offs = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
    out = dict(g, codes=codes, weight=np.asarray(weight if weight is not None else [], np.float64), thr=np.array([float(thr)]),
               gunited0=np.asarray(united[0], np.int32).reshape(-1, 2), gunited1=np.asarray(united[1], np.int32).reshape(-1, 2),
               nrange=np.array([len(ranges_rel)], np.int32))

    def put_tests(pfx, ts):
        """(list0, list1, outcome, stop_col, alnmode) of the restatement, checked against the reference's outcomes above"""
        for s, key in ((0, "_l0"), (1, "_l1")):
            out[pfx + key], out[pfx + key + "_off"] = cat([t[s] for t in ts], np.int32), offs([t[s] for t in ts])
        out[pfx + "_fuse"], out[pfx + "_mode"] = np.array([t[2] for t in ts], np.int32), np.array([t[4] for t in ts], np.int32)

    put_tests("test", mine)

    def put(pfx, f, rel):
        out[pfx + "_fused"] = np.array([f], np.int32)
        if f:
            out[pfx + "_grp"], out[pfx + "_grp_off"] = cat(rel[0], np.int32), offs(rel[0])
            for k, a in zip(("left", "right", "parent", "vol", "cur"), rel[1:]):
                out["%s_%s" % (pfx, k)] = a
    for k, a in zip(("left", "right", "parent", "vol", "cur"), tree):
        out["tree_" + k] = a
    put("whole", fused, srl)
    for i, (f, rel, pm) in enumerate(ranges_rel):
        put("r%d" % i, f, rel)
        put_tests("r%d_test" % i, pm)
    os.makedirs(GOLD, exist_ok=True)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)


# ---- families ------------------------------------------------------------------------------------------------------------------------
def clustered(sizes, length, seed, blocks, within=0.04, alphabet=_AA, gaps=0.0, shared_del=None, private_del=None):
    """clusters of sizes[c] members over one ancestor.  blocks: (left, right, clusters) -- inside the block those clusters carry an
    ancestor of their own (every column substituted); member m of a cluster has within * (1 + m) of its columns substituted.
    gaps: the fraction of positions at which a random gap run of 1 .. 4 columns starts.  shared_del: {cluster: [(left, right)]}
    columns deleted in every member of the cluster; private_del: {member: [(left, right)]} columns deleted in that member."""
    rng = np.random.default_rng(seed)
    na = len(alphabet)
    anc = rng.integers(0, na, length)
    rows = []
    for c, size in enumerate(sizes):
        ca = anc.copy()
        for l, r, which in blocks:
            if c in which:
                ca[l:r] = (ca[l:r] + 1 + rng.integers(0, na - 1, r - l)) % na
        for m in range(size):
            s = ca.copy()
            hit = rng.random(length) < within * (1 + m)
            s[hit] = rng.integers(0, na, int(hit.sum()))
            row = [alphabet[x] for x in s]
            for p in np.flatnonzero(rng.random(length) < gaps):
                for q in range(p, min(length, p + int(rng.integers(1, 5)))):
                    row[q] = "-"
            for l, r in (shared_del or {}).get(c, []):
                row[l:r] = "-" * (r - l)
            for l, r in (private_del or {}).get(len(rows), []):
                row[l:r] = "-" * (r - l)
            rows.append("".join(row))
    return rows


def timed(repeats):
    import fuselib as fl
    out = {}
    big = np.load(os.path.join(ROOT, "tests", "golden", "msa", "prog256x1024.npz"))["codes"]
    fx = max(fl.fixtures(), key=lambda ng: ng[1]["codes"].size)
    ref = reference(1)
    dec = np.array(list("?-X" + _AA + "BZ"))
    for name, codes in (("prog256x1024", big), (fx[0], fx[1]["codes"])):
        if int(fx[1]["molc"][0]) != 1 and name != "prog256x1024":
            continue
        rows = ["".join(dec[codes[:, m]]) for m in range(codes.shape[1])]
        whole = Msa(ref, rows, None)
        ts, info = [], {}
        for r in range(repeats + 1):
            ssrel = (C.c_char * 256)()
            ref.consreg(C.addressof(ssrel), whole.sd, 1)                       # builds ss and ktree (not timed)
            t0 = time.perf_counter()
            rrl = whole.consregss(C.addressof(ssrel))
            t1 = time.perf_counter()
            srl = rrl if rrl else C.addressof(ssrel)
            atk = ref.ranges(ref.consreg(srl, whole.sd, 1))
            t2 = time.perf_counter()
            inside = 0
            for l, rr in atk:
                part = Msa(ref, rows, None, l, rr)
                t3 = time.perf_counter()
                part.consregss(srl)
                inside += time.perf_counter() - t3
            ts.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3, inside * 1e3))
            info = {"groups": len(read_subset(srl)), "ranges": [list(x) for x in atk]}
        ts = np.array(ts[1:])
        out[name] = dict(info, members=codes.shape[1], columns=codes.shape[0], runs=repeats, consregss_ms=round(float(np.median(ts[:, 0])), 3),
                         grouped_consreg_ms=round(float(np.median(ts[:, 1])), 2), per_range_consregss_ms=round(float(np.median(ts[:, 2])), 3))
    print(json.dumps({"reference_preprrn_decisions_one_core": out}))


W12 = [0.4 + 0.1 * ((7 * i) % 13) for i in range(12)]
B3 = [(0, 38, (1, 2)), (71, 150, (2,)), (71, 110, (1,))]
JOBS = {
    # three clusters of four, no gap: NGP tests at the leaves, profile modes above; the join of two clusters is refused
    "clusters": lambda: run("prot12_clusters", 1, clustered([4, 4, 4], 150, 11, B3)),
    # clusters that share a deletion: their sons carry all-gap columns, groups with gap profiles still fuse
    "shared_del": lambda: run("prot12_shared_del", 1, clustered([4, 4, 4], 180, 12, [(0, 50, (1,)), (90, 180, (2,))], shared_del={0: [(60, 66)], 1: [(20, 24), (120, 127)], 2: [(100, 103)]})),
    # small and gapped enough for the naive records
    "nv": lambda: run("prot6_nv", 1, clustered([2, 2, 2], 140, 13, [(0, 45, (1,)), (80, 140, (2,))], private_del={0: [(20, 21)], 3: [(60, 61)], 4: [(100, 101)]}), want_modes=("nv10+", "nv10-")),
    "dna": lambda: run("dna9_clusters", 2, clustered([3, 3, 3], 240, 14, [(0, 80, (1,)), (130, 240, (2,))], alphabet=_NT, within=0.02, shared_del={1: [(30, 36)], 2: [(150, 158)]})),
    "weighted": lambda: run("prot12_weighted", 1, clustered([4, 4, 4], 160, 15, B3, gaps=0.01), weight=W12),
    "uv": lambda: run("prot10_u21_v93", 1, clustered([4, 3, 3], 200, 16, [(0, 60, (1,)), (120, 200, (2,))], private_del={1: [(30, 31)], 5: [(90, 91)], 8: [(150, 151)]}), u=2.1, v=9.3),
    # whole-MSA fusing, then further fusing inside a range: clusters 0 and 1 differ in [0, 45) only
    "two_rounds": lambda: run("prot12_two_rounds", 1, clustered([4, 4, 4], 220, 17, [(0, 45, (1,)), (0, 45, (2,)), (120, 220, (2,))]), want_two_rounds=True),
    "all_fused": lambda: run("prot8_all_fused", 1, clustered([4, 4], 120, 18, [], within=0.01), exempt=True),
    "none_fused": lambda: run("prot6_none_fused", 1, clustered([1] * 6, 130, 19, [(0, 130, (1,)), (0, 130, (2,)), (0, 130, (3,)), (0, 130, (4,)), (0, 130, (5,))]), exempt=True),
    # two clusters of eight, each with a shared deletion and two halves with a deletion of their own: gap profiles on both sides
    "gapped16": lambda: run("prot16_gapped", 1, clustered([8, 8], 400, 20, [(0, 90, (1,))], within=0.01, shared_del={0: [(100, 104)], 1: [(300, 305)]},
                                                          private_del=dict([(m, [(50, 51)]) for m in range(4)] + [(m, [(150, 151)]) for m in range(4, 8)]
                                                                           + [(m, [(250, 251)]) for m in range(8, 12)] + [(m, [(350, 351)]) for m in range(12, 16)])),
                            want_modes=("pf9+",)),
}

if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--time":
        timed(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    elif len(sys.argv) > 1:
        JOBS[sys.argv[1]]()
    else:
        for j in JOBS:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), j])
