#!/usr/bin/env python3
"""Generate tests/golden/ktree_groups/*.npz from the REAL reference (oracle/_ref): the weighting tree over given groups as
IterMsa::phyl_pwt builds it in the branch ss->num < ss->elms (src/prrn5.cc:343-391), on small MSAs.  phyl_pwt itself is a member
of a class the library cannot build from outside, so the tool composes its few lines from the reference's own parts, called in
oracle/_ref/libprrn_ref.so through ctypes by their mangled names:
  pairdvn(const Seq*, const int*, const int*)     the group divergence of every group pair (src/divseq.cc:65-105)
  mSeq::extseq + Ktree(Seq*) + Ktree::calcwt      per group of several members: its own tree, its members' weights, and the
                                                  root's height / res for the leaf
  Ktree(Seq*, Subset*, UPG_METHOD, Knode* lead)   the tree over the groups from the leaves the tool filled as phyl_pwt fills them
  Ktree::calcpw                                   its Kirchhoff weights
Knode is 80 bytes (phyl.h:115-126): left / right / parent at 0 / 8 / 16, tid 24, ndesc 28, height 32, length 40, vol 48, cur 56,
res 64.  Ktree holds lead at byte 48 and root at 56 (phyl.h:402-418).  Subset: {int** group; int* pool; int num; int elms}.

Data only: codes, groups, per group pair the reference's distance and the restatement's four counts (which give that distance bit
for bit), the leaves (ndesc, height, res), the members' weights inside their groups, the tree (all Knode fields) and the final
weights, for flat_leaves = 0 and 1.

Before a case is saved the restatement (tests/ktreegrouplib.py: literal loop AND closed form) must reproduce all of it bit for
bit, and the case must show what it was made for (see `want`).
Usage: python tools/make_ktree_groups_golden.py [case]      (needs oracle/_ref, i.e. the reference's sources at build time)
       python tools/make_ktree_groups_golden.py --time [large]   the reference's group pairdvn over all group pairs of
                                                            tests/golden/msa/prog256x1024.npz in 16 groups of 16 and in 128 pairs
                                                            (large: of tools/ktree_probe.py's 4096 x 5000 star in 64 groups of 64
                                                            and in 2048 pairs), wall clock on one core, one JSON line per input"""
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
GOLD = os.path.join(ROOT, "tests", "golden", "ktree_groups")
PAIRDVN_G = "_Z7pairdvnPK3SeqPKiS3_"
KTREE_SEQ = "_ZN5KtreeC1EP3SeqP6Subset7TreeMetP5Knode"
CALCWT = "_ZN5Ktree6calcwtEPd"
CALCPW = "_ZN5Ktree6calcpwEPd"
EXTSEQ = "_ZN4mSeq6extseqEPS_Piid"
CPY_SEQ, DEF_METHOD, UPG_METHOD, KNODE = 1, 0, 1, 80
EPS = 1.e-7
_AA = "ARNDCQEGHILKMFPSTWYV"
_NT = "ACGT"


class Ref:
    def __init__(self, molc):
        import refdump
        self.R = refdump.RefLib(molc=molc, band=True)
        L = self.L = self.R.lib
        self.pairdvn = getattr(L, PAIRDVN_G)
        self.pairdvn.restype = C.c_double
        self.pairdvn.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        self.ktree = getattr(L, KTREE_SEQ)
        self.ktree.restype = None
        self.ktree.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        self.calcwt = getattr(L, CALCWT)
        self.calcwt.restype = C.c_void_p
        self.calcwt.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self.calcpw = getattr(L, CALCPW)
        self.calcpw.restype = C.c_void_p
        self.calcpw.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        self.extseq = getattr(L, EXTSEQ)
        self.extseq.restype = C.c_void_p
        self.extseq.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_double]
        self.keep = []                                               # blocks the reference's objects point into: never freed, never destructed

    @staticmethod
    def ilist(lst):
        return (C.c_int * (len(lst) + 1))(*([int(x) for x in lst] + [-1]))

    def group_dist(self, sd, groups):
        lists = [self.ilist(g) for g in groups]
        out = np.zeros(len(groups) * (len(groups) - 1) // 2)
        k = 0
        for j in range(1, len(groups)):
            for i in range(j):
                out[k] = self.pairdvn(sd, lists[i], lists[j])
                k += 1
        return out

    def read_nodes(self, kt_addr, n):
        """every Knode of a Ktree of n leaves as a dict of arrays, and the root's index"""
        lead = C.cast(kt_addr + 48, C.POINTER(C.c_void_p))[0]
        root = C.cast(kt_addr + 56, C.POINTER(C.c_void_p))[0]
        nn = 2 * n - 1
        t = {k: np.full(nn, -1, np.int32) for k in ("left", "right", "parent")}
        t["ndesc"] = np.zeros(nn, np.int32)
        for k in ("height", "length", "vol", "cur", "res"):
            t[k] = np.zeros(nn)
        for k in range(nn):
            node = lead + KNODE * k
            assert C.cast(node + 24, C.POINTER(C.c_int))[0] == k
            for f, key in enumerate(("left", "right", "parent")):
                p = C.cast(node + 8 * f, C.POINTER(C.c_void_p))[0]
                if p:
                    assert (p - lead) % KNODE == 0 and 0 <= (p - lead) // KNODE < nn
                    t[key][k] = (p - lead) // KNODE
            t["ndesc"][k] = C.cast(node + 28, C.POINTER(C.c_int))[0]
            for off, key in ((32, "height"), (40, "length"), (48, "vol"), (56, "cur"), (64, "res")):
                t[key][k] = C.cast(node + off, C.POINTER(C.c_double))[0]
        r = (root - lead) // KNODE
        assert r == nn - 1 and t["parent"][r] == -1
        return t, int(r)

    def new_tree(self, sd, subset=None, method=DEF_METHOD, lead=None):
        obj = (C.c_char * 512)()
        self.keep.append(obj)
        self.ktree(C.addressof(obj), sd, subset, method, lead)
        return C.addressof(obj)

    def subtree(self, sd, gr):
        """Ktree subtree(extseq(group)); subtree.calcwt(swt): (weights, root height, root res)"""
        tmp = self.extseq(sd, None, self.ilist(gr), CPY_SEQ, 1.0)
        kt = self.new_tree(tmp)
        swt = (C.c_double * len(gr))()
        self.calcwt(kt, swt)
        t, r = self.read_nodes(kt, len(gr))
        return list(swt), float(t["height"][r]), float(t["res"][r])

    def group_tree(self, sd, groups, ndesc, height, res):
        """Ktree(msd, ss, UPG_METHOD, lead) with lead[k] as phyl_pwt leaves it, then calcpw"""
        num = len(groups)
        lead = (C.c_char * (KNODE * (2 * num - 1)))()
        base = C.addressof(lead)
        for k in range(num):
            C.cast(base + KNODE * k + 24, C.POINTER(C.c_int))[0] = k
            C.cast(base + KNODE * k + 28, C.POINTER(C.c_int))[0] = ndesc[k]
            C.cast(base + KNODE * k + 32, C.POINTER(C.c_double))[0] = height[k]
            C.cast(base + KNODE * k + 64, C.POINTER(C.c_double))[0] = res[k]
        lists = [self.ilist(g) for g in groups]
        grp = (C.c_void_p * (num + 1))(*([C.addressof(l) for l in lists] + [None]))
        ss = (C.c_char * 32)()
        C.cast(C.addressof(ss), C.POINTER(C.c_void_p))[0] = C.addressof(grp)
        C.cast(C.addressof(ss) + 16, C.POINTER(C.c_int))[0] = num
        C.cast(C.addressof(ss) + 20, C.POINTER(C.c_int))[0] = sum(len(g) for g in groups)
        self.keep += [lead, lists, grp, ss]
        kt = self.new_tree(sd, C.addressof(ss), UPG_METHOD, base)
        self.calcpw(kt, None)
        return self.read_nodes(kt, num)

    def phyl_pwt(self, sd, many, groups, flat):
        """prrn5.cc:343-391 composed from the reference's parts: (tree, root, weight, sumwt, leaves, weights inside the groups)"""
        weight = [0.] * many
        ndesc, height, res = [len(g) for g in groups], [0.] * len(groups), [0.] * len(groups)
        for k, gr in enumerate(groups):
            if len(gr) > 1:
                swt, h, r = self.subtree(sd, gr)
                for m, w in zip(gr, swt):
                    weight[int(m)] = w
                if not flat:
                    height[k], res[k] = h, r
            else:
                weight[int(gr[0])] = 1.
        inner = list(weight)
        t, root = self.group_tree(sd, groups, ndesc, height, res)
        for k, gr in enumerate(groups):
            for m in gr:
                weight[int(m)] *= float(t["vol"][k])
        sumwt = 0.
        for w in weight:
            sumwt += w
        return t, root, np.array(weight), sumwt, (ndesc, height, res), np.array(inner)


def b64(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def same_tree(a, b):
    return all(np.array_equal(np.asarray(a[k], np.int32), np.asarray(b[k], np.int32)) for k in ("left", "right", "parent", "ndesc")) and \
        all(np.array_equal(b64(a[k]), b64(b[k])) for k in ("height", "length", "res", "vol", "cur"))


def run(name, molc, rows, groups, want=(), save=True):
    import ktreegrouplib as kg
    import ktreelib
    from prrn_aln_amd import operator as op
    ref = Ref(molc)
    codes = op.encode(rows, molc)
    ln, many = codes.shape
    assert many <= 16 and ln <= 400
    groups = [np.asarray(g, np.int32) for g in groups]
    assert sorted(np.concatenate(groups).tolist()) == list(range(many))
    sd = ref.R.group(["m%d" % i for i in range(many)], rows)
    gdist = ref.group_dist(sd, groups)
    lit_d, lit_c = kg.group_divergence(codes, groups, kg.group_counts_literal)
    vec_d, vec_c = kg.group_divergence(codes, groups)
    assert np.array_equal(lit_c, vec_c), "%s: the closed form differs from the literal loop" % name
    assert np.array_equal(b64(lit_d), b64(gdist)), "%s: the restatement's group distances differ from the reference's" % name
    out = dict(molc=np.array([molc], np.int32), codes=codes, gstart=np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32),
               gmember=np.concatenate(groups).astype(np.int32), gdist=gdist, gcounts=lit_c)
    seen = set()
    for flat in (0, 1):
        t, root, weight, sumwt, leaves, inner = ref.phyl_pwt(sd, many, groups, flat)
        mt, mw, ms, _, _ = kg.phyl_pwt(codes, groups, bool(flat))
        assert mt["root"] == root and same_tree(mt, t), "%s (flat %d): the restatement's tree differs from the reference's" % (name, flat)
        assert np.array_equal(b64(mw), b64(weight)) and b64([ms])[0] == b64([sumwt])[0], "%s (flat %d): the restatement's weights differ" % (name, flat)
        pfx = "flat_" if flat else "tree_"
        for k, a in t.items():
            out[pfx + k] = a
        out[pfx + "weight"], out[pfx + "sumwt"] = weight, np.array([sumwt])
        out[pfx + "leaf_ndesc"], out[pfx + "leaf_height"], out[pfx + "leaf_res"] = np.array(leaves[0], np.int32), np.array(leaves[1]), np.array(leaves[2])
        out["inner_weight"] = inner
        num = len(groups)
        if not flat:
            par = t["parent"][:num]
            if (np.array(leaves[1]) > t["height"][par]).any() and (t["length"][:num] == 0).any():
                seen.add("clamped")
            if (t["res"][num:] == EPS).any():
                seen.add("res_eps")
            if (gdist == 0).any():
                seen.add("zero_dist")
            if any((np.diff(g) < 0).any() for g in groups):
                seen.add("unsorted")
    if all(len(g) == 1 for g in groups):                               # must be Ktree(msd) + calcpw on the members in the groups' order
        order = [int(g[0]) for g in groups]
        sd2 = ref.R.group(["m%d" % i for i in range(many)], [rows[m] for m in order])
        kt = ref.new_tree(sd2)
        ref.calcpw(kt, None)
        t2, r2 = ref.read_nodes(kt, many)
        assert same_tree({k[5:]: v for k, v in out.items() if k.startswith("tree_")}, t2), "%s: singletons differ from Ktree(msd)" % name
        seen.add("singletons")
    print("%-24s %2d x %3d in %s: %s; sumwt %.6f" % (name, many, ln, [len(g) for g in groups], sorted(seen), float(out["tree_sumwt"][0])))
    for w in want:
        assert w in seen, "%s does not show %s" % (name, w)
    if save:
        os.makedirs(GOLD, exist_ok=True)
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), **out)


def family(n, length, seed, dna=False, **kw):
    from prrn_aln_amd.synth import make_family, DNA
    return list(make_family(n, length, seed, **({"alphabet": DNA} if dna else {}), **kw).msa)


def mutated(row, frac, seed, alphabet=_AA):
    rng = np.random.default_rng(seed)
    r = list(row)
    for c in range(len(r)):
        if r[c] != "-" and rng.random() < frac:
            r[c] = alphabet[int(rng.integers(len(alphabet)))]
    return "".join(r)


def tall_leaf():
    """group 0 holds two members far from each other, group 1 a copy of each, and the two differ by substitutions only: the between-group divergence is half the
    divergence inside group 0, so leaf 0 is taller than its merge with leaf 1 and rl = res + height - leaf height is 0"""
    f = family(6, 120, 71, indel=0.04, max_indel=5)
    far = mutated(f[1], 0.8, 5)
    return [f[0], far, f[0], far, f[2], f[3], f[4], f[5]], [[0, 1], [2, 3], [4, 5], [6], [7]]


def timed(large=False):
    ref = Ref(1)
    dec = np.array(list("?-X" + _AA + "BZ"))
    if large:
        import ktree_probe
        name, codes, sizes = "synthetic 4096 x 5000 star", ktree_probe.synthetic(4096, 5000, 4096), (("64_groups_of_64", 64), ("2048_pairs", 2))
    else:
        name, codes, sizes = "prog256x1024 start MSA", np.load(os.path.join(ROOT, "tests", "golden", "msa", "prog256x1024.npz"))["codes"], (("16_groups_of_16", 16), ("128_pairs", 2))
    rows = ["".join(dec[codes[:, m]]) for m in range(codes.shape[1])]
    sd = ref.R.group(["m%d" % i for i in range(len(rows))], rows)
    out = {}
    for label, size in sizes:
        groups = [list(range(s, s + size)) for s in range(0, codes.shape[1], size)]
        t0 = time.perf_counter()
        ref.group_dist(sd, groups)
        out[label] = {"input": name, "members": codes.shape[1], "columns": codes.shape[0], "groups": len(groups), "ms": round((time.perf_counter() - t0) * 1e3, 1)}
        print(json.dumps({"reference_group_pairdvn_one_core": {label: out[label]}}), flush=True)


F12 = lambda: family(12, 150, 61, indel=0.05, max_indel=6)
JOBS = {
    "prot8": lambda: run("prot8_3groups", 1, family(8, 120, 60, indel=0.05, max_indel=6), [[0, 1, 2], [3, 4], [5, 6, 7]]),
    "prot12": lambda: run("prot12_5142", 1, F12(), [[0, 1, 2, 3, 4], [5], [6, 7, 8, 9], [10, 11]]),
    "dna10": lambda: run("dna10_4groups", 2, family(10, 90, 62, dna=True, indel=0.04, max_indel=8), [[0, 1, 2], [3, 4, 5, 6], [7], [8, 9]]),
    "unsorted": lambda: run("prot12_unsorted", 1, F12(), [[7, 2, 9], [11], [4, 0, 10, 1], [8, 3], [6, 5]], want=("unsorted",)),
    "tall": lambda: run("prot8_tall_leaf", 1, *tall_leaf(), want=("clamped", "res_eps")),
    "twins": lambda: (lambda f: run("prot8_identical", 1, [f[0], f[0], f[0], f[0], f[1], f[1], f[2], f[3]], [[0, 1], [2, 3], [4, 5], [6, 7]], want=("zero_dist",)))(family(4, 100, 63, indel=0.05, max_indel=5)),
    "two": lambda: run("prot9_two_groups", 1, family(9, 140, 64, indel=0.05, max_indel=6), [[0, 1, 2, 3, 4], [5, 6, 7, 8]]),
    "singletons": lambda: run("prot7_singletons", 1, family(7, 110, 65, indel=0.05, max_indel=6), [[3], [0], [6], [1], [2], [5], [4]], want=("singletons",)),
    "wide": lambda: run("prot16x400", 1, family(16, 110, 66, indel=0.04, max_indel=6), [[0, 5, 3], [1, 2, 4, 6, 7, 8, 9], [10], [15, 14, 13, 12, 11]]),
}

if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--time":
        timed(large=len(sys.argv) > 2 and sys.argv[2] == "large")
    elif len(sys.argv) > 1:
        JOBS[sys.argv[1]]()
    else:
        for j in JOBS:                                                 # (one process per case: the reference keeps its parameters in globals)
            subprocess.check_call([sys.executable, os.path.abspath(__file__), j])
