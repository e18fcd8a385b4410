#!/usr/bin/env python3
"""Generate tests/golden/progressive/*.npz from the REAL reference (oracle/_ref): progressive alignments of small families over
given guide trees, merge by merge.  The tool walks the tree post-order in Python and does at every inner node what
ProgMsa::prog_up does there (reference src/prrn5.h:94-100): Seq::exg_seq(0, 0) on both sons' results and the reference's own
mSeq* align2(mSeq*, mSeq*, mSeq*, ALPRM*) (src/maln2.cc:2063; msd = 0, alp = the library's alprm), called in
oracle/_ref/libprrn_ref.so through ctypes by their mangled names.  Every leaf is a file read by the shim's ref_group_read.

Per inner node it records what ref_align_dump of the same pair gives -- DP score, swp, alnmode, the members of the PwdM's two
sides, the skeleton of align2 -- and the merged block: its codes (read from the dump of the merge one level up, where the block is
a side; the root's from a dump against a leaf), its length, and the member order, found by matching de-gapped rows (the members of
a case are pairwise distinct: asserted).  With them the sequences, the parameters as the reference's PwdM reports them, the
similarity matrix and the tree.  Data only.

Before a case is saved: every merged block must be its two sons' blocks interleaved by the recorded skeleton, the PwdM's a side
first (tests/proglib.py's restatement), and hold gap code 1 wherever it holds no residue.  Over the whole set (checked after the
last case): each of NGP_ALB, NTV_ALB, HLF_ALB, RHF_ALB and GPF_ALB occurs; swp = 1 occurs in RHF and GPF; swp = 0 in NTV and GPF;
some merge has 8 or more members on each side.  swp = 1 in NTV cannot occur here: PwdM::selAlnMode swaps the shorter side away in
NTV_ALN only (src/maln2.cc:109-111), and with algmode.bnd = 1 -- the only setting g2g_progressive takes -- the mode is NTV_ALB,
which never swaps; the tool asserts that too.

The reference keeps its parameters in process globals: one process per case.
Usage: python tools/make_progressive_golden.py [case]      (needs oracle/_ref, i.e. the reference's sources at build time)
       python tools/make_progressive_golden.py --time-bench [probe.json]
           the reference's own merges of the bench family (synth.make_family(256, 1024, 1)) over the guide tree that
           tools/progressive_probe.py wrote into profiles/progressive_probe.json, wall clock on one core; the figures are written
           into the same file under "reference_one_core"."""
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
GOLD = os.path.join(ROOT, "tests", "golden", "progressive")
ALIGN2 = "_Z6align2P4mSeqS0_S0_P5ALPRM"
EXG_SEQ = "_ZN3Seq7exg_seqEii"
_AA = "ARNDCQEGHILKMFPSTWYV"


class Ref:
    def __init__(self, molc, ls=0, uv=None):
        import refdump
        self.R = refdump.RefLib(molc=molc, ls=ls, band=True)
        L = self.L = self.R.lib
        if uv is not None:
            L.ref_set_uv.argtypes = [C.c_double, C.c_double]
            L.ref_set_uv(*uv)
        self.align2 = getattr(L, ALIGN2)
        self.align2.restype = C.c_void_p
        self.align2.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.exg_seq = getattr(L, EXG_SEQ)
        self.exg_seq.restype = None
        self.exg_seq.argtypes = [C.c_void_p, C.c_int, C.c_int]
        self.alprm = C.addressof(C.c_char.in_dll(L, "alprm"))

    def leaf(self, name, row):
        return self.R.group([name], [row])

    def merge(self, l, r):
        """prog_up's body at an inner node"""
        self.exg_seq(l, 0, 0)
        self.exg_seq(r, 0, 0)
        msd = self.align2(l, r, None, self.alprm)
        assert msd
        return msd


# ---- trees: leaves 0 .. n - 1, inner nodes n .. 2 n - 2, the root last ---------------------------------------------------------------
def tree_arrays(sons, n):
    left = np.full(2 * n - 1, -1, np.int32); right = left.copy(); parent = left.copy()
    for k, (l, r) in enumerate(sons, n):
        left[k], right[k] = l, r
        parent[l] = parent[r] = k
    return left, right, parent


def caterpillar(n, leaf_side):
    """leaf_side(j) -> True: the new leaf of inner node n + j is its LEFT son"""
    sons = [(0, 1)]
    for j in range(1, n - 1):
        sons.append((j + 1, n + j - 1) if leaf_side(j) else (n + j - 1, j + 1))
    return tree_arrays(sons, n)


def balanced(n):
    level, sons, nxt = list(range(n)), [], n
    while len(level) > 1:
        up = []
        for i in range(0, len(level), 2):
            sons.append((level[i], level[i + 1]))
            up.append(nxt); nxt += 1
        level = up
    return tree_arrays(sons, n)


def tree_from_kmers(codes, molc, k):
    import kmerlib
    import ktreelib
    t = ktreelib.tree_from_dist(kmerlib.distance(codes, molc, k)[0], with_weights=False)
    return tuple(np.asarray(t[f], np.int32) for f in ("left", "right", "parent"))


# ---- families ----------------------------------------------------------------------------------------------------------------------
def family(n, length, seed, dna=False, **kw):
    from prrn_aln_amd.synth import make_family, DNA
    return list(make_family(n, length, seed, **({"alphabet": DNA} if dna else {}), **kw).seqs)


def ungapped(n, length, seed, sub=0.25):
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 20, length)
    rows = []
    for m in range(n):
        s = anc.copy()
        hit = rng.random(length) < sub * (0.3 + 1.4 * m / n)
        s[hit] = rng.integers(0, 20, int(hit.sum()))
        rows.append("".join(_AA[x] for x in s))
    return rows


def walk(ref, rows, tree, timed=False):
    """the reference's merges over the tree, sons before fathers.  Returns ({node: record}, {node: codes of its block}, the inner
    nodes with the root first); with timed only the clock runs: (milliseconds in prog_up's body, merges, columns of the root's block)"""
    left, right, parent = tree
    n = len(rows)
    root = int(np.flatnonzero(parent < 0)[0])
    hs = {i: ref.leaf("s%03d" % i, rows[i]) for i in range(n)}
    rec, codes = {}, {}
    # (post-order without recursion: a caterpillar of hundreds of leaves is as deep as it is long)
    order, stack = [], [root]
    while stack:
        k = stack.pop()
        if left[k] >= 0:
            order.append(k)
            stack += [int(left[k]), int(right[k])]
    t_ms = 0.
    for k in reversed(order):
        l, r = hs[int(left[k])], hs[int(right[k])]
        t0 = time.perf_counter()
        hs[k] = ref.merge(l, r)
        t_ms += (time.perf_counter() - t0) * 1e3
        if timed:
            ref.R.free(l); ref.R.free(r)
            continue
        d = ref.R.align_dump(l, r)
        swp = int(d["swp"][0])
        rec[k] = dict(swp=swp, mode=int(d["alnmode"][0]), scr=float(d["align2_scr"][0]), skl=d["align2_skl"].reshape(-1, 2).astype(np.int32),
                      na=int(d["a_many"][0]), nb=int(d["b_many"][0]), dump=d)
        sa, sb = (int(right[k]), int(left[k])) if swp else (int(left[k]), int(right[k]))
        codes[sa] = d["a_seq"].reshape(-1, rec[k]["na"])[1:-1].copy()
        codes[sb] = d["b_seq"].reshape(-1, rec[k]["nb"])[1:-1].copy()
    if timed:
        return t_ms, len(order), ref.L.ref_group_len(hs[root])
    # the root's block: a side of a dump against a fresh copy of leaf 0
    d = ref.R.align_dump(hs[root], ref.leaf("again", rows[0]))
    side = "a_" if int(d["a_many"][0]) == n else "b_"
    assert int(d[side + "many"][0]) == n and n > 1
    codes[root] = d[side + "seq"].reshape(-1, n)[1:-1].copy()
    return rec, codes, order


def run(name, molc, rows, tree, ls=0, uv=None, save=True):
    import proglib as pl
    from prrn_aln_amd import operator as op
    left, right, parent = tree
    n = len(rows)
    assert len(set(rows)) == n, "%s: the members must be pairwise distinct" % name
    ref = Ref(molc, ls, uv)
    enc = [op.encode([r], molc).reshape(-1) for r in rows]
    rec, codes, order = walk(ref, rows, tree)
    leaf_of = {e.tobytes(): i for i, e in enumerate(enc)}
    for i in range(n):
        assert np.array_equal(codes[i].reshape(-1), enc[i]), "%s: leaf %d is not read as it was written" % (name, i)
    members = {i: np.array([i], np.int32) for i in range(n)}
    for k in reversed(order):
        r = rec[k]
        blk = codes[k]
        assert blk.min() >= 1, "%s: node %d holds a nil code" % (name, k)
        r["order"] = np.array([leaf_of[pl.degap(blk[:, m]).tobytes()] for m in range(blk.shape[1])], np.int32)
        l, rr = int(left[k]), int(right[k])
        mine, mo = pl.merge((codes[l], members[l]), (codes[rr], members[rr]), r["swp"], r["skl"])
        assert np.array_equal(mo, r["order"]), "%s: node %d: members %s, the swapped order gives %s" % (name, k, r["order"], mo)
        assert np.array_equal(mine, blk), "%s: node %d is not its sons interleaved by the recorded skeleton" % (name, k)
        members[k] = r["order"]
        r["codes"], r["len"] = blk, len(blk)
    d0 = rec[order[-1]]["dump"]
    nodes = sorted(rec)
    cat = lambda xs, dt: np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs])
    offs = lambda xs: np.concatenate([[0], np.cumsum([np.asarray(x).size for x in xs])]).astype(np.int64)
    if save:
        os.makedirs(GOLD, exist_ok=True)
        sc = lambda key, dt: np.array([d0[key].reshape(-1)[0]], dt)
        np.savez_compressed(
            os.path.join(GOLD, name + ".npz"), molc=np.array([molc], np.int32), codes=cat(enc, np.uint8), lens=np.array([len(e) for e in enc], np.int32),
            tree_left=left, tree_right=right, tree_parent=parent,
            u=sc("alnprm_u", np.float64), v=sc("alnprm_v", np.float64), u1=sc("alnprm_u1", np.float64), tgapf=sc("alnprm_tgapf", np.float64),
            scale=sc("alnprm_scale", np.float64), k1=sc("alnprm_k1", np.int32), ls=sc("alnprm_ls", np.int32), sh=sc("alnprm_sh", np.int32),
            simmtx=d0["simmtx"].astype(np.float64),
            node=np.array(nodes, np.int32), node_len=np.array([rec[k]["len"] for k in nodes], np.int32),
            node_scr=np.array([rec[k]["scr"] for k in nodes], np.float64), node_swp=np.array([rec[k]["swp"] for k in nodes], np.int32),
            node_mode=np.array([rec[k]["mode"] for k in nodes], np.int32), node_na=np.array([rec[k]["na"] for k in nodes], np.int32),
            node_nb=np.array([rec[k]["nb"] for k in nodes], np.int32),
            node_order=cat([rec[k]["order"] for k in nodes], np.int32), node_order_off=offs([rec[k]["order"] for k in nodes]),
            node_codes=cat([rec[k]["codes"] for k in nodes], np.uint8), node_codes_off=offs([rec[k]["codes"] for k in nodes]),
            node_skl=cat([rec[k]["skl"] for k in nodes], np.int32), node_skl_off=offs([rec[k]["skl"] for k in nodes]))
    modes = {}
    for k in nodes:
        key = "%s/swp%d" % (pl.MODE_NAME.get(rec[k]["mode"], str(rec[k]["mode"])), rec[k]["swp"])
        modes[key] = modes.get(key, 0) + 1
    print("%-18s %2d members, lengths %d .. %d -> %d columns; %s; widest merge %s" % (
        name, n, min(map(len, rows)), max(map(len, rows)), rec[order[0]]["len"], modes,
        max(((rec[k]["na"], rec[k]["nb"]) for k in nodes), key=lambda t: min(t))))


def check_set():
    import proglib as pl
    seen, wide = set(), False
    for name in pl.names():
        g = pl.load(name)
        for m, s, a, b in zip(g["node_mode"].tolist(), g["node_swp"].tolist(), g["node_na"].tolist(), g["node_nb"].tolist()):
            seen.add((pl.MODE_NAME[m], s))
            wide = wide or min(a, b) >= 8
    for m in pl.MODE_NAME.values():
        assert any(x[0] == m for x in seen), "no merge in mode %s" % m
    for want in (("RHF_ALB", 1), ("GPF_ALB", 1), ("NTV_ALB", 0), ("GPF_ALB", 0)):
        assert want in seen, "no merge with mode %s and swp %d" % want
    # selAlnMode swaps by length in NTV_ALN alone (src/maln2.cc:109-111); the banded NTV_ALB falls to `default: swp = a->inex.intr`
    assert ("NTV_ALB", 1) not in seen, "a banded NTV merge swapped: the reference does not do that"
    assert wide, "no merge with 8 or more members on each side"
    print("the set covers", sorted(seen))


def time_bench(path):
    """the reference's own time for the merges of the bench family over the probe's tree, one core"""
    from prrn_aln_amd.synth import make_family
    out = json.load(open(path))
    t = out["tree"]
    tree = tuple(np.asarray(t[k], np.int32) for k in ("left", "right", "parent"))
    rows = list(make_family(out["members"], out["length"], 1).seqs)
    ms, merges, columns = walk(Ref(1), rows, tree, timed=True)
    out["reference_one_core"] = {"what": "exg_seq + align2(mSeq*, mSeq*, 0, &alprm) of every inner node of the same tree, sons before fathers, one core of the build machine",
                                 "merges": merges, "total_ms": round(ms, 1), "columns": columns, "same_columns_as_the_library": columns == out["columns"]}
    json.dump(out, open(path, "w"), indent=1)
    print(json.dumps(out["reference_one_core"]))


def _dna12(seed):
    return family(12, 120, seed, dna=True, indel=0.03, sub=0.12)


def _with_tree(rows, molc, k):
    from prrn_aln_amd import operator as op
    return rows, tree_from_kmers([op.encode([r], molc).reshape(-1) for r in rows], molc, k)


JOBS = {
    "prot2": lambda: run("prot2_unequal", 1, family(2, 100, 11, indel=0.06, sub=0.2), balanced(2)),
    "prot3_l": lambda: run("prot3_leaf_left", 1, family(3, 90, 12, indel=0.04, sub=0.2), caterpillar(3, lambda j: True)),
    "prot3_r": lambda: run("prot3_leaf_right", 1, family(3, 90, 13, indel=0.04, sub=0.2), caterpillar(3, lambda j: False)),
    "prot8": lambda: run("prot8_gapfree", 1, ungapped(8, 120, 14), balanced(8)),
    "prot16": lambda: run("prot16_indels", 1, *_with_tree(family(16, 130, 33, indel=0.03, sub=0.15), 1, 3)),
    "prot24": lambda: run("prot24_caterpillar", 1, family(24, 100, 16, indel=0.02, sub=0.12), caterpillar(24, lambda j: j % 2 == 1)),
    "dna12": lambda: run("dna12", 2, *_with_tree(_dna12(17), 2, 6)),
    "dna12_ls3": lambda: run("dna12_ls3", 2, *_with_tree(_dna12(18), 2, 6), ls=3),
    "prot12_uv": lambda: run("prot12_u2.1_v9.3", 1, *_with_tree(family(12, 110, 19, indel=0.03, sub=0.15), 1, 3), uv=(2.1, 9.3)),
}

if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--time-bench":
        time_bench(sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "progressive_probe.json"))
    elif len(sys.argv) > 1 and sys.argv[1] == "--check-set":
        check_set()
    elif len(sys.argv) > 1:
        JOBS[sys.argv[1]]()
    else:
        for j in JOBS:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), j])
        check_set()
