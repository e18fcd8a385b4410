"""Test-side restatement of the reference's weighting tree (Ssrel::calcweight: Ktree(msd) + calcpw, reference src/prrn5.cc:385-386)
in plain Python / numpy, and loaders for every (MSA, tree) pair the fixtures hold.  Checker only -- the product's versions are
csrc/g2g_ktree.hip (divergence kernel on the GPU, tree and weights in C++).

  pairdvn / divergence   calcdistseq / pairdvn           src/phyl.cc:344-385, src/divseq.cc:33-63
  upg_tree               DistTree::upg_method + dminidx / dminrow, Knode::teachparent   src/phyl.cc:911-1026, 583-595
  calcpw                 Ktree::calcpw -> pairwt         src/phyl.cc:704-767, 813-826

Python floats are IEEE doubles and every expression keeps the reference's operand order, so the results are meant to be
bit-equal to the reference's -- tests/test_ktree_host.py holds the restatement itself to that on the 26 trees the fixtures
recorded."""
from __future__ import annotations

import functools
import gzip
import json
import math
import os
import sys

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FLT_MAX = 3.4028234663852886e+38
EPS = 1.e-7                      # fepsilon, src/cmn.h:54
GAPFRAC = 0.8                    # src/divseq.cc:29


def elem(i: int, j: int) -> int:
    """src/cmn.h:115-117"""
    return j * (j - 1) // 2 + i if i < j else i * (i - 1) // 2 + j


# ---- 1. divergence --------------------------------------------------------------------------------------------------------
def pairdvn_counts(ci, cj):
    """the walk of one pair, column by column: (mch, mmc, unp, gap).  A code <= 1 is a gap (IsGap)."""
    mch = mmc = unp = gap = gsi = gsj = 0
    for a, b in zip(ci.tolist(), cj.tolist()):
        if a <= 1:
            if b > 1:
                unp += 1
                if gsi <= gsj:
                    gap += 1
                gsj = 0
            gsi += 1                          # (also on a gap / gap column, where gsj stands still)
        else:
            if b <= 1:
                unp += 1
                if gsi >= gsj:
                    gap += 1
                gsj += 1
            else:
                if a == b:
                    mch += 1
                else:
                    mmc += 1
                gsj = 0
            gsi = 0
    return mch, mmc, unp, gap


def counts_to_dist(counts: np.ndarray) -> np.ndarray:
    """src/divseq.cc:61-62 on arrays of counts: elementwise IEEE double arithmetic in the reference's order"""
    c = np.asarray(counts, np.int64).reshape(-1, 4).astype(np.float64)
    mch, mmc, unp, gap = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    gapunp = GAPFRAC * gap + (1 - GAPFRAC) * unp
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1. - mch / ((gapunp + mch) + mmc)


def divergence_scalar(codes: np.ndarray):
    """(dist, counts) of an MSA ((len, many) codes) by the column-by-column walk -- small inputs"""
    many = codes.shape[1]
    counts = np.zeros((many * (many - 1) // 2, 4), np.int32)
    for j in range(1, many):
        for i in range(j):
            counts[elem(i, j)] = pairdvn_counts(codes[:, i], codes[:, j])
    return counts_to_dist(counts), counts


def _run_before(flag: np.ndarray, inc: np.ndarray) -> np.ndarray:
    """For every column: the sum of `inc` over the columns of the current run of `flag` that lie BEFORE this column (a run ends
    at a column where flag is false) -- the value a counter that adds inc inside a run and resets outside it holds on entry."""
    s = np.cumsum(inc, axis=-1, dtype=np.int32)
    base = np.maximum.accumulate(np.where(flag, 0, s), axis=-1)       # s at the last column outside a run (s never decreases)
    after = s - base
    before = np.zeros_like(after)
    before[..., 1:] = after[..., :-1]
    return before


def divergence(codes: np.ndarray):
    """The same, vectorised over the columns and over all partners i < j of a member j: gsi on entry to a column is the length of
    member i's gap run so far; gsj counts, within member j's gap run so far, the columns where i had a residue."""
    codes = np.ascontiguousarray(codes, np.uint8)
    many = codes.shape[1]
    rows = np.ascontiguousarray(codes.T)
    isgap = rows <= 1
    gsi_all = _run_before(isgap, isgap)
    counts = np.zeros((many * (many - 1) // 2, 4), np.int32)
    for j in range(1, many):
        a, ga, gsi = rows[:j], isgap[:j], gsi_all[:j]
        b, gb = rows[j][None, :], isgap[j][None, :]
        gsj = _run_before(np.broadcast_to(gb, ga.shape), gb & ~ga)
        both = ~ga & ~gb
        k0 = j * (j - 1) // 2
        counts[k0:k0 + j, 0] = (both & (a == b)).sum(1)
        counts[k0:k0 + j, 1] = (both & (a != b)).sum(1)
        counts[k0:k0 + j, 2] = (ga != gb).sum(1)
        counts[k0:k0 + j, 3] = ((ga & ~gb & (gsi <= gsj)) | (~ga & gb & (gsi >= gsj))).sum(1)
    return counts_to_dist(counts), counts


# ---- 2. the tree ----------------------------------------------------------------------------------------------------------
class Node:
    __slots__ = ("left", "right", "parent", "ndesc", "height", "length", "res", "vol", "cur", "ros")

    def __init__(self):
        self.left = self.right = self.parent = -1
        self.ndesc = 0
        self.height = self.length = self.res = self.vol = self.cur = self.ros = 0.


def upg_tree(many: int, dist_in):
    """DistTree::upg_method (UPG_METHOD) + teachparent: (nodes, root).  dist_in is not modified."""
    d = [float(x) for x in dist_in]
    lead = [Node() for _ in range(2 * many - 1)]
    row = list(range(many))
    nodes = list(range(many))
    nnbr = [0] * many
    nnbr[0] = 1
    k = 0
    for m in range(many):
        lead[m].ndesc = 1
        for n in range(m):
            if d[k] < d[elem(m, nnbr[m])]:
                nnbr[m] = n
            if d[k] < d[elem(n, nnbr[n])]:
                nnbr[n] = m
            k += 1
    m = many
    root = 0
    for n in range(many - 1, 0, -1):
        # dminidx over row[0 .. n): the first minimum wins
        ii = row[0]
        dmin = d[elem(ii, nnbr[ii])]
        for j in range(1, n):
            jj = row[j]
            dij = d[elem(jj, nnbr[jj])]
            if dij < dmin:
                ii, dmin = jj, dij
        jj = nnbr[ii]
        root = m
        m += 1
        rt, ln, rn = lead[root], lead[nodes[ii]], lead[nodes[jj]]
        rt.left, rt.right = nodes[ii], nodes[jj]
        rt.height = dmin / 2
        ln.length = rt.height - ln.height
        if ln.length < 0:
            ln.length = 0.
        rn.length = rt.height - rn.height
        if rn.length < 0:
            rn.length = 0.
        rl = ln.res + rt.height - ln.height
        rr = rn.res + rt.height - rn.height
        rt.res = (rl * rr) / (rl + rr) if (rl > EPS and rr > EPS) else EPS
        rt.ndesc = ln.ndesc + rn.ndesc
        jpos = 0
        nnbr[ii] = -1
        for k in range(n + 1):
            kk = row[k]
            if kk == ii:
                continue
            if kk == jj:
                jpos = k
                continue
            e = elem(kk, ii)
            x = d[e]
            x *= ln.ndesc                    # three separate roundings
            x += rn.ndesc * d[elem(kk, jj)]
            x /= rt.ndesc
            d[e] = x
            if nnbr[kk] == ii or nnbr[kk] == jj:
                nnbr[kk] = -1
        nodes[ii] = root
        row[jpos] = row[n]
        for k in range(n):
            kk = row[k]
            if nnbr[kk] < 0:               # dminrow: from FLT_MAX, strict <, the row itself when nothing is nearer
                best, arg = FLT_MAX, kk
                for q in range(n):
                    qq = row[q]
                    if qq == kk:
                        continue
                    dq = d[elem(kk, qq)]
                    if dq < best:
                        best, arg = dq, qq
                nnbr[kk] = arg

    def teachparent(i):                      # iterative post-order (the big tree is deeper than Python likes to recurse)
        low = {}
        stack = [(i, False)]
        while stack:
            v, done = stack.pop()
            nd = lead[v]
            if nd.left < 0:
                low[v] = v
                continue
            if not done:
                lead[nd.left].parent = lead[nd.right].parent = v
                stack.append((v, True))
                stack.append((nd.right, False))
                stack.append((nd.left, False))
                continue
            nd.ndesc = lead[nd.left].ndesc + lead[nd.right].ndesc
            l, r = low[nd.left], low[nd.right]
            if l > r:
                l = r
                nd.left, nd.right = nd.right, nd.left
            low[v] = l

    teachparent(root)
    lead[root].parent = -1
    return lead, root


def calcpw(lead, root: int) -> None:
    """Ktree::calcpw -> pairwt with wfact = 0, cfact = true: fills vol / cur (children are visited left first, which no value
    depends on: a node only reads its parent and writes itself and its children)."""
    lead[root].vol = 1.
    stack = [(root, FLT_MAX)]
    while stack:
        i, ros = stack.pop()
        node = lead[i]
        node.ros = ros
        if node.left < 0:
            node.vol = lead[node.parent].vol * node.cur
            continue
        left, right = lead[node.left], lead[node.right]
        a = left.res + left.length
        b = right.res + right.length
        if i == root:
            node.cur = left.cur = right.cur = 1.
        elif node.ros <= EPS or a + b <= EPS:
            a = b = 0.
            left.cur = right.cur = 0.5
            node.vol = node.cur * lead[node.parent].vol
        else:
            if a <= 0.:
                b += a
                a = EPS
            if b <= 0.:
                a += b
                b = EPS
            c = node.length + node.ros
            wab = a * b / (a + b)
            wbc = a * (b + c)
            wfa = 1. + a * node.ros / ((wab + c) * (a + c))
            wfb = 1. + b * node.ros / ((wab + c) * (b + c))
            wab = wbc + b * c
            wbc /= wab * wfb
            wac = b * (a + c) / (wab * wfa)
            wab = c * (a + b) / wab
            a *= node.ros / (a + node.ros)
            b *= node.ros / (b + node.ros)
            node.cur *= math.sqrt(wac * wbc / wab)
            node.vol = node.cur * lead[node.parent].vol
            left.cur = math.sqrt(wab * wac / wbc)
            right.cur = math.sqrt(wab * wbc / wac)
        stack.append((node.right, a))
        stack.append((node.left, b))


def tree_dict(lead, root: int) -> dict:
    keys = ("left", "right", "parent", "ndesc", "height", "length", "res", "vol", "cur")
    t = {k: [getattr(nd, k) for nd in lead] for k in keys}
    t["root"] = root
    return t


def tree_from_dist(dist, with_weights: bool = True) -> dict:
    n = len(dist)
    many = int(round((1 + math.sqrt(1 + 8 * n)) / 2))
    assert many * (many - 1) // 2 == n
    lead, root = upg_tree(many, dist)
    if with_weights:
        calcpw(lead, root)
    return tree_dict(lead, root)


def bits(x) -> np.ndarray:
    """doubles as their bit patterns: equality of these is bit equality (-0. != 0., NaN == the same NaN)"""
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


# ---- fixtures -------------------------------------------------------------------------------------------------------------
# A `-O4` read-out of these three pairsum fixtures reuses the Ssrel of the refinement loop: their case #1 records the tree of case
# #0's MSA (its `tree` equals case #0's `tree`) next to the rows of the REFINED MSA -- so that (rows, tree) is no pair.
NOT_A_PAIR = {("prot40x60_ls3", 1), ("prot66x40_ls3", 1), ("prot72x50", 1)}


@functools.lru_cache(maxsize=None)
def pairs():
    """[(id, codes (len, many) uint8, reference tree dict)]: the five refine fixtures and the cases of the pairsum fixtures"""
    import pairsumlib
    from prrn_aln_amd import operator as op
    out = []
    for n in sorted(os.listdir(GOLD)):
        if n.startswith("refine_") and (n.endswith(".json") or n.endswith(".json.gz")):
            p = os.path.join(GOLD, n)
            f = json.load(gzip.open(p, "rt") if n.endswith(".gz") else open(p))
            out.append((n.split(".json")[0], op.encode(f["rows"], f["molc"]), f["tree"]))
    pdir = os.path.join(GOLD, "pairsum")
    for n in sorted(os.listdir(pdir)):
        if not n.endswith(".json"):
            continue
        f = json.load(open(os.path.join(pdir, n)))
        for k, case in enumerate(f["cases"]):
            if (f["name"], k) in NOT_A_PAIR:
                continue
            out.append(("pairsum_%s#%d" % (f["name"], k), pairsumlib.case_codes(case), case["tree"]))
    return out


@functools.lru_cache(maxsize=None)
def restated(idx: int):
    """(dist, counts, tree dict) of pairs()[idx] by the restatement -- computed once per session"""
    _, codes, _ = pairs()[idx]
    dist, counts = divergence(codes)
    dist.setflags(write=False)
    counts.setflags(write=False)
    return dist, counts, tree_from_dist(dist)


def ktree_fixtures():
    """tests/golden/ktree/*.json (tools/make_ktree_golden.py): [(name, codes, reference tree dict)]"""
    from prrn_aln_amd import operator as op
    d = os.path.join(GOLD, "ktree")
    out = []
    for n in sorted(os.listdir(d)):
        if n.endswith(".json"):
            f = json.load(open(os.path.join(d, n)))
            out.append((f["name"], op.encode(f["rows"], f["molc"]), f["tree"]))
    return out


if __name__ == "__main__":
    import time
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for k, (name, codes, ref) in enumerate(pairs()):
        t0 = time.time()
        _, _, t = restated(k)
        ok = all(t[q] == ref[q] for q in ("left", "right", "parent")) and all(np.array_equal(bits(t[q]), bits(ref[q])) for q in ("vol", "cur"))
        print("%-36s %4d x %5d  %s  %.2f s" % (name, codes.shape[1], codes.shape[0], "bit-equal" if ok else "DIFFERS", time.time() - t0))
