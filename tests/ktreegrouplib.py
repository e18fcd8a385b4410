"""Test-side restatement of the weighting tree over groups the caller brings: IterMsa::phyl_pwt in the branch ss->num < ss->elms
(reference src/prrn5.cc:333-391), in plain Python / numpy on top of ktreelib.  Checker only -- the product's version is
csrc/g2g_ktree_groups.hip (include/g2g_groups.h).

  group_counts_literal   pairdvn(const Seq*, const int*, const int*)   src/divseq.cc:65-105, the triple loop as written
  group_counts           the same counts without the ni x nj loop (the form the device code uses)
  upg_tree_leaves        DistTree::upg_method from preset leaves (ndesc, height, res)   src/phyl.cc:943-1026
  kirchhof / calcwt      Knode::kirchhof, Ktree::calcwt                 src/phyl.cc:637-649, 692-702
  phyl_pwt               the few lines of IterMsa::phyl_pwt around them

tests/test_ktree_groups_host.py holds group_counts to group_counts_literal on seeded random cases."""
from __future__ import annotations

import numpy as np

import ktreelib
from ktreelib import EPS, FLT_MAX, Node, elem


# ---- 1. the group divergence ------------------------------------------------------------------------------------------------
def group_counts_literal(codes: np.ndarray, ga, gb):
    """(mch, mmc, unp, gap) of group A = ga against group B = gb (lists of members, in list order): divseq.cc:65-105 line by line"""
    ni, nj = len(ga), len(gb)
    gsi, gsj = [0] * ni, [0] * nj
    mch = mmc = unp = gap = 0
    for row in np.asarray(codes).tolist():
        for i in range(ni):
            a = row[ga[i]]
            for j in range(nj):
                b = row[gb[j]]
                if a <= 1:
                    if b > 1:
                        unp += 1
                        if gsi[i] <= gsj[j]:
                            gap += 1
                        gsj[j] = 0
                    gsi[i] += 1
                else:
                    if b <= 1:
                        unp += 1
                        if gsi[i] >= gsj[j]:
                            gap += 1
                        gsj[j] += 1
                    else:
                        if a == b:
                            mch += 1
                        else:
                            mmc += 1
                        gsj[j] = 0
                    gsi[i] = 0
    return mch, mmc, unp, gap


def _run_before(flag: np.ndarray, inc: np.ndarray) -> np.ndarray:
    """per column: the sum of inc over the columns of the current run of flag BEFORE this column (inc is 0 outside runs)"""
    s = np.cumsum(inc, axis=-1, dtype=np.int64)
    base = np.maximum.accumulate(np.where(flag, 0, s), axis=-1)
    after = s - base
    before = np.zeros_like(after)
    before[..., 1:] = after[..., :-1]
    return before


def group_counts(codes: np.ndarray, ga, gb):
    """The same four counts, vectorised over the columns.  Entering a column: g[i] = nj x (i's gap run ending just before it),
    h[j] = the residues A had over the columns of j's current gap run, R[i] = the residues of A among the members before i.
    Inside the column gsi[i] is g[i] + j while A[i] is a gap and (g[i] at j = 0, 0 behind) otherwise; gsj[j] is h[j] + R[i] while
    B[j] is a gap and (h[j] at i = 0, 0 behind) otherwise."""
    rows = np.ascontiguousarray(np.asarray(codes, np.uint8).T)
    A, B = rows[list(ga)], rows[list(gb)]
    a, b = A <= 1, B <= 1
    ni, nj = len(ga), len(gb)
    ra, rb = (~a).sum(0), (~b).sum(0)
    unp = int(((ni - ra) * rb + ra * (nj - rb)).sum())
    both = ~a[:, None, :] & ~b[None, :, :]
    same = both & (A[:, None, :] == B[None, :, :])
    mch = int(same.sum())
    mmc = int(both.sum()) - mch
    g = nj * _run_before(a, a.astype(np.int64))
    h = _run_before(b, np.where(b, ra[None, :], 0))
    R = np.cumsum(~a, axis=0) - (~a)
    jj = np.arange(nj)[:, None]
    gap = int((a[0][None, :] & ~b & (g[0][None, :] + jj <= h)).sum())                      # i = 0 against the residues of B
    gap += int((~b[0][None, :] & a[1:] & (g[1:] == 0)).sum())                               # j = 0, the gaps of A behind its first member
    gap += int((b[0][None, :] & ~a & (g >= h[0][None, :] + R)).sum())                       # j = 0 against the residues of A
    gap += int(((ra > 0)[None, :] & b[1:] & (h[1:] == 0)).sum())                            # A's first residue, the gaps of B behind its first member
    return mch, mmc, unp, gap


def group_divergence(codes: np.ndarray, groups, counter=group_counts):
    """(dist, counts) over all group pairs k < l at l (l - 1) / 2 + k: calcdistseq(sd, ss)"""
    num = len(groups)
    counts = np.zeros((num * (num - 1) // 2, 4), np.int32)
    for l in range(1, num):
        for k in range(l):
            counts[elem(k, l)] = counter(codes, groups[k], groups[l])
    return ktreelib.counts_to_dist(counts), counts


# ---- 2. the tree from preset leaves -------------------------------------------------------------------------------------------
def upg_tree_leaves(num: int, dist_in, ndesc=None, height=None, res=None):
    """ktreelib.upg_tree with leaves that start as phyl_pwt leaves them in lead[k]: (nodes, root)"""
    d = [float(x) for x in dist_in]
    lead = [Node() for _ in range(2 * num - 1)]
    row = list(range(num))
    nodes = list(range(num))
    nnbr = [0] * num
    nnbr[0] = 1
    k = 0
    for m in range(num):
        lead[m].ndesc = max(int(ndesc[m]), 1) if ndesc is not None else 1          # phyl.cc:956
        if height is not None:
            lead[m].height = float(height[m])
        if res is not None:
            lead[m].res = float(res[m])
        for n in range(m):
            if d[k] < d[elem(m, nnbr[m])]:
                nnbr[m] = n
            if d[k] < d[elem(n, nnbr[n])]:
                nnbr[n] = m
            k += 1
    m = num
    root = 0
    for n in range(num - 1, 0, -1):
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
        rl = ln.res + rt.height - ln.height                                          # (not clamped)
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
            x *= ln.ndesc
            x += rn.ndesc * d[elem(kk, jj)]
            x /= rt.ndesc
            d[e] = x
            if nnbr[kk] == ii or nnbr[kk] == jj:
                nnbr[kk] = -1
        nodes[ii] = root
        row[jpos] = row[n]
        for k in range(n):
            kk = row[k]
            if nnbr[kk] < 0:
                best, arg = FLT_MAX, kk
                for q in range(n):
                    qq = row[q]
                    if qq == kk:
                        continue
                    dq = d[elem(kk, qq)]
                    if dq < best:
                        best, arg = dq, qq
                nnbr[kk] = arg

    low = {}
    stack = [(root, False)]                                                          # Knode::teachparent
    while stack:
        v, done = stack.pop()
        nd = lead[v]
        if nd.left < 0:
            low[v] = v
            continue
        if not done:
            lead[nd.left].parent = lead[nd.right].parent = v
            stack += [(v, True), (nd.right, False), (nd.left, False)]
            continue
        nd.ndesc = lead[nd.left].ndesc + lead[nd.right].ndesc
        l, r = low[nd.left], low[nd.right]
        if l > r:
            l = r
            nd.left, nd.right = nd.right, nd.left
        low[v] = l
    lead[root].parent = -1
    return lead, root


def tree_from_dist_leaves(dist, ndesc=None, height=None, res=None, with_weights: bool = True) -> dict:
    n = len(dist)
    num = int(round((1 + (1 + 8 * n) ** 0.5) / 2))
    assert num * (num - 1) // 2 == n
    lead, root = upg_tree_leaves(num, dist, ndesc, height, res)
    if with_weights:
        ktreelib.calcpw(lead, root)
    return ktreelib.tree_dict(lead, root)


# ---- 3. weights inside a group --------------------------------------------------------------------------------------------------
def kirchhof(lead, root: int) -> None:
    """Knode::kirchhof from the root, phyl.cc:637-649 (a father is visited before its sons)"""
    stack = [root]
    while stack:
        i = stack.pop()
        nd = lead[i]
        if i == root:
            nd.vol = nd.res
            nd.cur = 1.
        else:
            par = lead[nd.parent]
            pres = nd.res + nd.length
            nd.cur = par.vol / pres if pres > 0. else par.cur / 2.
            nd.vol = par.vol - nd.length * nd.cur
        if nd.left >= 0:
            stack += [nd.right, nd.left]


def calcwt(lead, root: int, members: int):
    """Ktree::calcwt, phyl.cc:692-702, bwt = F_UNIF_WEIGHT = 0"""
    bwt = 0.
    kirchhof(lead, root)
    nf = 1. / (1. + bwt)
    return [(lead[root].ndesc * lead[i].cur + lead[i].ndesc * bwt) * nf for i in range(members)]


# ---- 4. phyl_pwt ------------------------------------------------------------------------------------------------------------
def phyl_pwt(codes: np.ndarray, groups, flat_leaves: bool = False, counter=group_counts):
    """prrn5.cc:343-391 with seqs given and no weights of their own: (tree dict over the groups, weight[many], sumwt, group dist,
    group counts).  A group's own tree is Ktree(extseq(group)): pairdvn over the extracted members in list order."""
    codes = np.asarray(codes, np.uint8)
    many, num = codes.shape[1], len(groups)
    weight = [0.] * many
    ndesc, height, res = [0] * num, [0.] * num, [0.] * num
    for k, gr in enumerate(groups):
        gr = [int(m) for m in gr]
        ndesc[k] = len(gr)
        if len(gr) > 1:
            sub_dist, _ = ktreelib.divergence(codes[:, gr])
            lead, root = ktreelib.upg_tree(len(gr), sub_dist)
            for m, w in zip(gr, calcwt(lead, root, len(gr))):
                weight[m] = w
            if not flat_leaves:
                height[k], res[k] = lead[root].height, lead[root].res
        else:
            weight[gr[0]] = 1.
    dist, counts = group_divergence(codes, groups, counter)
    tree = tree_from_dist_leaves(dist, ndesc, height, res)
    for k, gr in enumerate(groups):
        for m in gr:
            weight[int(m)] *= tree["vol"][k]
    sumwt = 0.
    for w in weight:
        sumwt += w
    return tree, np.array(weight, np.float64), sumwt, dist, counts


# ---- inputs ---------------------------------------------------------------------------------------------------------------------
def random_msa(rng, many: int, ln: int, nres: int = 4, pgap: float = 0.35, prun: float = 0.7, pnil: float = 0.) -> np.ndarray:
    """(len, many) codes with run-structured gaps: a member stays in / out of a gap with probability prun; nil codes with pnil"""
    out = np.zeros((ln, many), np.uint8)
    for m in range(many):
        gapped = rng.random() < pgap
        for c in range(ln):
            if rng.random() > prun:
                gapped = rng.random() < pgap
            out[c, m] = (0 if rng.random() < pnil else 1) if gapped else 2 + rng.integers(nres)
    return out


def random_groups(rng, many: int, num: int):
    """num non-empty groups over a random permutation of the members: uneven, unsorted lists"""
    perm = rng.permutation(many)
    cuts = np.sort(rng.choice(np.arange(1, many), num - 1, replace=False)) if num > 1 else np.zeros(0, int)
    return [g.astype(np.int32) for g in np.split(perm, cuts)]


def fixtures():
    """tests/golden/ktree_groups/*.npz (tools/make_ktree_groups_golden.py): one dict per case, arrays as saved plus name / groups"""
    import os
    d = os.path.join(ktreelib.GOLD, "ktree_groups")
    out = []
    for n in sorted(os.listdir(d)) if os.path.isdir(d) else []:
        if n.endswith(".npz"):
            f = dict(np.load(os.path.join(d, n)))
            f["name"] = n[:-4]
            f["groups"] = [f["gmember"][f["gstart"][g]:f["gstart"][g + 1]].copy() for g in range(len(f["gstart"]) - 1)]
            out.append(f)
    return out


# ---- refinement between given groups (tests/test_refine_groups_host.py, tests/test_gpu_refine_groups.py) ---------------------------------
def tree5(tree: dict):
    return tuple(np.asarray(tree[k], np.int32 if k in ("left", "right", "parent") else np.float64) for k in ("left", "right", "parent", "vol", "cur"))


def plan_groups(codes, groups, tree: dict, alp, thr, weight):
    """fuselib.plan started from the given relation instead of singletons: the dict refineplanlib.plan_object takes"""
    import fuselib as fl
    ln = codes.shape[0]
    rel0 = ([[int(m) for m in g] for g in groups],) + tree5(tree)
    whole = fl.consregss(codes, rel0, alp, weight)
    srl = whole[1]
    out = dict(nothing=len(srl[0]) < 2, whole=whole, ranges=[], at_left=[], at_right=[], per_range=[])
    if not out["nothing"]:
        out["ranges"] = fl.consreg_groups(codes, srl, alp, thr, weight, dissim=True)
        for l, r in out["ranges"]:
            out["at_left"].append(int(l == 0))
            out["at_right"].append(int(r == ln))
            out["per_range"].append(fl.consregss(codes, srl, alp, weight, l, r))
    return out


def rows_without_common_gaps(codes, members):
    """the rows of some members with the columns dropped that are all gaps in them"""
    sub = np.asarray(codes)[:, list(members)]
    return sub[(sub > 1).any(1)]


def family_in_groups():
    """a 10-member family over an ancestor of 200 residues, in groups of 4, 3, 1 and 2 with unsorted lists: (codes, groups)"""
    from prrn_aln_amd import operator as op
    from prrn_aln_amd.synth import make_family
    rows = list(make_family(n_seq=10, length=200, seed=77, indel=0.05, max_indel=6).msa)
    return op.encode(rows, 1), [np.array(g, np.int32) for g in ([0, 3, 1, 2], [6, 4, 5], [7], [9, 8])]
