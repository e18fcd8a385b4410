"""Restatement of the reference's group fusing and of what IterMsa::preprrn decides with it (src/consreg.cc:452-464, 569-589, 667-711,
484-518; src/prrn5.cc:794-823) in plain Python, on top of tests/consreglib.py (column scores of the library's HOST-built pairs):

    fthr        Conserved2::fthr (consreg.cc:73): (VTYPE) -((2 * u + v)) * a->sumwt * b->sumwt with u, v floats
    fuse_scan   the recurrence of may_fuse_ng / _nv / _hf / _pf: scr += s; a positive scr becomes 0; break where scr < fthr
    testssrel   ConservedT::testssrel: the post-order walk, its tests in the reference's order, the groups in leaf post-order
    rearrange   ConservedT::rearrange: the tree over the new groups
    consregss   Ssrel::consregss on a column range
    grouped_divisions / consreg_groups   Ssrel::consreg over a relation with groups (Randiv::tree_tab + bin2lst2g)
    plan        preprrn's decisions

A relation is (groups, left, right, parent, vol, cur): groups a list of member lists, leaf g of the tree is group g."""
import glob
import os

import numpy as np

import consreglib as cl

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "fuse")


def fixtures():
    return [(os.path.basename(f)[:-4], dict(np.load(f))) for f in sorted(glob.glob(os.path.join(GOLD, "*.npz")))]


def fthr(u, v, sumwt_a, sumwt_b):
    f = -(np.float32(2) * np.float32(u) + np.float32(v))                    # float arithmetic, then the cast to VTYPE = double
    return float(np.float64(f)) * float(sumwt_a) * float(sumwt_b)


def fuse_scan(s, thr):
    """(fuse 0 / 1, stop_col): stop_col the column at which scr < fthr first held, -1 when the walk reached the end"""
    scr = 0.0
    for i, x in enumerate(s):
        scr += float(x)
        if scr > 0:
            scr = 0.0
        if scr < thr:
            return 0, i
    return 1, -1


def pair_fthr(pw, u, v):
    p = pw.problem
    return fthr(u, v, p.a.sumwt, p.b.sumwt)


def may_fuse(codes, l0, l1, alp, weight=None, left=0, right=None):
    """the fuse test of two member lists over the columns [left, right): (fuse, stop_col, alnmode)"""
    right = codes.shape[0] if right is None else right
    pw = cl.host_pair(codes[left:right], (list(l0), list(l1)), alp, weight)
    f, c = fuse_scan(cl.colscores(pw.problem), pair_fthr(pw, alp.u, alp.v))
    return f, c, pw.alnmode


def root_of(parent):
    r = [k for k in range(len(parent)) if parent[k] < 0]
    assert len(r) == 1
    return r[0]


def testssrel(groups, left, right, parent, test):
    """test(list0, list1) -> truthy when the two lists fuse.  Returns (new groups, leaf): leaf[k] the group a node stands for or -1 --
    set for leaves and fused nodes, as ConservedT::leaf is"""
    leaf = [-1] * len(left)
    out = []

    def walk(k):
        if left[k] < 0:
            out.append(list(groups[k]))
            leaf[k] = len(out) - 1
            return leaf[k]
        lt = walk(int(left[k]))
        rt = walk(int(right[k]))
        if lt >= 0 and rt >= 0:
            assert rt == lt + 1 == len(out) - 1
            if test(out[lt], out[rt]):
                out[lt] = out[lt] + out.pop()
                leaf[k] = lt
                return lt
        return -1
    walk(root_of(parent))
    return out, leaf


def rearrange(leaf, n, left, right, parent, vol, cur):
    """the tree over n groups: (left, right, parent, vol, cur, origin) as int32 / float64 arrays of 2 n - 1 nodes"""
    nn = 2 * n - 1
    nl, nr, npar, org = (np.full(nn, -1, np.int32) for _ in range(4))
    nv, nc = np.zeros(nn), np.zeros(nn)
    ntid = [n]

    def walk(k):
        ilf = leaf[k] >= 0
        if not ilf:
            lf, rt = walk(int(left[k])), walk(int(right[k]))
            t = ntid[0]
            ntid[0] += 1
        else:
            t = leaf[k]
        org[t], nv[t], nc[t] = k, vol[k], cur[k]
        if not ilf:
            nl[t], nr[t] = lf, rt
            npar[lf] = npar[rt] = t
        return t
    walk(root_of(parent))
    assert ntid[0] == nn or n == 1
    return nl, nr, npar, nv, nc, org


def consregss(codes, rel, alp, weight=None, left=0, right=None, tests=None):
    """Ssrel::consregss on the columns [left, right): (fused, relation, origin); tests (a list) receives (list0, list1, fuse, stop_col,
    alnmode) of every test in the reference's order"""
    groups, tl, tr, tp, vol, cur = rel

    def test(l0, l1):
        f, c, mode = may_fuse(codes, l0, l1, alp, weight, left, right)
        if tests is not None:
            tests.append((list(l0), list(l1), f, c, mode))
        return f
    out, leaf = testssrel(groups, tl, tr, tp, test)
    if len(out) == len(groups):
        return 0, rel, np.arange(len(tl), dtype=np.int32)
    nl, nr, npar, nv, nc, org = rearrange(leaf, len(out), tl, tr, tp, vol, cur)
    return 1, (out, nl, nr, npar, nv, nc), org


def grouped_divisions(groups, left, right, parent):
    """[(son 0, son 1)] for node 0 .. 2 num - 4 of the tree over the groups: the groups in ascending order, each handing over its members
    in its own order (bin2lst2g, src/randiv.cc:88-100)"""
    num = len(groups)
    below = {}

    def leaves(k):
        if k not in below:
            below[k] = {k} if left[k] < 0 else leaves(int(left[k])) | leaves(int(right[k]))
        return below[k]
    out = []
    for k in range(2 * num - 3):
        ins = leaves(k)
        sons = ([], [])
        for g in range(num):
            sons[1 if g in ins else 0].extend(int(m) for m in groups[g])
        out.append(sons)
    return out


def consreg_groups(codes, rel, alp, thr, weight=None, dissim=False):
    groups, tl, tr, tp = rel[:4]
    ln = codes.shape[0]
    united = [(0, ln)]
    for lists in grouped_divisions(groups, tl, tr, tp):
        pw = cl.host_pair(codes, lists, alp, weight)
        united = cl.cmnrng(united, cl.scan(cl.colscores(pw.problem), cl.vthr_of(pw, thr)))
    return cl.complerng(ln, united) if dissim else united


def rounds_of(groups, left, right, parent, leaf):
    """how many level-by-level rounds the tests of a walk take: the height of the tallest tested node over the leaves"""
    depth = {}

    def h(k):
        if k not in depth:
            depth[k] = 0 if left[k] < 0 else 1 + max(h(int(left[k])), h(int(right[k])))
        return depth[k]
    tested = [k for k in range(len(groups), len(left)) if leaf[int(left[k])] >= 0 and leaf[int(right[k])] >= 0]
    return max([h(k) for k in tested] or [0])


def fuse_rounds(codes, rel, alp, weight=None, left=0, right=None):
    """(tests, rounds) of one fusing run level by level"""
    t = []
    out, leaf = testssrel(rel[0], rel[1], rel[2], rel[3], lambda a, b: (t.append(0), may_fuse(codes, a, b, alp, weight, left, right)[0])[1])
    return len(t), rounds_of(rel[0], rel[1], rel[2], rel[3], leaf)


def plan(codes, tree, alp, thr, weight=None):
    """preprrn's decisions: dict(nothing, whole = (fused, relation, origin), ranges, at_left, at_right, per_range = [(fused, relation,
    origin)], tests = the count of fuse tests)"""
    ln, many = codes.shape
    tl, tr, tp, vol, cur = tree
    rel0 = ([[m] for m in range(many)], tl, tr, tp, vol, cur)
    tests = []
    whole = consregss(codes, rel0, alp, weight, tests=tests)
    srl = whole[1]
    out = dict(nothing=len(srl[0]) < 2, whole=whole, ranges=[], at_left=[], at_right=[], per_range=[])
    if not out["nothing"]:
        out["ranges"] = consreg_groups(codes, srl, alp, thr, weight, dissim=True)
        for l, r in out["ranges"]:
            out["at_left"].append(int(l == 0))
            out["at_right"].append(int(r == ln))
            out["per_range"].append(consregss(codes, srl, alp, weight, l, r, tests=tests))
    out["tests"] = len(tests)
    return out


# ---- the fixtures --------------------------------------------------------------------------------------------------------------------
def unpack_lists(g, key):
    off = g[key + "_off"]
    return [[int(x) for x in g[key][off[k]:off[k + 1]]] for k in range(len(off) - 1)]


def fixture_tree(g, pfx="tree"):
    return tuple(g["%s_%s" % (pfx, k)] for k in ("left", "right", "parent", "vol", "cur"))


def fixture_relation(g, pfx):
    """(fused, groups, left, right, parent, vol, cur) of a recorded relation; fused 0: the arrays are empty (the reference's NULL)"""
    fused = int(g[pfx + "_fused"][0])
    if not fused:
        return 0, None
    return 1, (unpack_lists(g, pfx + "_grp"),) + fixture_tree(g, pfx)


def fixture_tests(g, pfx="test"):
    """[(list0, list1, outcome, alnmode)] of a fusing in the reference's order: "test" the whole MSA's, "r<i>_test" range i's"""
    return list(zip(unpack_lists(g, pfx + "_l0"), unpack_lists(g, pfx + "_l1"), g[pfx + "_fuse"].tolist(), g[pfx + "_mode"].tolist()))


def all_fixture_tests(g):
    """[(left, right, list0, list1, outcome, alnmode)]: the whole-MSA tests and every range's"""
    ln = g["codes"].shape[0]
    out = [(0, ln) + t for t in fixture_tests(g)]
    for i, (l, r) in enumerate(g["gunited1"].tolist()):
        out += [(l, r) + t for t in fixture_tests(g, "r%d_test" % i)]
    return out
