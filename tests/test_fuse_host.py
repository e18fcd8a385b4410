"""Group fusing and preprrn's plan on the host: the Python restatement (tests/fuselib.py, on the library's host-built PwdMs) against what
the REFERENCE computed (tests/golden/fuse: every fuse test of ConservedT::testssrel, the subset and tree of Ssrel::consregss, the
grouped Ssrel::consreg, every attack range's own relation), the recurrence and ConservedT::rearrange by hand, and the new entry points:
that they exist and that their refusals need no device."""
import ctypes as C

import numpy as np
import pytest

import consreglib as cl
import fuselib as fl
from prrn_aln_amd import _abi, guide, operator as op
from prrn_aln_amd._lib import G2GError, last_error, lib

FIX = fl.fixtures()
IDS = [n for n, _ in FIX]
G2G_ERR_ARG, G2G_ERR_MODE = -1, -2
bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.int64)


def weight_of(g):
    return g["weight"] if len(g["weight"]) else None


def same_relation(got, want):
    """got: a fuselib relation; want: (groups, left, right, parent, vol, cur) as recorded"""
    assert [list(map(int, x)) for x in got[0]] == want[0]
    for a, b in zip(got[1:4], want[1:4]):
        assert np.array_equal(a, b)
    for a, b in zip(got[4:6], want[4:6]):
        assert np.array_equal(bits(a), bits(b))


def test_the_set_of_fixtures():
    assert 8 <= len(FIX) <= 10
    modes, fused_modes = set(), set()
    for name, g in FIX:
        ln, many = g["codes"].shape
        assert 6 <= many <= 16 and 120 <= ln <= 400, name
        t = fl.fixture_tests(g)
        modes |= {m for _, _, _, _, _, m in fl.all_fixture_tests(g)}
        fused_modes |= {m for _, _, _, _, f, m in fl.all_fixture_tests(g) if f}
        if name not in ("prot8_all_fused", "prot6_none_fused"):
            n = len(fl.unpack_lists(g, "whole_grp"))
            assert any(f for _, _, f, _ in t) and any(not f for _, _, f, _ in t) and 1 < n < many, name
    assert modes == {cl.NGP_ALB, cl.HLF_ALB, cl.RHF_ALB, cl.GPF_ALB, cl.NTV_ALB}
    assert {cl.NGP_ALB, cl.RHF_ALB, cl.GPF_ALB, cl.NTV_ALB} <= fused_modes          # (no HLF test of the set fuses: pinned by refusals)
    by = dict(FIX)
    assert len(fl.unpack_lists(by["prot8_all_fused"], "whole_grp")) == 1 and int(by["prot8_all_fused"]["nrange"][0]) == 0
    assert int(by["prot6_none_fused"]["whole_fused"][0]) == 0
    assert any(len(g["weight"]) for _, g in FIX) and any(int(g["molc"][0]) == 2 for _, g in FIX)
    assert any(float(g["u"][0]) == float(np.float32(2.1)) and float(g["v"][0]) == float(np.float32(9.3)) for _, g in FIX)
    two = by["prot12_two_rounds"]                                                       # whole-MSA fusing, then more inside a range
    assert int(two["whole_fused"][0]) == 1 and any(int(two["r%d_fused" % i][0]) for i in range(int(two["nrange"][0])))


@pytest.mark.parametrize("k", range(len(FIX)), ids=IDS)
def test_restatement_reproduces_the_reference(k):
    name, g = FIX[k]
    codes, alp, thr, weight = g["codes"], cl.alp_of(g), float(g["thr"][0]), weight_of(g)
    ln, many = codes.shape
    tree = fl.fixture_tree(g)
    rel0 = ([[m] for m in range(many)],) + tree
    tests = []
    fused, srl, org = fl.consregss(codes, rel0, alp, weight, tests=tests)
    assert [(a, b, f, m) for a, b, f, c, m in tests] == fl.fixture_tests(g)
    assert all((c < 0) == bool(f) and -1 <= c < ln for _, _, f, c, _ in tests)
    want_fused, want = fl.fixture_relation(g, "whole")
    assert fused == want_fused
    if fused:
        same_relation(srl, want)
        assert all(np.array_equal(bits(np.asarray(srl[4 + i])), bits(np.asarray(tree[3 + i])[org])) for i in (0, 1))     # vol / cur are copies
    else:
        assert srl is rel0
    if len(srl[0]) < 2:
        assert int(g["nrange"][0]) == 0 and len(g["gunited1"]) == 0
        return
    for dissim in (0, 1):
        assert fl.consreg_groups(codes, srl, alp, thr, weight, bool(dissim)) == [tuple(r) for r in g["gunited%d" % dissim].tolist()]
    atk = [tuple(r) for r in g["gunited1"].tolist()]
    assert int(g["nrange"][0]) == len(atk)
    for i, (l, r) in enumerate(atk):
        t = []
        f, rel, _ = fl.consregss(codes, srl, alp, weight, l, r, tests=t)
        wf, w = fl.fixture_relation(g, "r%d" % i)
        assert f == wf and [(a, b, x, m) for a, b, x, c, m in t] == fl.fixture_tests(g, "r%d_test" % i)
        if f:
            same_relation(rel, w)
    p = fl.plan(codes, tree, alp, thr, weight)
    assert p["ranges"] == atk and p["at_left"] == [int(l == 0) for l, _ in atk] and p["at_right"] == [int(r == ln) for _, r in atk]


def test_fuse_scan_by_hand():
    assert fl.fuse_scan([], -16.) == (1, -1)
    assert fl.fuse_scan([-17.], -16.) == (0, 0)                           # a break in the first column
    assert fl.fuse_scan([1., 1., -17.], -16.) == (0, 2)                   # ... in the last one
    assert fl.fuse_scan([-8., -8.], -16.) == (1, -1)                      # scr == fthr does not break
    eps = np.nextafter(16., 17.) - 16.                                     # (-8 - (8 + eps) is the double below -16)
    assert fl.fuse_scan([-8., -(8. + eps)], -16.) == (0, 1)               # one ulp below it does
    assert fl.fuse_scan([100., -10., -6.], -16.) == (1, -1)               # a positive scr is clamped to 0, it buys nothing later
    assert fl.fuse_scan([100., -10., -7.], -16.) == (0, 2)
    assert fl.fuse_scan([-10., 4., -10.], -16.) == (1, -1)                # ... a negative one is kept: -10 + 4 - 10 = -16
    assert fl.fuse_scan([-10., 3., -10.], -16.) == (0, 2)
    assert fl.fuse_scan([-10., 11., -10.], -16.) == (1, -1)


def test_fthr_is_formed_as_the_reference_forms_it():
    assert fl.fthr(3., 10., 1., 1.) == -16. and fl.fthr(3., 10., 4., 3.) == -192.
    f = -(np.float32(2) * np.float32(2.1) + np.float32(9.3))              # floats, then the cast, then the products from left to right
    assert fl.fthr(2.1, 9.3, 1.3, 0.7) == float(f) * 1.3 * 0.7
    assert fl.fthr(0.1, 0.2, 1., 1.) == -float(np.float32(2) * np.float32(0.1) + np.float32(0.2)) != -(2 * 0.1 + 0.2)


def test_rearrange_by_hand():
    #            8
    #          /   \
    #         6     7          leaves 0 .. 4; 5 = (0, 1), 6 = (5, 2), 7 = (3, 4), 8 = (6, 7)
    #        / \   / \
    #       5   2 3   4
    #      / \
    #     0   1
    left = np.array([-1, -1, -1, -1, -1, 0, 5, 3, 6], np.int32)
    right = np.array([-1, -1, -1, -1, -1, 1, 2, 4, 7], np.int32)
    parent = np.array([5, 5, 6, 7, 7, 6, 8, 8, -1], np.int32)
    vol, cur = np.arange(9) * 1.5, np.arange(9) * 0.25
    groups = [[m] for m in range(5)]
    asked = []

    def test(l0, l1):
        asked.append((list(l0), list(l1)))
        return (l0, l1) in (([0], [1]), ([3], [4]))                       # 5 and 7 fuse, 6 is refused: 8 is never tested
    out, leaf = fl.testssrel(groups, left, right, parent, test)
    assert asked == [([0], [1]), ([0, 1], [2]), ([3], [4])]
    assert out == [[0, 1], [2], [3, 4]] and leaf == [0, 1, 1, 2, 3, 0, -1, 2, -1]
    nl, nr, npar, nv, nc, org = fl.rearrange(leaf, 3, left, right, parent, vol, cur)
    # the groups are leaves 0, 1, 2; node 6 becomes 3 (made first in post-order), the root 4
    assert nl.tolist() == [-1, -1, -1, 0, 3] and nr.tolist() == [-1, -1, -1, 1, 2] and npar.tolist() == [3, 3, 4, 4, -1]
    assert org.tolist() == [5, 2, 7, 6, 8] and nv.tolist() == (org * 1.5).tolist() and nc.tolist() == (org * 0.25).tolist()
    assert fl.grouped_divisions(out, nl, nr, npar) == [([2, 3, 4], [0, 1]), ([0, 1, 3, 4], [2]), ([0, 1, 2], [3, 4])]
    # everything fused: one group, a tree of one node copied from the root
    out, leaf = fl.testssrel(groups, left, right, parent, lambda a, b: True)
    assert out == [[0, 1, 2, 3, 4]]
    nl, nr, npar, nv, nc, org = fl.rearrange(leaf, 1, left, right, parent, vol, cur)
    assert nl.tolist() == [-1] and npar.tolist() == [-1] and org.tolist() == [8]
    # two groups: one division
    assert fl.grouped_divisions([[0, 1, 2], [3, 4]], [-1, -1, 0], [-1, -1, 1], [2, 2, -1]) == [([3, 4], [0, 1, 2])]


# ---- the new entry points: present, and their refusals need no device --------------------------------------------------------------------
def test_the_new_symbols_exist():
    L = lib()
    for name in ("g2g_mayfuse_batch", "g2g_consregss", "g2g_consreg_groups", "g2g_refine_plan", "g2g_refine_plan_free", "g2g_relation_free", "g2g_subset_free"):
        assert getattr(L, name)
    for name in ("may_fuse_batch", "fuse_groups", "conserved_regions_groups", "refine_plan"):
        assert callable(getattr(guide, name))


def _pair(rows_a, rows_b, **kw):
    alp = op.AlnParam(u=3., v=10., u0=0., u1=0., ls=2, sh=100, **kw)
    return op.PwdM([op.mSeq(rows_a, alp), op.mSeq(rows_b, alp)], alp)


def _mayfuse_rc(pwds, u=3., v=10.):
    n = len(pwds)
    hs = (C.c_void_p * max(1, n))(*[p._h for p in pwds])
    fz, sc = (C.c_int * max(1, n))(), (C.c_int * max(1, n))()
    return lib().g2g_mayfuse_batch(None, n, hs, float(u), float(v), fz, sc, None)


def test_mayfuse_batch_refusals():
    good = _pair(["ACDEFGHIKL", "ACDEFGHIKL"], ["ACDEFGHIKL"])
    unequal = _pair(["ACDEFGHIKL", "ACDEFGHIKL"], ["ACDEFGHIK"])
    assert _mayfuse_rc([good, unequal]) == G2G_ERR_ARG and "pair 1" in last_error() and "same length" in last_error()
    unbanded = _pair(["ACDEFGHIKL", "ACDEFGHIKL"], ["ACDEFGHIKL"], banded=0)
    assert _mayfuse_rc([unbanded]) == G2G_ERR_MODE and "banded" in last_error()
    discounted = _pair(["-CDEFGHIKL", "ACDEFGHIKL"], ["ACDEFGHIKL"], tgapf=0.5)
    assert _mayfuse_rc([discounted]) == G2G_ERR_MODE and "terminal" in last_error()
    assert _mayfuse_rc([good], u=-1.) == G2G_ERR_ARG
    # the masks of the members whose runs are read must fit 48 KB of LDS: 36 bytes each
    wide, pair = np.full((12, 1400), 5, np.uint8), np.full((12, 2), 7, np.uint8)
    pair[4:6, 0] = 1
    alp = op.AlnParam(u=3., v=10., u0=0., u1=0., ls=2, sh=100)
    for a, b in ((pair, wide), (wide, pair)):
        assert _mayfuse_rc([op.PwdM([op.mSeq(a, alp), op.mSeq(b, alp)], alp)]) == G2G_ERR_MODE and "1365 members" in last_error()
    # well-formed arguments without a context: refused as an argument, never computed on the host
    assert _mayfuse_rc([good]) == G2G_ERR_ARG and "context" in last_error() and "g2g_mayfuse_batch" in last_error()
    with pytest.raises(G2GError, match="context"):
        guide.may_fuse_batch(None, [good])


class _Tree:
    def __init__(self, g, pfx="tree"):
        self.left, self.right, self.parent, self.vol, self.cur = (np.array(a) for a in fl.fixture_tree(g, pfx))


def _alp(g, **kw):
    a = cl.alp_of(g)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_consregss_refusals():
    g = dict(FIX)["prot12_clusters"]
    codes, t = g["codes"], _Tree(g)
    ln, many = codes.shape
    call = lambda a=None, tree=t, c=codes, **kw: guide.fuse_groups(None, c, tree, (a or cl.alp_of(g)).to_c()[0], **kw)
    for kw, word in ((dict(banded=0), "banded"), (dict(u0=1.), "u0"), (dict(tgapf=0.5), "terminal")):
        with pytest.raises(G2GError, match="g2g_consregss rc=%d.*%s" % (G2G_ERR_MODE, word)):
            call(a=_alp(g, **kw))
    for kw in (dict(left=5, right=5), dict(left=-1), dict(right=ln + 1), dict(left=9, right=3)):
        with pytest.raises(G2GError, match="rc=%d.*range" % G2G_ERR_ARG):
            call(**kw)
    with pytest.raises(G2GError, match="rc=%d.*two members" % G2G_ERR_ARG):
        call(c=codes[:, :1], tree=_Tree(dict(tree_left=[-1], tree_right=[-1], tree_parent=[-1], tree_vol=[0.], tree_cur=[0.])))
    bad = _Tree(g)
    bad.left[len(bad.left) - 1] = 0                                       # the root takes a leaf that hangs elsewhere
    with pytest.raises(G2GError, match="rc=%d.*tree" % G2G_ERR_ARG):
        call(tree=bad)
    singles = [[m] for m in range(many)]
    for groups in (singles[:-1] + [[0]], singles[:-1] + [[many]], singles[:-1] + [[]]):
        with pytest.raises(G2GError, match="rc=%d.*subset" % G2G_ERR_ARG):
            call(groups=groups)
    with pytest.raises(G2GError, match="rc=%d.*tree" % G2G_ERR_ARG):      # three groups need a tree of five nodes
        call(groups=[[0, 1, 2, 3], [4, 5, 6, 7], [8, 9, 10, 11]])
    with pytest.raises(G2GError, match="rc=%d.*context" % G2G_ERR_ARG):   # everything in order but no device context
        call()
    with pytest.raises(G2GError, match="rc=%d.*context" % G2G_ERR_ARG):
        call(groups=singles, left=3, right=40)


def test_consreg_groups_refusals():
    g = dict(FIX)["prot12_clusters"]
    codes = g["codes"]
    _, whole = fl.fixture_relation(g, "whole")
    wt = _Tree(g, "whole")
    call = lambda a=None, tree=wt, groups=whole[0], thr=35.: guide.conserved_regions_groups(None, codes, tree, (a or cl.alp_of(g)).to_c()[0], groups, thr)
    for kw, word in ((dict(banded=0), "banded"), (dict(u0=1.), "u0"), (dict(tgapf=0.5), "terminal")):
        with pytest.raises(G2GError, match="g2g_consreg_groups rc=%d.*%s" % (G2G_ERR_MODE, word)):
            call(a=_alp(g, **kw))
    with pytest.raises(G2GError, match="rc=%d.*thr" % G2G_ERR_ARG):
        call(thr=0.)
    with pytest.raises(G2GError, match="rc=%d.*tree" % G2G_ERR_ARG):      # the tree of the members is not a tree over three groups
        call(tree=_Tree(g))
    with pytest.raises(G2GError, match="rc=%d.*subset" % G2G_ERR_ARG):
        call(groups=[whole[0][0], whole[0][1], whole[0][2][:-1] + [whole[0][0][0]]])
    with pytest.raises(G2GError, match="rc=%d.*two groups" % G2G_ERR_ARG):
        call(groups=[sum(whole[0], [])], tree=_Tree(dict(tree_left=[-1], tree_right=[-1], tree_parent=[-1], tree_vol=[0.], tree_cur=[0.])))
    with pytest.raises(G2GError, match="rc=%d.*context" % G2G_ERR_ARG):
        call()
    with pytest.raises(G2GError, match="rc=%d.*context" % G2G_ERR_ARG):   # without groups: g2g_consreg's driver
        call(tree=_Tree(g), groups=None)


def test_refine_plan_refusals():
    g = dict(FIX)["prot12_clusters"]
    codes, t = g["codes"], _Tree(g)
    call = lambda a=None, tree=t, thr=35.: guide.refine_plan(None, codes, tree, (a or cl.alp_of(g)).to_c()[0], thr)
    for kw, word in ((dict(banded=0), "banded"), (dict(u0=1.), "u0"), (dict(tgapf=0.5), "terminal")):
        with pytest.raises(G2GError, match="g2g_refine_plan rc=%d.*%s" % (G2G_ERR_MODE, word)):
            call(a=_alp(g, **kw))
    with pytest.raises(G2GError, match="rc=%d.*thr" % G2G_ERR_ARG):
        call(thr=-1.)
    bad = _Tree(g)
    bad.parent[0] = -1                                                    # a second root
    with pytest.raises(G2GError, match="rc=%d.*tree" % G2G_ERR_ARG):
        call(tree=bad)
    with pytest.raises(G2GError, match="rc=%d.*context" % G2G_ERR_ARG):
        call()
