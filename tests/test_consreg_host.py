"""The conserved-region search on the host: the Python restatement (tests/consreglib.py, on the library's host-built PwdMs) against
what the REFERENCE computed (tests/golden/consreg: per-division ranges of Ssrel::constwo, united ranges of Ssrel::consreg for both
dissim), cmnrng / complerng -- restatement and library (g2g_ranges_combine) -- on hand-made lists, and the refusals of
g2g_constwo_batch / g2g_consreg that need no device."""
import ctypes as C

import numpy as np
import pytest

import consreglib as cl
from prrn_aln_amd import _abi, guide, operator as op
from prrn_aln_amd._lib import G2GError, last_error, lib

FIX = cl.fixtures()
IDS = [n for n, _ in FIX]
G2G_ERR_ARG, G2G_ERR_MODE = -1, -2


def test_the_set_of_fixtures():
    assert len(FIX) == 8
    modes = set()
    for _, g in FIX:
        ln, many = g["codes"].shape
        assert 6 <= many <= 16 and 120 <= ln <= 400
        assert int(g["div_in_tree"].sum()) == 2 * many - 3
        assert max(len(d[2]) for d in cl.fixture_divisions(g)) >= 4
    assert sum(1 for _, g in FIX if len(g["united0"]) == 0) == 1
    assert any(len(g["weight"]) for _, g in FIX) and any(int(g["molc"][0]) == 2 for _, g in FIX)
    assert any(float(g["u"][0]) != 3. and float(g["v"][0]) != 10. for _, g in FIX)


@pytest.mark.parametrize("k", range(len(FIX)), ids=IDS)
def test_restatement_reproduces_the_reference(k):
    name, g = FIX[k]
    codes, alp, thr = g["codes"], cl.alp_of(g), float(g["thr"][0])
    weight = g["weight"] if len(g["weight"]) else None
    ln, many = codes.shape
    tree_divs = cl.divisions(g["tree_left"], g["tree_right"], g["tree_parent"], many)
    united = [(0, ln)]
    n_tree = 0
    for l0, l1, want, in_tree in cl.fixture_divisions(g):
        pw = cl.host_pair(codes, (l0, l1), alp, weight)
        got = cl.scan(cl.colscores(pw.problem), cl.vthr_of(pw, thr))
        assert got == want, (name, l0, l1)
        if in_tree:
            assert (l0, l1) == tree_divs[n_tree]                         # the divisions of the recorded tree, in Randiv's numbering
            n_tree += 1
            united = cl.cmnrng(united, got)
    assert n_tree == len(tree_divs)
    assert united == [tuple(r) for r in g["united0"].tolist()]
    assert cl.complerng(ln, united) == [tuple(r) for r in g["united1"].tolist()]


def test_all_four_branches_of_constwo_occur():
    """through the library's own alnmode: NGP -> cons2_ng, NTV -> cons2_nv, HLF and RHF -> cons2_hf, GPF -> cons2_pf"""
    seen = set()
    for name, g in FIX:
        alp = cl.alp_of(g)
        weight = g["weight"] if len(g["weight"]) else None
        divs = cl.fixture_divisions(g)
        for k in sorted({int(np.flatnonzero(g["div_mode"] == m)[0]) for m in set(g["div_mode"].tolist())}):
            pw = cl.host_pair(g["codes"], divs[k][:2], alp, weight)
            assert pw.alnmode == int(g["div_mode"][k])
            seen.add(pw.alnmode)
    assert seen == {cl.NGP_ALB, cl.HLF_ALB, cl.RHF_ALB, cl.GPF_ALB, cl.NTV_ALB}


RANGE_CASES = [
    ([(0, 10)], [(0, 10)]),
    ([(0, 5), (5, 9)], [(3, 7)]),                      # touching ranges
    ([(0, 5), (5, 9)], [(5, 6)]),
    ([(2, 4)], [(4, 8)]),                              # touching, nothing in common
    ([], [(1, 3)]),                                    # empty operands
    ([(1, 3)], []),
    ([], []),
    ([(0, 3), (6, 20)], [(2, 7), (9, 12), (15, 20)]),  # a range ending at len = 20
    ([(0, 20)], [(0, 1), (19, 20)]),
    ([(1, 2), (3, 4), (5, 6)], [(0, 10)]),
    ([(0, 4), (4, 8)], [(0, 8)]),
]


@pytest.mark.parametrize("a,b", RANGE_CASES)
def test_cmnrng_and_complerng(a, b):
    ln = 20
    cover = lambda r: {c for l, rr in r for c in range(l, rr)}
    got = cl.cmnrng(a, b)
    assert cover(got) == cover(a) & cover(b) and all(l < r for l, r in got) and got == sorted(got)
    assert got == cl.cmnrng(b, a)
    assert [tuple(x) for x in guide.ranges_intersect(a, b).tolist()] == got
    for r in (a, b, got):
        comp = cl.complerng(ln, r)
        assert cover(comp) == set(range(ln)) - cover(r) and all(l < rr for l, rr in comp)
        assert [tuple(x) for x in guide.ranges_complement(r, ln).tolist()] == comp
        assert cl.complerng(ln, comp) == sorted((min(c), max(c) + 1) for c in _runs(cover(r)))


def _runs(cols):
    out, cur = [], []
    for c in sorted(cols):
        if cur and c != cur[-1] + 1:
            out.append(cur); cur = []
        cur.append(c)
    return out + ([cur] if cur else [])


def test_scan_by_hand():
    # one range opens at the first positive score, closes where the sum peaked, and is emitted once the sum has fallen by vthr
    s = [-1., 2., 3., -1., 4., -9., -9., 1., 1.]
    assert cl.scan(s, 5.) == [(1, 5)]
    assert cl.scan(s, 8.) == [(1, 5)]
    assert cl.scan(s, 8.5) == []
    assert cl.scan([3.] * 4, 5.) == [(0, 4)]                              # still open at the end
    assert cl.scan([], 5.) == [] and cl.scan([-1.] * 5, 5.) == []


def _pair(rows_a, rows_b, **kw):
    alp = op.AlnParam(u=3., v=10., u0=0., u1=0., ls=2, sh=100, **kw)
    return op.PwdM([op.mSeq(rows_a, alp), op.mSeq(rows_b, alp)], alp), alp


def _constwo_rc(pwds, thr=35.):
    n = len(pwds)
    hs = (C.c_void_p * max(1, n))(*[p._h for p in pwds])
    rng = (C.POINTER(_abi.Range) * max(1, n))()
    nr = (C.c_int * max(1, n))()
    return lib().g2g_constwo_batch(None, n, hs, float(thr), rng, nr, None, None)


def test_constwo_batch_refusals():
    good, _ = _pair(["ACDEFGHIKL", "ACDEFGHIKL"], ["ACDEFGHIKL"])
    assert _constwo_rc([good], thr=0.) == G2G_ERR_ARG and "thr" in last_error()
    assert _constwo_rc([good], thr=-1.) == G2G_ERR_ARG
    unequal, _ = _pair(["ACDEFGHIKL", "ACDEFGHIKL"], ["ACDEFGHIK"])
    assert _constwo_rc([good, unequal]) == G2G_ERR_ARG and "pair 1" in last_error() and "same length" in last_error()
    unbanded, _ = _pair(["ACDEFGHIKL", "ACDEFGHIKL"], ["ACDEFGHIKL"], banded=0)
    assert _constwo_rc([unbanded]) == G2G_ERR_MODE and "banded" in last_error()
    # well-formed arguments without a context: refused as an argument, never computed on the host
    assert _constwo_rc([good]) == G2G_ERR_ARG and "context" in last_error()
    with pytest.raises(G2GError):
        guide.constwo_batch(None, [good])


def test_consreg_refusals():
    name, g = FIX[0]
    codes, alp = g["codes"], cl.alp_of(g)

    class T:
        left, right, parent = g["tree_left"], g["tree_right"], g["tree_parent"]
    call = lambda a=alp, t=T, c=codes, thr=35.: guide.conserved_regions(None, c, t, a.to_c()[0], thr)
    for kw, word in ((dict(banded=0), "banded"), (dict(u0=1.), "u0"), (dict(tgapf=0.5), "terminal")):
        a2 = cl.alp_of(g)
        for k, v in kw.items():
            setattr(a2, k, v)
        with pytest.raises(G2GError, match="rc=%d.*%s" % (G2G_ERR_MODE, word)):
            call(a=a2)
    with pytest.raises(G2GError, match="rc=%d.*thr" % G2G_ERR_ARG):
        call(thr=0.)
    with pytest.raises(G2GError, match="rc=%d.*three" % G2G_ERR_ARG):
        class T2:
            left, right, parent = np.array([-1, -1, 0], np.int32), np.array([-1, -1, 1], np.int32), np.array([2, 2, -1], np.int32)
        call(t=T2, c=codes[:, :2])

    class Bad:
        left, right, parent = g["tree_left"].copy(), g["tree_right"], g["tree_parent"]
    Bad.left[len(Bad.left) - 1] = 0                                       # the root takes a leaf that hangs elsewhere
    with pytest.raises(G2GError, match="rc=%d.*tree" % G2G_ERR_ARG):
        call(t=Bad)
    with pytest.raises(G2GError, match="rc=%d.*context" % G2G_ERR_ARG):   # everything in order but no device context
        call()
