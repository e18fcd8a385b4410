"""The X merges of the v6 `_pf` strips run a compile-time bucket of slots (4, 8, 12, 16; 4, 8, 10 with Noll 3) picked from the
wave's longest row t list (v6_cell_pf, g2g_kernels_v6.hip).  These cases put that length on both sides of every bucket edge, in
the first strip, in the last (partial) strip and across a strip boundary, and mix the lengths in one launch.

Inputs are built by hand: group a has K + 2 members of 150 columns, member j >= 2 with one gap run of j - 1 columns that ends
just before column c0; group b has four members of 140 columns with a few gap runs of its own.  Row c0 - 1 of a then carries a
t list of K entries (rows c0 - K .. c0 - 1 carry 1 .. K) and row c0 an s list of K + 1, every other row at most one: the strip
that holds row c0 - 1 runs its X merges with a longest t list of K.  Each test checks those lengths in the problem it built.

The engine takes a `_pf` DP on v6 only while a's longest list WITH its terminator fits the register slots (maxlist <= 16;
<= 10 with Noll 3): the s list of K + 1 entries makes that K <= 14 (K <= 8 with Noll 3).  K = 15 (K = 9 with Noll 3) built this
way is kept as a case: it must NOT run on v6, and its result is checked all the same.  Those two lengths reach v6 from a group
whose members are ALL gapped (test_longest_t_lists_v6_takes): its longest s list has K entries, not K + 1.  Expected values:
the CPU oracle (score equal as a double, equal skeleton, status 0)."""
import numpy as np
import pytest

import oraclelib
from prrn_aln_amd import engine, operator as op
from widelib import base as _base, list_lengths, member as _member, stair as group_a

pytestmark = pytest.mark.gpu

LEN_A, LEN_B = 150, 140
SLOTS = {2: 16, 3: 10}                          # G2G_V6_NA / G2G_V6_NA3: register slots of a row list (terminator included)
FIRST, LAST, ACROSS = 60, 140, 65               # c0: long lists in strip 0 / in the partial strip of rows 128-149 / t list K - 1 in row 63, K in row 64


def group_b(base):
    rng = np.random.default_rng(7)
    return [_member(rng, base, e, g) for e, g in ((0, 0), (50, 2), (50, 3), (100, 4))]


class Case:
    """One DP: its PwdM, the lengths its lists must have, and (once) the oracle's result."""
    _oracle = {}

    def __init__(self, ls, K, c0, related=False, plain=2):
        self.key = (ls, K, c0, related, plain)
        self.top = K + (1 if plain else 0)          # entries of the longest s and r lists
        self.noll = 3 if ls == 3 else 2
        self.K, self.c0 = K, c0
        alp = op.AlnParam(ls=ls)
        base_a = _base(5, LEN_A)
        # (related: b is a's own base sequence without its first five columns, so the best path runs down the rows of the long lists)
        base_b = base_a[5:5 + LEN_B] if related else _base(9, LEN_B)
        self.pw = op.PwdM([op.mSeq(group_a(K, c0, base_a, plain), alp), op.mSeq(group_b(base_b), alp)], alp)
        self.on_v6 = self.top + 1 <= SLOTS[self.noll]

    def check_lists(self):
        P, K, c0, top = self.pw.problem, self.K, self.c0, self.top
        assert self.pw.alnmode == 9 and not self.pw.swp and P.noll == self.noll and (P.a.left, P.a.right) == (0, LEN_A)
        s, t, r = list_lengths(P.a)
        want_t = np.zeros(LEN_A, int)
        want_t[c0 - K:c0] = np.arange(1, K + 1)
        assert np.array_equal(t[1:], want_t), t
        assert s[1 + c0] == top and s.max() == top and (np.delete(s, 1 + c0) <= 1).all(), s
        assert r[c0] == top and r.max() == top
        assert int(max(x.max() for x in (s, t, r))) + 1 == top + 1                    # DevSide::maxlist counts the terminator
        strip = (c0 - 1) // 64
        longest = [int(t[1 + 64 * i:1 + 64 * (i + 1)].max()) for i in range(3)]       # per strip: what the X merges are sized by
        assert longest[strip] == K and all(x <= max(1, K - 1) for i, x in enumerate(longest) if i != strip), longest
        if c0 == ACROSS and K > 1:
            assert longest[0] == K - 1 and longest[1] == K

    def oracle(self, L):
        if self.key not in Case._oracle:
            class H:
                c = self.pw.problem
            scr, _, tr = oraclelib.forward(L, H)
            Case._oracle[self.key] = (scr, oraclelib.stdskl(L, tr))
        return Case._oracle[self.key]


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def L():
    return oraclelib.load()


@pytest.fixture(autouse=True)
def _v6_whatever_the_batch_size(ctx):
    ctx.reset_options()
    ctx.set_option("G2G_V6_MIN_STRIPS", "0")
    yield
    ctx.reset_options()


def run_and_check(ctx, L, cases, distinct=None):
    """One launch of `cases`; every DP on v6 (or, where its lists do not fit the slots, not on v6) and equal to the oracle.
    distinct: the case whose content cases[i] repeats (the oracle runs once per content)."""
    class H:
        def __init__(self, pw):
            self.c = pw.problem
    batch = ctx.prepare([H(c.pw) for c in cases])
    try:
        chosen = batch.paths()
        batch.run()
        res = batch.fetch()
        ran = batch.paths()
    finally:
        batch.free()
    for i, (c, (scr, cells, tr, st)) in enumerate(zip(cases, res)):
        assert (chosen[i] == 6) == c.on_v6 and (ran[i] == 6) == c.on_v6, (c.key, chosen[i], ran[i])
        oscr, oskl = (distinct[i] if distinct else c).oracle(L)
        assert st == 0, (c.key, st)
        assert scr == oscr, (c.key, scr, oscr)
        assert np.array_equal(engine.stdskl(tr), oskl), c.key


EDGES = [(1, K) for K in (1, 4, 5, 8, 9, 12, 13, 14, 15)] + [(3, K) for K in (1, 4, 5, 8, 9)]


@pytest.mark.parametrize("ls,K", EDGES, ids=["noll%d_K%d" % (3 if ls == 3 else 2, K) for ls, K in EDGES])
def test_bucket_edges_first_strip(ctx, L, ls, K):
    """K on both sides of every bucket edge, the long lists in the first strip (row 59: lane 59 of 64)."""
    c = Case(ls, K, FIRST)
    c.check_lists()
    run_and_check(ctx, L, [c])


PLACED = [(1, 4), (1, 9), (1, 13), (3, 4), (3, 5)]


@pytest.mark.parametrize("c0", [LAST, ACROSS], ids=["last_partial_strip", "across_rows_63_64"])
@pytest.mark.parametrize("ls,K", PLACED, ids=["noll%d_K%d" % (3 if ls == 3 else 2, K) for ls, K in PLACED])
def test_bucket_edges_other_strips(ctx, L, ls, K, c0):
    """The long lists in the last strip (rows 128-149: 22 active lanes) and on both sides of the boundary between strips 0 and 1
    (strip 0 runs with K - 1, strip 1 with K)."""
    c = Case(ls, K, c0)
    c.check_lists()
    run_and_check(ctx, L, [c])


@pytest.mark.parametrize("ls,Ks", [(1, (13, 1, 9, 4, 14, 5, 8, 12)), (3, (8, 1, 5, 4))], ids=["noll2", "noll3"])
def test_mixed_lengths_in_one_launch(ctx, L, ls, Ks):
    """Several K in one launch at one strip per CU: with more strips than workgroups a workgroup pops strips of different DPs one
    after the other, and the longest t list changes between its queue entries."""
    ctx.set_option("G2G_V6_WPC", "1")
    placed = (FIRST, LAST, ACROSS)
    first = [Case(ls, K, placed[i % 3]) for i, K in enumerate(Ks)]
    for c in first:
        c.check_lists()
    reps = 384 // (3 * len(Ks)) + 1                                            # 3 strips per DP: beyond 384 strips in all
    cases, distinct = [], []
    for rep in range(reps):
        for c in first:
            cases.append(c if rep == 0 else Case(*c.key))                       # (a PwdM of its own per DP)
            distinct.append(c)
    run_and_check(ctx, L, cases, distinct)


@pytest.mark.parametrize("ls,K", [(1, 13), (1, 5), (3, 8)], ids=["noll2_K13", "noll2_K5", "noll3_K8"])
def test_related_groups(ctx, L, ls, K):
    """b derived from a's base sequence: the optimal path runs through the rows of the long lists instead of along the band edge."""
    c = Case(ls, K, FIRST, related=True)
    c.check_lists()
    _, oskl = c.oracle(L)
    # one diagonal run of the skeleton spans the rows of the long lists, five columns off the main diagonal (the band is far wider)
    assert any(m2 - m1 == n2 - n1 and m1 <= FIRST - K - 1 and m2 > FIRST and m1 - n1 == 5 for (m1, n1), (m2, n2) in zip(oskl[:-1], oskl[1:])), oskl
    run_and_check(ctx, L, [c])


FULL = [(1, 15), (1, 13), (1, 12), (3, 9), (3, 8)]


@pytest.mark.parametrize("ls,K", FULL, ids=["noll%d_K%d" % (3 if ls == 3 else 2, K) for ls, K in FULL])
def test_longest_t_lists_v6_takes(ctx, L, ls, K):
    """Every member of a gapped (no plain member): the s list of row c0 has K entries like the t list of row c0 - 1, so v6 takes
    K = 15 (K = 9 with Noll 3) -- the longest t list it can meet, in the last bucket of each kernel."""
    c = Case(ls, K, FIRST, plain=0)
    c.check_lists()
    assert c.on_v6
    run_and_check(ctx, L, [c])
