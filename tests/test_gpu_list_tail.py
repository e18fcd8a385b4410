"""The list loops of the v6 `_pf` cell end at the wave's last live entry: the Y merges and the b-side newdelta decide a list's
end in front of the wave's exit test (g2g_kernels_v6.hip), so the iteration behind the wave's longest list -- which changed
no state -- is not run.  These cases put the lists' ends where a loop that leaves one entry early, or one late, or on the wrong
lane's length, would give another score or another path.  The v3r `_hf` cell has loops of the same shape over the row lists;
ending them on the strip's longest lists was built and measured slower, so its loops are unchanged -- the cases
that pin where its lists end are kept for the next attempt.

Every problem is built by hand with tests/widelib.py.  Expected values: the CPU oracle (score equal as a double, equal
skeleton, status 0); g2g_batch_paths says which kernel ran.  test_lists_are_what_the_cases_claim runs without a GPU and pins
the list lengths of every problem, so the edges are known to be hit.

v6 (`_pf`, 150 x 140, three strips of 64, 64 and 22 rows; the column side b is what the two loops walk):
  same1 .. same3   every column of b has a t list of L entries (and an r list of L + 1): the dead iteration was the last one of
                   every step.  L + 1 sparse members hold a residue every (L + 1)-th column, each at its own offset, so that at
                   any column the L others are inside runs of L different lengths.  The first L - 1 columns have fewer entries:
                   every run that is open at column 0 has length 1 there.
  long             t lists of 6 and of 9 entries (columns 39 and 99) among columns without a t entry.  A run is one entry longer at
                   every column, so a list of K entries stands at the top of a staircase of 1 .. K - 1; no column outside the two
                   staircases has a t entry.  Dynamic lists of up to 7 and 10 entries: the eight-entry heads, the scanning
                   instance, and newdelta results beyond the inline part.
  heads            no column of b with a t list but seven: lenr 1, lent 0 nearly everywhere -- a wave whose active lanes all stand
                   on such columns runs the Y loop exactly once.
  heads_noend      the same with terminal gaps that cost nothing (tgapf 0): the last column of b has no r head either
                   (lenr 0, lent 0).  The last step of a strip has one active lane, on that column: the Y loop does not run.
  edge             staircases of 6 at columns 1 .. 6 and 133 .. 138.  The band (lw -94, up 84) cuts the corners of the rectangle:
                   columns 133 .. 138 are live in strip 0 only in lanes 49 .. 63, in its ramp-down steps, and columns 1 .. 6 in
                   strip 1 only in lanes 0 .. 36, in its ramp-up steps.

v3r (`_hf`: a group of 150 columns against one sequence of 140; the row side a is what the loops walk):
  K = 1 (six plain members: a smaller group is not aligned in the `_hf` mode), 8 (two plain members) and 15 (no plain member: the s list of row c0 has K entries, not K + 1, and a list of 15 entries
  with its terminator fills the 16 register slots -- the loops end at i == N there); the staircase in strip 0 (c0 60), in the
  partial last strip (c0 140) and across rows 63 | 64 (c0 65: t list K - 1 in row 63, K in row 64); a group of 129 columns whose
  last strip is the one row that holds the longest lists.  With c0 65 the strips' longest s / t / r lists differ: (1, K - 1, K)
  in strip 0 and (K + 1, K, K + 1) in strip 1 with the r head; without a plain member the row of the longest r list has no head
  and r is as long as t (an r list is the t list with or without one head entry: three different lengths need the head)."""
import numpy as np
import pytest

import oraclelib
from prrn_aln_amd import engine, operator as op
from widelib import base as _base, list_lengths, member as _member, stair as _stair

LEN_A, LEN_B = 150, 140
V3, V6 = 3, 6                                   # g2g_batch_paths
V3R_SLOTS = 16                                  # G2G_V3_NA, terminator included
V6_SLOTS = {2: 16, 3: 10}                       # G2G_V6_NA / G2G_V6_NA3
FIRST, LAST, ACROSS = 60, 140, 65
SPEC_A = ((0, 0), (50, 2), (50, 3), (100, 4), (0, 0), (0, 0), (30, 1), (0, 0))


def few_gaps(base, members):
    """`members` rows, the first eight with the runs of SPEC_A (end, length), the rest without a gap"""
    rng = np.random.default_rng(7)
    return [_member(rng, base, *(SPEC_A[i] if i < len(SPEC_A) else (0, 0))) for i in range(members)]


def same_length(base, L):
    """two plain members and L + 1 sparse ones: member j holds a residue at the columns c with c % (L + 1) == j"""
    rng = np.random.default_rng(21)
    rows = [_member(rng, base) for _ in range(2)]
    for j in range(L + 1):
        r = _member(rng, base)
        rows.append("".join(ch if c % (L + 1) == j else "-" for c, ch in enumerate(r)))
    return rows


def staircases(base, steps):
    """one plain member and, per (K, c0) of `steps`, K members with runs of 1 .. K columns that end just before column c0"""
    rng = np.random.default_rng(3)
    return [_member(rng, base)] + [_member(rng, base, c0, g) for K, c0 in steps for g in range(1, K + 1)]


LONG = ((6, 40), (9, 100))
EDGE = ((6, 7), (6, LEN_B - 1))


class Case:
    """One DP: its PwdM, what its lists must look like, and (once) the oracle's result."""
    _oracle = {}

    def __init__(self, name, ls):
        self.key = (name, ls)
        self.name, self.noll = name, 3 if ls == 3 else 2
        tgapf = 0.0 if name == "heads_noend" else 1.0
        alp = op.AlnParam(ls=ls, tgapf=tgapf)
        kind, _, arg = name.partition(":")
        if kind == "hf":                                        # hf:K,c0,plain,len_a
            self.K, self.c0, self.plain, self.len_a = (int(x) for x in arg.split(","))
            rows_a = _stair(self.K, self.c0, _base(5, LEN_A)[:self.len_a], self.plain)
            rows_b = [_member(np.random.default_rng(7), _base(9, LEN_B))]
            self.want = V3
        else:
            self.len_a = LEN_A
            rows_a = few_gaps(_base(5, LEN_A), 18)
            bb = _base(9, LEN_B)
            rows_b = (same_length(bb, int(name[4:])) if name.startswith("same") else staircases(bb, LONG) if name == "long"
                      else staircases(bb, EDGE) if name == "edge" else few_gaps(bb, 4))
            self.want = V6
        self.pw = op.PwdM([op.mSeq(rows_a, alp), op.mSeq(rows_b, alp)], alp)

    def check_lists(self):
        P = self.pw.problem
        assert not self.pw.swp and P.noll == self.noll and (P.a.left, P.a.right, P.b.left, P.b.right) == (0, self.len_a, 0, LEN_B)
        sa, ta, ra = list_lengths(P.a)                          # [row + 1]
        longest_a = int(max(x.max() for x in (sa, ta, ra))) + 1  # DevSide::maxlist counts the terminator
        if self.want == V3:
            self.check_hf(P, sa[1:], ta[1:], ra[1:], longest_a)
            return
        assert self.pw.alnmode == 9 and longest_a <= V6_SLOTS[self.noll]
        assert (P.lw, P.up) == (-94, 84)
        s, t, r = (x[1:] for x in list_lengths(P.b))            # [column]
        cols = np.arange(LEN_B)
        name = self.name
        if name.startswith("same"):
            L = int(name[4:])
            assert np.array_equal(t, np.minimum(cols + 1, L)), t
            assert np.array_equal(r, t + 1)
        elif name in ("long", "edge"):
            want = np.zeros(LEN_B, int)
            for K, c0 in (LONG if name == "long" else EDGE):
                want[c0 - K:c0] = np.arange(1, K + 1)
            assert np.array_equal(t, want), t
            assert np.array_equal(r, t + 1)                     # (the plain member: an r head in every column)
            if name == "long":
                assert t[39] == 6 and t[99] == 9 and t.max() == 9
            else:
                live = lambda c, m: P.lw <= c - m <= P.up
                for c in range(133, 139):                       # strip 0 meets them in its last lanes only
                    assert [m for m in range(0, 64) if live(c, m)] == list(range(c - 84, 64)) and c - 84 >= 49
                for c in range(1, 7):                           # strip 1 in its first lanes only
                    assert [m for m in range(64, 128) if live(c, m)] == list(range(64, c + 95)) and c + 94 <= 100
        else:
            assert t.max() == 2 and np.count_nonzero(t) == 7 and np.array_equal(np.flatnonzero(t), [47, 48, 49, 96, 97, 98, 99])
            if name == "heads":
                assert np.array_equal(r, t + 1)                 # lenr 1, lent 0 in 133 columns
            else:
                assert np.array_equal(r[:-1], t[:-1] + 1) and r[-1] == 0 and t[-1] == 0          # the last column: neither

    def check_hf(self, P, s, t, r, longest_a):
        K, c0, top = self.K, self.c0, self.K + (1 if self.plain else 0)
        assert self.pw.alnmode == 7 and P.b.many == 1 and longest_a <= V3R_SLOTS
        want_t = np.zeros(self.len_a, int)
        want_t[c0 - K:c0] = np.arange(1, K + 1)
        assert np.array_equal(t, want_t), t
        assert r[c0 - 1] == top and r.max() == top
        if c0 < self.len_a:
            assert s[c0] == top and s.max() == top
        if K == 15:
            assert longest_a == V3R_SLOTS                       # 15 entries and the terminator: every register slot taken
        per_strip = [tuple(int(x[64 * i:64 * (i + 1)].max()) for x in (s, t, r)) for i in range((self.len_a + 63) // 64)]
        if self.len_a == 129:
            assert c0 == 129 and per_strip[2] == (1, K, K + 1) and (t[128], r[128]) == (K, K + 1)      # a last strip of one row
        elif c0 == FIRST:
            assert per_strip[0][1:] == (K, top) and per_strip[1][1] == 0
        elif c0 == LAST:
            assert per_strip[2][1:] == (K, top) and per_strip[0][1] == per_strip[1][1] == 0
        elif self.plain:                                        # ACROSS, with the r head: three different lengths in both strips
            assert per_strip[0] == (1, K - 1, K) and per_strip[1] == (K + 1, K, K + 1), per_strip
        else:                                                   # ACROSS, the rows of the long lists have no r head
            assert per_strip[0] == (1, K - 1, K) and per_strip[1] == (K, K, K), per_strip
            assert r[c0 - 1] == t[c0 - 1] == K

    def oracle(self, L):
        if self.key not in Case._oracle:
            class H:
                c = self.pw.problem
            scr, _, tr = oraclelib.forward(L, H)
            Case._oracle[self.key] = (scr, oraclelib.stdskl(L, tr))
        return Case._oracle[self.key]


V6_NAMES = ["same1", "same2", "same3", "long", "heads", "heads_noend", "edge"]
HF_NAMES = ["hf:%d,%d,%d,%d" % x for x in ((1, FIRST, 6, LEN_A), (8, FIRST, 2, LEN_A), (15, FIRST, 0, LEN_A), (8, LAST, 2, LEN_A),
                                          (8, ACROSS, 2, LEN_A), (15, ACROSS, 0, LEN_A), (8, 129, 2, 129))]
ALL = [(n, ls) for n in V6_NAMES + HF_NAMES for ls in (1, 3)]


def _id(name, ls):
    return "%s-noll%d" % (name.replace(":", "_").replace(",", "_"), 3 if ls == 3 else 2)


def test_lists_are_what_the_cases_claim():
    """every problem of this file has the list lengths its case is named for (no GPU: the groups are built on the host)"""
    for name, ls in ALL:
        Case(name, ls).check_lists()


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    c.reset_options()
    c.set_option("G2G_V6_MIN_STRIPS", "0")      # small _pf DPs run on v6
    yield c
    c.reset_options()
    c.close()


@pytest.fixture(scope="module")
def L():
    return oraclelib.load()


@pytest.mark.gpu
@pytest.mark.parametrize("name,ls", ALL, ids=[_id(n, ls) for n, ls in ALL])
def test_list_tail(ctx, L, name, ls):
    c = Case(name, ls)
    c.check_lists()

    class H:
        pass
    H.c = c.pw.problem
    batch = ctx.prepare([H])
    try:
        chosen = batch.paths()
        batch.run()
        (scr, cells, tr, st), = batch.fetch()
        ran = batch.paths()
    finally:
        batch.free()
    assert chosen[0] == c.want and ran[0] == c.want, (c.key, chosen, ran)
    oscr, oskl = c.oracle(L)
    assert st == 0, (c.key, st)
    assert scr == oscr, (c.key, scr, oscr)
    assert np.array_equal(engine.stdskl(tr), oskl), c.key
