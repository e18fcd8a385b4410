"""The rings of b's static lists in the v6 `_pf` strips (g2g_kernels_v6.hip) have the size the lists need, rounded up to 32
entries -- not a power of two -- and a mirrored tail behind them; a list's start is reduced to a slot once per cell with a
wave-uniform base and one conditional subtract.  These cases make the rings wrap several times, put lists across the ring's
end (they are read through the tail), and mix ring-hungry and sparse DPs under one launch-wide plan.

Inputs: two gap-rich groups, one base sequence each, every member but the first with random gap runs of at most 8 columns:
a 12 members x 190 columns (8 runs per member), b 12 members x 360 columns (16 runs per member).  On the host that gives
alnmode 9, not swapped, 190 rows = two full strips and one of 62 rows (with lw = -114 the third starts on column 14: a ring
base of its own), lists of at most 6 entries in a; b needs 133 s entries and 187 t entries in a window of 88 columns:
rings of 160 and 192 entries, over pools of 505 and 609 -- each ring wraps three times.  Each test asserts what it got from the
problem's own offset tables and from the plan the engine recorded (option V6_RING_PLAN) before it runs.

With Noll 3 (ls = 3) a row of dynamic lists has nine record slots instead of six, and v6 takes a DP only while its plan fits
40 KB: that holds when one side's dynamic lists have a capacity of four dwords (hetero <= 3), so with ls = 3 only two members
of a carry gap runs (hetero 3).  b, whose lists the rings hold, is the same in both.

Expected values: the CPU oracle (score equal as a double, equal skeleton, status 0); every DP on v6."""
import os
import re

import numpy as np
import pytest

import oraclelib
from prrn_aln_amd import engine, operator as op
from test_gpu_v6_xmerge_bounds import Case as SparseCase
from widelib import base as _base, list_lengths

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HDR = open(os.path.join(ROOT, "prrn_aln_amd", "csrc", "g2g_lds.h")).read()
V6_AHEAD = int(re.search(r"#define V6_AHEAD (\d+)", _HDR).group(1))
V6_WINDOW = 64 + V6_AHEAD + 4
LEN_A, LEN_B, MANY = 190, 360, 12


def gapped_group(seed, many, n, runs, maxrun=8, stairs=0, gapped=None):
    """one base sequence; every member but the first (`gapped`: only members 1 .. gapped) carries `runs` random gap runs of
    1 .. maxrun columns; members 1 .. stairs also end with a gap run of their index's length (lists of `stairs` entries and more
    in the last column)"""
    rng = np.random.default_rng(seed)
    b = _base(seed, n)
    out = [b]
    for j in range(1, many):
        r = list(b)
        for _ in range(runs if gapped is None or j <= gapped else 0):
            ln = int(rng.integers(1, maxrun + 1))
            s = int(rng.integers(1, n - ln - 1))
            r[s:s + ln] = "-" * ln
        if j <= stairs:
            r[n - j:] = "-" * j
        out.append("".join(r))
    return out


def ring_facts(P):
    """per view (s, t) of b: need over V6_WINDOW columns, ring size, pool entries, compact start and length of every column's list"""
    b = P.b
    lo, hi = b.left, b.right
    out = []
    for v in range(2):
        off = np.ctypeslib.as_array(b.gfq.off[v], shape=(b.len + 2,)).astype(np.int64)
        comp = off - np.arange(b.len + 2)                        # comp[c + 1]: entries in front of column c's list
        c = np.arange(lo, hi)
        need = int(max(1, (comp[np.minimum(c + V6_WINDOW, hi) + 1] - comp[c + 1]).max()))
        out.append(dict(need=need, S=max(32, (need + 31) & ~31), pool=int(comp[hi + 1] - comp[lo + 1]),
                        start=comp[lo + 1:hi + 1] - comp[lo + 1], length=np.diff(off)[lo + 1:hi + 1] - 1))
    return out


def ring_plan(ctx):
    """option V6_RING_PLAN: {launch index: (S of the s ring, S of the t ring, T, LDS bytes)}"""
    txt = ctx.get_option("V6_RING_PLAN")
    assert txt, txt
    return {int(k): tuple(int(x) for x in v.split(",")) for k, v in (e.split(":") for e in txt.split(";"))}


class RingCase:
    """One DP of the two gap-rich groups, and (once per content) the oracle's result."""
    _oracle = {}

    def __init__(self, ls, len_b=LEN_B, stairs=0):
        self.key = ("ring", ls, len_b, stairs)
        self.noll = 3 if ls == 3 else 2
        alp = op.AlnParam(ls=ls)
        a = gapped_group(11, MANY, LEN_A, 8, gapped=2 if ls == 3 else None)
        b = [m[:len_b] for m in gapped_group(23, MANY, LEN_B, 16)] if not stairs else gapped_group(23, MANY, len_b, 16, stairs=stairs)
        self.pw = op.PwdM([op.mSeq(a, alp), op.mSeq(b, alp)], alp)
        self.on_v6 = True

    def check_shape(self, len_b=LEN_B):
        P = self.pw.problem
        assert self.pw.alnmode == 9 and not self.pw.swp and P.noll == self.noll
        assert (P.a.left, P.a.right, P.b.left, P.b.right) == (0, LEN_A, 0, len_b)
        assert int(max(x.max() for x in list_lengths(P.a))) + 1 <= 10          # a's lists fit the register slots of both kernels

    def oracle(self, L):
        if self.key not in RingCase._oracle:
            class H:
                c = self.pw.problem
            scr, _, tr = oraclelib.forward(L, H)
            RingCase._oracle[self.key] = (scr, oraclelib.stdskl(L, tr))
        return RingCase._oracle[self.key]


def check_wraps(P, plan):
    """what makes the case a test of the ring: the launch's S (at least this DP's) is no power of two in some view, the pools
    hold three rings and more, and some list lies across the ring's end -- its entries are read through the mirrored tail"""
    S_plan, T = plan[:2], plan[2]
    facts = ring_facts(P)
    longest = int(max(x[P.b.left + 1:P.b.right + 1].max() for x in list_lengths(P.b)))       # over the three views: what DevSide::maxlist - 1 is
    assert T % 4 == 0 and T >= ((longest + 1 + 3) & ~3), (T, longest)
    assert any(S & (S - 1) for S in S_plan), S_plan
    across = 0
    for f, S in zip(facts, S_plan):
        assert S % 32 == 0 and S >= f["S"] >= f["need"], (S, f["S"], f["need"])
        assert f["pool"] >= 3 * S, (f["pool"], S)
        near_end = 0
        for m0 in range(P.a.left, P.a.right, 64):                # slot 0 of a strip's ring is the list start of its first column
            cb = max(m0 + P.lw, P.b.left) - P.b.left
            slot = (f["start"][cb:] - f["start"][cb]) % S
            near_end += int(((slot >= S - longest) & (f["length"][cb:] > 0)).sum())       # lists that start within the last maxlist - 1 slots
            across += int((slot + f["length"][cb:] > S).sum())
        assert near_end, (S, longest)
    assert across >= 2, across
    return facts


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


def run_and_check(ctx, L, cases, distinct=None, before_run=None):
    class H:
        def __init__(self, pw):
            self.c = pw.problem
    batch = ctx.prepare([H(c.pw) for c in cases])
    try:
        chosen = batch.paths()
        assert all(g == 6 for g in chosen), chosen
        if before_run:
            before_run(ring_plan(ctx))
        batch.run()
        res = batch.fetch()
        ran = batch.paths()
    finally:
        batch.free()
    for i, (c, (scr, cells, tr, st)) in enumerate(zip(cases, res)):
        assert ran[i] == 6, (c.key, ran[i])
        oscr, oskl = (distinct[i] if distinct else c).oracle(L)
        assert st == 0, (c.key, st)
        assert scr == oscr, (c.key, scr, oscr)
        assert np.array_equal(engine.stdskl(tr), oskl), c.key


def one_launch(plan, noll):
    assert list(plan) == [noll - 2], plan                        # one v6 launch: footprint class A of this Noll
    return plan[noll - 2]


@pytest.mark.parametrize("ls", [1, 3], ids=["noll2", "noll3"])
def test_ring_wraps_alone(ctx, L, ls):
    """(a) the DP alone: the launch's rings are exactly this DP's (160 and 192 entries)."""
    c = RingCase(ls)
    c.check_shape()

    def before(plan):
        p = one_launch(plan, c.noll)
        facts = check_wraps(c.pw.problem, p)
        assert p[:2] == (facts[0]["S"], facts[1]["S"]) == (160, 192), p
        assert p[3] <= 40960

    run_and_check(ctx, L, [c], before_run=before)


@pytest.mark.parametrize("ls", [1, 3], ids=["noll2", "noll3"])
def test_ring_beside_sparse_dps(ctx, L, ls):
    """(b) 44 of it and 44 sparse DPs (a's lists long, b's next to none) interleaved in one launch at one strip per CU: 264 strips
    for 256 workgroups, so a workgroup pops strips of different list densities one after the other under one launch-wide S / T."""
    ctx.set_option("G2G_V6_WPC", "1")
    ring0, sparse0 = RingCase(ls), SparseCase(ls, 5, 60)
    ring0.check_shape()
    sparse0.check_lists()
    assert sparse0.on_v6
    cases, distinct = [], []
    for rep in range(44):
        cases += [ring0 if rep == 0 else RingCase(ls), sparse0 if rep == 0 else SparseCase(*sparse0.key)]
        distinct += [ring0, sparse0]

    def before(plan):
        p = one_launch(plan, ring0.noll)
        check_wraps(ring0.pw.problem, p)
        sp = ring_facts(sparse0.pw.problem)
        assert all(f["S"] < S for f, S in zip(sp, p[:2])), (sp[0]["S"], sp[1]["S"], p)       # the sparse DPs run under rings far beyond their own

    run_and_check(ctx, L, cases, distinct, before_run=before)


@pytest.mark.parametrize("ls", [1, 3], ids=["noll2", "noll3"])
def test_b_shorter_than_the_window(ctx, L, ls):
    """(c) b cut to its first 70 columns: the first refill takes all of b, the ring never wraps."""
    c = RingCase(ls, len_b=70)
    c.check_shape(70)
    assert 70 < V6_WINDOW

    def before(plan):
        p = one_launch(plan, c.noll)
        facts = ring_facts(c.pw.problem)
        assert all(f["pool"] == f["need"] <= S for f, S in zip(facts, p[:2])), p

    run_and_check(ctx, L, [c], before_run=before)


@pytest.mark.parametrize("ls", [1, 3], ids=["noll2", "noll3"])
def test_longest_list_in_the_last_column(ctx, L, ls):
    """(d) nine members of b end with gap runs of 1 .. 9 columns: the longest lists of b (t 9, r 10 entries) sit in its very last
    column, whose reads past the list's end have nothing behind them but the ring's own slots and tail."""
    c = RingCase(ls, stairs=9)
    c.check_shape()
    s, t, r = list_lengths(c.pw.problem.b)
    assert t[-1] == t.max() == 9 and r[-1] == r.max() == 10 and s.max() < 9, (s.max(), t[-1], r[-1])

    def before(plan):
        p = one_launch(plan, c.noll)
        check_wraps(c.pw.problem, p)
        assert p[2] >= 11                                        # the tail covers the r view's ten entries and one more

    run_and_check(ctx, L, [c], before_run=before)
