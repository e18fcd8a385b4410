"""The v6 `_pf` cell takes the nins of a diagonal H's a-side list update from the stretched keys its d1 X merge has already
looked up, and runs the d1 / gnph / goph merges of the 4- and 8-slot buckets in one loop over the ring, gnph / goph of the
12-slot bucket in one (v6_cell_pf, v6_xmerge3, g2g_kernels_v6.hip).  Both are regroupings of the same integer lookups and the
same f64 sums: results must not move by a bit.

Inputs are the staircase groups of tests/widelib.py on a 150 x 140 DP: group a has two plain members and K members with one gap
run of 1 .. K columns that ends just before column c0, so row c0 - 1 carries a t list of K entries and the strip that holds it
sizes its X merges by K.  K = 1, 4 (fused bucket of 4), 5, 8 (fused bucket of 8), 9 and 12 (the bucket whose d1 merge keeps
its own loop) with Noll 2, K = 4, 5 and 8 with Noll 3 (the fourth merge stays a call of its own), K = 9 with Noll 3 from a group
without a plain member; the long rows in the first strip, in the last, partial
strip and across the boundary of strips 0 and 1.  related: b is a's own base sequence five columns in, the diagonal wins along
the rows of the long lists and the a-side update of H (the reused values) is live there; unrelated: it is off in most lanes.
Expected values: the CPU oracle (score equal as a double, equal skeleton, status 0), every DP on v6.

The cell's eight-entry and scanning instances and its long-store path need dynamic lists of more than five and eight entries.
None of the tests/golden/wide fixtures reaches them: every one of those runs on v1, v2 or v3 by default (their row lists are
beyond v6's register slots; DEFAULT_PATH of tests/test_gpu_wide.py), and no fixture records dynamic-list lengths.  Those
instances are held to the oracle by tests/test_gpu_fullsize.py::test_progressive_start_divisions_vs_oracle."""
import numpy as np
import pytest

import oraclelib
from prrn_aln_amd import engine, operator as op
from widelib import base as _base, list_lengths, member as _member, stair as group_a

pytestmark = pytest.mark.gpu

LEN_A, LEN_B = 150, 140
FIRST, LAST, ACROSS = 60, 140, 65               # c0: long lists in strip 0 / in the partial strip of rows 128-149 / t list K - 1 in row 63, K in row 64
KS = {2: (1, 4, 5, 8, 9, 12), 3: (4, 5, 8)}     # Noll -> K: the buckets of 4, 8 and 12 slots, every edge between them
LS = {2: 1, 3: 3}                               # Noll -> AlnParam.ls
V6 = 6                                          # g2g_batch_paths


def group_b(base):
    rng = np.random.default_rng(7)
    return [_member(rng, base, e, g) for e, g in ((0, 0), (50, 2), (50, 3), (100, 4))]


class Case:
    """One DP: its PwdM, the lengths its lists must have, and the oracle's result."""

    def __init__(self, noll, K, c0, related, plain=2):
        self.key = (noll, K, c0, related, plain)
        self.noll, self.K, self.c0, self.related = noll, K, c0, related
        self.top = K + (1 if plain else 0)          # entries of the longest s and r lists
        alp = op.AlnParam(ls=LS[noll])
        base_a = _base(5, LEN_A)
        base_b = base_a[5:5 + LEN_B] if related else _base(9, LEN_B)
        self.pw = op.PwdM([op.mSeq(group_a(K, c0, base_a, plain), alp), op.mSeq(group_b(base_b), alp)], alp)

    def check_lists(self):
        P, K, c0 = self.pw.problem, self.K, self.c0
        assert self.pw.alnmode == 9 and not self.pw.swp and P.noll == self.noll and (P.a.left, P.a.right) == (0, LEN_A)
        s, t, r = list_lengths(P.a)
        want_t = np.zeros(LEN_A, int)
        want_t[c0 - K:c0] = np.arange(1, K + 1)
        assert np.array_equal(t[1:], want_t), t
        assert s.max() == self.top and r.max() == self.top
        strip = (c0 - 1) // 64
        longest = [int(t[1 + 64 * i:1 + 64 * (i + 1)].max()) for i in range(3)]       # per strip: what the X merges are sized by
        assert longest[strip] == K and all(x <= max(1, K - 1) for i, x in enumerate(longest) if i != strip), longest
        if c0 == ACROSS and K > 1:
            assert longest[0] == K - 1 and longest[1] == K

    def oracle(self, L):
        class H:
            c = self.pw.problem
        scr, _, tr = oraclelib.forward(L, H)
        return scr, oraclelib.stdskl(L, tr)


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


def diagonal_through_long_rows(skl, K, c0):
    """one diagonal run of the skeleton spans rows c0 - K .. c0 - 1, five columns off the main diagonal"""
    return any(m2 - m1 == n2 - n1 and m1 <= c0 - K - 1 and m2 >= c0 and m1 - n1 == 5 for (m1, n1), (m2, n2) in zip(skl[:-1], skl[1:]))


def run_and_check(ctx, L, cases, related):
    want = []
    for c in cases:
        c.check_lists()
        want.append(c.oracle(L))
        if related:
            assert diagonal_through_long_rows(want[-1][1], c.K, c.c0), (c.key, want[-1][1])

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
    for i, (c, (oscr, oskl), (scr, cells, tr, st)) in enumerate(zip(cases, want, res)):
        assert chosen[i] == V6 and ran[i] == V6, (c.key, chosen[i], ran[i])
        assert st == 0, (c.key, st)
        assert scr == oscr, (c.key, scr, oscr)
        assert np.array_equal(engine.stdskl(tr), oskl), c.key


@pytest.mark.parametrize("related", [True, False], ids=["related", "unrelated"])
@pytest.mark.parametrize("noll", [2, 3], ids=["noll2", "noll3"])
def test_reused_lookups_and_fused_merges(ctx, L, noll, related):
    """Every K at every placement in one launch: on v6, equal to the oracle."""
    run_and_check(ctx, L, [Case(noll, K, c0, related) for K in KS[noll] for c0 in (FIRST, LAST, ACROSS)], related)


@pytest.mark.parametrize("related", [True, False], ids=["related", "unrelated"])
def test_noll3_bucket_beyond_eight(ctx, L, related):
    """Noll 3 holds ten slots: a t list of nine entries reaches v6 only from a group without a plain member (its longest s list
    then has nine entries as well).  Its bucket runs gnph and goph in one loop over ten slots and gnph2 in a call of its own."""
    run_and_check(ctx, L, [Case(3, 9, c0, related, plain=0) for c0 in (FIRST, LAST, ACROSS)], related)
