"""Group fusing on the GPU (g2g_mayfuse_kernel in csrc/g2g_consreg.hip: one workgroup per test, tiles of 256 columns, one lane walks):
g2g_mayfuse_batch on pairs the DEVICE builders built against the REFERENCE's outcomes (tests/golden/fuse) and the restatement's stop
columns (tests/fuselib.py), g2g_consregss / g2g_consreg_groups / g2g_refine_plan against the recorded subsets, trees and ranges, and
the edges of the tiling and of the recurrence on hand-made pairs whose column scores are entries of a small integer matrix, so that
every sum is exact.  No tolerance anywhere: outcomes, columns, subsets and tree indices are integers, vol / cur are copies."""
import numpy as np
import pytest

import consreglib as cl
import fuselib as fl
from prrn_aln_amd import engine, guide, operator as op
from prrn_aln_amd.synth import make_family

pytestmark = pytest.mark.gpu
FIX = fl.fixtures()
IDS = [n for n, _ in FIX]
T = 256                                         # CR_T of csrc/g2g_consreg.hip: columns per tile
bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.int64)


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


def weight_of(g):
    return g["weight"] if len(g["weight"]) else None


class Tree:
    def __init__(self, arrs):
        self.left, self.right, self.parent, self.vol, self.cur = arrs


def device_pairs(ctx, codes, lists, alp, weight=None):
    pairs = []
    for l0, l1 in lists:
        sons = []
        for lst in (l0, l1):
            w = None if weight is None else ([1.0] if len(lst) == 1 else [float(weight[m]) for m in lst])
            sons.append(op.mSeq(np.ascontiguousarray(codes[:, list(lst)]), alp, w))
        pairs.append(sons)
    return op.PwdM.batch(ctx, pairs, alp)


def restated(codes, lists, alp, weight=None):
    """[(fuse, stop_col, alnmode)] of the restatement on host-built pairs"""
    return [fl.may_fuse(codes, l0, l1, alp, weight) for l0, l1 in lists]


def same_relation(rel, groups, tree, given_vol_cur=None):
    assert [g.tolist() for g in rel.groups] == groups
    assert np.array_equal(rel.left, tree[0]) and np.array_equal(rel.right, tree[1]) and np.array_equal(rel.parent, tree[2])
    assert np.array_equal(bits(rel.vol), bits(tree[3])) and np.array_equal(bits(rel.cur), bits(tree[4]))
    if given_vol_cur is not None:                # origin: every node is a copy of the node it names
        assert np.array_equal(bits(rel.vol), bits(given_vol_cur[0][rel.origin])) and np.array_equal(bits(rel.cur), bits(given_vol_cur[1][rel.origin]))
        assert len(set(rel.origin.tolist())) == len(rel.origin)


# ---- the fixtures ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(FIX)), ids=IDS)
def test_mayfuse_on_the_fixtures(ctx, k):
    """every recorded test, the whole MSA's and every range's, in one batch per column range: the reference's outcome, the restatement's
    stop column, and the restatement's walk over the device's own column scores"""
    name, g = FIX[k]
    alp, weight = cl.alp_of(g), weight_of(g)
    by_range = {}
    for l, r, l0, l1, f, m in fl.all_fixture_tests(g):
        by_range.setdefault((l, r), []).append((l0, l1, f, m))
    for (l, r), tests in by_range.items():
        codes = g["codes"][l:r]
        lists = [t[:2] for t in tests]
        pws = device_pairs(ctx, codes, lists, alp, weight)
        fuse, stop = guide.may_fuse_batch(ctx, pws, alp.u, alp.v)
        want = restated(codes, lists, alp, weight)
        assert [p.alnmode for p in pws] == [t[3] for t in tests] == [w[2] for w in want]
        assert fuse.tolist() == [t[2] for t in tests], (name, l, r)
        assert stop.tolist() == [w[1] for w in want], (name, l, r)
        for i, (rng, s) in enumerate(guide.constwo_batch(ctx, pws, float(g["thr"][0]), want_colscore=True)):
            assert fl.fuse_scan(s, fl.pair_fthr(pws[i], alp.u, alp.v)) == (int(fuse[i]), int(stop[i])), (name, i)


@pytest.mark.parametrize("k", range(len(FIX)), ids=IDS)
def test_relations_and_plan_on_the_fixtures(ctx, k):
    name, g = FIX[k]
    alp, weight, thr = cl.alp_of(g), weight_of(g), float(g["thr"][0])
    codes = g["codes"]
    ln, many = codes.shape
    tree = fl.fixture_tree(g)
    prm, keep = alp.to_c()
    singles = [[m] for m in range(many)]
    # g2g_consregss on the whole MSA
    rel, stats = guide.fuse_groups(ctx, codes, Tree(tree), prm, weight=weight)
    wf, want = fl.fixture_relation(g, "whole")
    assert rel.fused == bool(wf) and stats.tests == len(fl.fixture_tests(g)) and stats.fused == sum(t[2] for t in fl.fixture_tests(g))
    whole = want if wf else (singles,) + tree
    same_relation(rel, whole[0], whole[1:], tree[3:])
    natk = int(g["nrange"][0])
    atk = g["gunited1"].reshape(-1, 2)
    if len(whole[0]) >= 2:
        # g2g_consreg_groups over it, and g2g_consregss inside every range
        for dissim in (0, 1):
            got = guide.conserved_regions_groups(ctx, codes, Tree(whole[1:]), prm, whole[0], thr, weight, bool(dissim))
            assert np.array_equal(got, g["gunited%d" % dissim].reshape(-1, 2)), (name, dissim)
        for i, (l, r) in enumerate(atk.tolist()):
            rr, st = guide.fuse_groups(ctx, codes, Tree(whole[1:]), prm, groups=whole[0], left=l, right=r, weight=weight)
            f, w = fl.fixture_relation(g, "r%d" % i)
            assert rr.fused == bool(f) and st.tests == len(fl.fixture_tests(g, "r%d_test" % i))
            w = w if f else whole
            same_relation(rr, w[0], w[1:], whole[4:6])
    # g2g_refine_plan: all of it in one call
    plan = guide.refine_plan(ctx, codes, Tree(tree), prm, thr, weight)
    assert plan.nothing_to_refine == (len(whole[0]) < 2)
    same_relation(plan.whole, whole[0], whole[1:], tree[3:])
    assert plan.whole.fused == bool(wf)
    assert np.array_equal(plan.ranges, atk) and len(plan.relations) == natk
    assert plan.at_left.tolist() == [int(l == 0) for l, _ in atk.tolist()] and plan.at_right.tolist() == [int(r == ln) for _, r in atk.tolist()]
    for i in range(natk):
        f, w = fl.fixture_relation(g, "r%d" % i)
        w = w if f else whole
        assert plan.relations[i].fused == bool(f)
        same_relation(plan.relations[i], w[0], w[1:], whole[4:6])
    assert plan.stats.tests == len(fl.all_fixture_tests(g))


# ---- hand-made pairs: the score of a column is an entry of a small integer matrix ------------------------------------------------------------
VALS = [1, 5, -1, -2, -3, -4, -7, -8, -10, -17, 3, 4, 11, -6, -16, 0, 2, -5, -9, -12]      # M[3][3 + i]: residue 3 + i of b against residue 3 of a


def hand_alp():
    m = np.zeros((25, 25))
    for i, v in enumerate(VALS):
        m[3, 3 + i] = m[3 + i, 3] = float(v)
    return op.AlnParam(u=3., v=10., u0=0., u1=0., ls=2, sh=100, simmtx=m, max_code=25)       # fthr of two single members: -16


def hand_pairs(ctx, columns):
    """one pair per list of column scores: a is residue 3 throughout, b the residue that scores what is asked for"""
    alp = hand_alp()
    pairs = []
    for s in columns:
        b = np.array([3 + VALS.index(int(x)) for x in s], np.uint8)[:, None]
        pairs.append([op.mSeq(np.full((len(s), 1), 3, np.uint8), alp), op.mSeq(b, alp)])
    return op.PwdM.batch(ctx, pairs, alp)


def run_hand(ctx, columns, want):
    pws = hand_pairs(ctx, columns)
    assert all(p.alnmode == cl.NGP_ALB for p in pws)
    fuse, stop = guide.may_fuse_batch(ctx, pws)
    got = list(zip(fuse.tolist(), stop.tolist()))
    assert got == [fl.fuse_scan(s, -16.) for s in columns]
    assert got == want
    for p, s in zip(pws, columns):               # (the scores are what they were made to be, and fthr is -16)
        assert fl.pair_fthr(p, 3., 10.) == -16. and cl.colscores(p.problem).tolist() == [float(x) for x in s]


@pytest.mark.parametrize("length", [1, T - 1, T, T + 1, 2 * T + 1])
def test_lengths_and_breaks_around_the_tile(ctx, length):
    base = [1] * length
    cols, want = [base], [(1, -1)]
    for c in sorted({0, T - 1, T, length - 1}):
        if c < length:
            s = list(base)
            s[c] = -17                           # the break in column 0, T - 1, T, the last column
            cols.append(s); want.append((0, c))
    s = [-1] * length                            # a slow descent: -17 is reached in column 16, wherever the tiles end
    cols.append(s); want.append((0, 16) if length > 16 else (1, -1))
    if length > T:                               # ... and one that crosses the first tile's end before it breaks
        s = list(base)
        s[T - 8:T + 9] = [-1] * 17
        cols.append(s); want.append((0, T + 8))
    run_hand(ctx, cols, want)


def test_equality_clamp_and_carry(ctx):
    pad = [1] * (T - 2)
    cols = [
        pad + [-8, -8] + [1] * 9,                # lands exactly on fthr across the tile boundary: fuses
        pad + [-8, -8, -1] + [1] * 8,            # one step below it: the break in column T + 1
        pad + [-8, -7, -1, -1] + [1] * 8,        # reaches -16 in column T, -17 in T + 1
        [5, 5, 5, -17] + pad,                    # a positive stretch is clamped to 0 before the negative one: the break in column 3
        [11] * (T - 1) + [-10, -7] + [1] * 9,    # ... also when it fills a whole tile
        [-10, 4, -10] + pad,                     # a negative scr is kept: -10 + 4 - 10 = -16 fuses
        [-10, 3, -10] + pad,                     # -17 does not
        [-10, 11, -10] + pad,
        [-16] + pad, [-16, 0, 0, -1] + pad, [0] * (T + 3),
    ]
    want = [(1, -1), (0, T), (0, T + 1), (0, 3), (0, T), (1, -1), (0, 2), (1, -1), (1, -1), (0, 3), (1, -1)]
    run_hand(ctx, cols, want)


def gap_run_family():
    """twelve members over one ancestor; 0, 3, 10, 11 stay as they are.  Members 4 .. 9 carry mismatches around the tiles' ends (8 and 9
    from in front of the first one, 4 .. 6 from behind it, all of them around the second), so that a walk runs down there without being
    clamped; gap runs lie across both ends"""
    rng = np.random.default_rng(41)
    ln = 2 * T + 40
    fam = np.repeat(rng.integers(3, 23, ln).astype(np.uint8)[:, None], 12, 1)
    second = (2 * T - 3, 2 * T + 12)
    for m, stretches in ((4, ((T + 1, T + 30), second)), (5, ((T + 1, T + 30), second)), (6, ((T + 1, T + 30), second)), (7, (second,)),
                         (8, ((T - 3, T + 30), second)), (9, ((T - 3, T + 30), second))):
        for lo, hi in stretches:
            fam[lo:hi, m] = (fam[lo:hi, m] - 3 + 1 + rng.integers(0, 19, hi - lo)) % 20 + 3
    fam[T - 1:T + 1, 4] = 1                      # a run of two across the first boundary
    fam[T - 2:T + 3, 5] = 1                      # of five
    fam[T - 1:2 * T + 1, 6] = 1                  # a whole tile and both its boundaries
    fam[2 * T - 1:2 * T + 2, 7] = 1              # across the second boundary
    fam[T - 1:T + 2, 8] = 1
    fam[T + 2:T + 4, 1] = 1                      # runs of a's own behind the boundaries, read against b's run lengths
    fam[2 * T:2 * T + 2, 2] = 1
    return fam


CLEAN = (0, 3, 10, 11)
GAP_LISTS = [((0,), (4,)), ((1,), (4,)), ((0, 1), (4,)), ((0, 1), (5,)), ((1, 2), (4, 5)), ((2,), (7,)), ((0, 2), (7,)), ((0, 1, 2), (6,)), ((0, 3), (6, 7)),
             (CLEAN, (8, 9)), ((8, 9), CLEAN), (CLEAN, (6, 7)), ((6, 7), CLEAN), (CLEAN, (4, 5, 8, 9)), (CLEAN, (5, 6, 7, 8, 9)),
             ((0, 1, 2, 3), (8, 9)), ((0, 1, 2, 3), (6, 7)), ((0, 1, 2, 3), (4, 5, 6, 7))]


def negative_since(s, thr):
    """(stop_col, the first column of the unclamped stretch that ends there) of a walk that breaks"""
    scr, since = 0.0, 0
    for i, x in enumerate(s):
        scr += float(x)
        if scr > 0:
            scr = 0.0
        if scr == 0:
            since = i + 1
        if scr < thr:
            return i, since
    return -1, -1


def test_gap_runs_across_a_tile_boundary(ctx):
    """gap runs that begin in one tile and end in the next (one covers a whole tile), read by _nv from both sides, by _hf from the gap
    profiles of a and the run lengths of b: walks that are below 0 from in front of a tile's end to the column where they break behind
    it, so that the column depends on what was carried over -- the restatement's outcome and column in every mode"""
    fam = gap_run_family()
    alp = op.AlnParam(u=3., v=10., u0=0., u1=0., ls=2, sh=100)
    pws = device_pairs(ctx, fam, GAP_LISTS, alp)
    fuse, stop = guide.may_fuse_batch(ctx, pws)
    crossed = set()
    for i, (l0, l1) in enumerate(GAP_LISTS):
        hp = cl.host_pair(fam, (list(l0), list(l1)), alp)
        s = cl.colscores(hp.problem)
        assert hp.alnmode == pws[i].alnmode
        assert (int(fuse[i]), int(stop[i])) == fl.fuse_scan(s, fl.pair_fthr(hp, 3., 10.)), (l0, l1)
        c, since = negative_since(s, fl.pair_fthr(hp, 3., 10.))
        crossed |= {(hp.alnmode, b) for b in (T, 2 * T) if since < b <= c}
    for b in (T, 2 * T):
        assert {m for m, bb in crossed if bb == b} == {cl.NTV_ALB, cl.HLF_ALB, cl.RHF_ALB, cl.GPF_ALB}, (b, crossed)
    cs = guide.constwo_batch(ctx, pws, 35., want_colscore=True)
    for i, p in enumerate(pws):
        assert fl.fuse_scan(cs[i][1], fl.pair_fthr(p, 3., 10.)) == (int(fuse[i]), int(stop[i]))


# ---- order, batches, rounds ------------------------------------------------------------------------------------------------------------------
def test_order_and_batch_size_do_not_matter(ctx):
    g = dict(FIX)["prot16_gapped"]
    alp = cl.alp_of(g)
    lists = [t[:2] for t in fl.fixture_tests(g)]
    pws = device_pairs(ctx, g["codes"], lists, alp)
    fwd = guide.may_fuse_batch(ctx, pws)
    perm = np.random.default_rng(3).permutation(len(pws))
    shuf = guide.may_fuse_batch(ctx, [pws[i] for i in perm])
    assert np.array_equal(shuf[0], fwd[0][perm]) and np.array_equal(shuf[1], fwd[1][perm])
    for i in (0, len(pws) - 1):
        one = guide.may_fuse_batch(ctx, [pws[i]])
        assert one[0].tolist() == [fwd[0][i]] and one[1].tolist() == [fwd[1][i]]
    none = guide.may_fuse_batch(ctx, [])
    assert len(none[0]) == 0 and len(none[1]) == 0
    assert fwd[0].tolist() == [t[2] for t in fl.fixture_tests(g)] and 0 in fwd[0] and 1 in fwd[0]
    # a chunk size of one cuts every round into launches of one test: same relation
    tree = fl.fixture_tree(g)
    prm, keep = alp.to_c()
    a, sa = guide.fuse_groups(ctx, g["codes"], Tree(tree), prm)
    ctx.set_option("FUSE_CHUNK", 1)
    try:
        b, sb = guide.fuse_groups(ctx, g["codes"], Tree(tree), prm)
    finally:
        ctx.set_option("FUSE_CHUNK", None)
    assert [x.tolist() for x in a.groups] == [x.tolist() for x in b.groups] and np.array_equal(a.origin, b.origin)
    assert sa.tests == sb.tests == sb.launches > sa.launches


def test_rounds(ctx):
    # prot12_clusters: every cluster fuses (three rounds deep), the join of two clusters -- both sons fused -- is refused itself, and the
    # root, with a refused son, is not tested
    g = dict(FIX)["prot12_clusters"]
    alp = cl.alp_of(g)
    codes = g["codes"]
    many = codes.shape[1]
    tree = fl.fixture_tree(g)
    rel0 = ([[m] for m in range(many)],) + tree
    ntests, rounds = fl.fuse_rounds(codes, rel0, alp)
    rel, st = guide.fuse_groups(ctx, codes, Tree(tree), alp.to_c()[0])
    assert st.tests == ntests == 10 and st.fused == 9 and st.launches == rounds and len(rel.groups) == 3
    refused = [t for t in fl.fixture_tests(g) if not t[2]]
    assert len(refused) == 1 and len(refused[0][0]) == 4 and len(refused[0][1]) == 4        # two whole clusters
    assert many - 1 - ntests == 1                                                              # of the 11 inner nodes one was never asked
    # prot12_two_rounds: the rounds of its two ranges run together -- the launches are the whole MSA's rounds plus the DEEPEST range's
    g = dict(FIX)["prot12_two_rounds"]
    alp = cl.alp_of(g)
    codes = g["codes"]
    tree = fl.fixture_tree(g)
    _, whole = fl.fixture_relation(g, "whole")
    n0, r0 = fl.fuse_rounds(codes, ([[m] for m in range(codes.shape[1])],) + tree, alp)
    per = [fl.fuse_rounds(codes, whole, alp, None, l, r) for l, r in g["gunited1"].tolist()]
    plan = guide.refine_plan(ctx, codes, Tree(tree), alp.to_c()[0], float(g["thr"][0]))
    assert len(per) == 2 and all(r >= 1 for _, r in per)
    assert plan.stats.tests == n0 + sum(n for n, _ in per)
    assert plan.stats.launches == r0 + max(r for _, r in per) < r0 + sum(r for _, r in per)


# ---- memory, timing ------------------------------------------------------------------------------------------------------------------------
def test_nothing_is_left_allocated(ctx):
    g = dict(FIX)["prot12_two_rounds"]
    alp = cl.alp_of(g)
    pws = device_pairs(ctx, g["codes"], [t[:2] for t in fl.fixture_tests(g)], alp)
    guide.may_fuse_batch(ctx, pws)
    c1 = ctx.mem_counters()
    guide.may_fuse_batch(ctx, pws)
    c2 = ctx.mem_counters()
    # the second call is served from the context's pool and hands its block back
    assert c2["hip_malloc"] == c1["hip_malloc"] and c2["hip_free"] == c1["hip_free"]
    assert c2["pool_hits"] > c1["pool_hits"] and c2["pool_free_bytes"] == c1["pool_free_bytes"]
    del pws
    prm, keep = alp.to_c()
    runs = []
    for _ in range(3):
        guide.refine_plan(ctx, g["codes"], Tree(fl.fixture_tree(g)), prm, float(g["thr"][0]))
        runs.append(ctx.mem_counters())
    # the plan frees its groups and pairs: whatever it took is back in the pool
    assert runs[2]["hip_malloc"] - runs[2]["hip_free"] == runs[1]["hip_malloc"] - runs[1]["hip_free"]
    assert runs[2]["pool_free_bytes"] == runs[1]["pool_free_bytes"]


def test_timing_switch(ctx):
    g = dict(FIX)["prot12_two_rounds"]
    ctx.set_option("FUSE_TIMING", 1)
    try:
        guide.refine_plan(ctx, g["codes"], Tree(fl.fixture_tree(g)), cl.alp_of(g).to_c()[0], float(g["thr"][0]))
        assert float(ctx.get_option("FUSE_KERNEL_MS")) > 0 and float(ctx.get_option("FUSE_BUILD_MS")) > 0
        assert float(ctx.get_option("FUSE_HOST_MS")) >= 0
    finally:
        ctx.set_option("FUSE_TIMING", None)
