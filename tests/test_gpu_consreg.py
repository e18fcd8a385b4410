"""The conserved-region search on the GPU (csrc/g2g_consreg.hip: one workgroup per division, lanes across a tile of 256 columns, one
lane scans): g2g_constwo_batch on pairs the DEVICE builders built -- every column's s bit-equal to the Python restatement
(tests/consreglib.py, on the host-built twins of the same pairs) and the ranges equal to the REFERENCE's (tests/golden/consreg) --,
g2g_consreg equal to the reference's united ranges, and the edges of the tiling on synthetic families: lengths around the tile,
gap runs and ranges across a tile boundary, all-gap columns at a tile's ends, everything / nothing conserved."""
import numpy as np
import pytest

import consreglib as cl
from prrn_aln_amd import engine, guide, operator as op
from prrn_aln_amd.synth import make_family

pytestmark = pytest.mark.gpu
FIX = cl.fixtures()
IDS = [n for n, _ in FIX]
T = 256                                         # CR_T of csrc/g2g_consreg.hip: columns per tile
bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.int64)


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


def device_pairs(ctx, codes, lists, alp, weight=None):
    pairs = []
    for l0, l1 in lists:
        sons = []
        for lst in (l0, l1):
            w = None if weight is None else ([1.0] if len(lst) == 1 else [float(weight[m]) for m in lst])
            sons.append(op.mSeq(np.ascontiguousarray(codes[:, list(lst)]), alp, w))
        pairs.append(sons)
    return op.PwdM.batch(ctx, pairs, alp)


def check(ctx, codes, lists, alp, thr, weight=None):
    """constwo_batch on device-built pairs against the restatement on host-built ones: (modes, [ranges])"""
    pws = device_pairs(ctx, codes, lists, alp, weight)
    got = guide.constwo_batch(ctx, pws, thr, want_colscore=True)
    plain = guide.constwo_batch(ctx, pws, thr)
    modes, out = [], []
    for k, (l0, l1) in enumerate(lists):
        hp = cl.host_pair(codes, (list(l0), list(l1)), alp, weight)
        assert hp.alnmode == pws[k].alnmode
        s = cl.colscores(hp.problem)
        want = cl.scan(s, cl.vthr_of(hp, thr))
        assert np.array_equal(bits(got[k][1]), bits(s)), (k, l0, l1, cl.MODE_NAME[hp.alnmode], np.flatnonzero(bits(got[k][1]) != bits(s))[:8])
        assert [tuple(r) for r in got[k][0].tolist()] == want, (k, l0, l1)
        assert np.array_equal(plain[k], got[k][0])
        modes.append(hp.alnmode); out.append(want)
    return modes, out


@pytest.mark.parametrize("k", range(len(FIX)), ids=IDS)
def test_constwo_on_the_fixtures(ctx, k):
    """a batch of all recorded divisions (2 N - 3 of the tree, and the exchanged ones): s of every column, and the reference's ranges"""
    name, g = FIX[k]
    alp, thr = cl.alp_of(g), float(g["thr"][0])
    weight = g["weight"] if len(g["weight"]) else None
    divs = cl.fixture_divisions(g)
    modes, rng = check(ctx, g["codes"], [d[:2] for d in divs], alp, thr, weight)
    assert modes == g["div_mode"].tolist()
    assert rng == [d[2] for d in divs]


@pytest.mark.parametrize("k", range(len(FIX)), ids=IDS)
def test_consreg_on_the_fixtures(ctx, k):
    name, g = FIX[k]
    alp, thr = cl.alp_of(g), float(g["thr"][0])
    weight = g["weight"] if len(g["weight"]) else None

    class Tree:
        left, right, parent = g["tree_left"], g["tree_right"], g["tree_parent"]
    prm, keep = alp.to_c()
    for dissim in (0, 1):
        got = guide.conserved_regions(ctx, g["codes"], Tree, prm, thr, weight, bool(dissim))
        assert np.array_equal(got, g["united%d" % dissim].reshape(-1, 2)), (name, dissim)


def test_order_and_batch_size_do_not_matter(ctx):
    g = dict(FIX)["prot12_hf"]
    alp, thr = cl.alp_of(g), float(g["thr"][0])
    divs = [d for d in cl.fixture_divisions(g) if d[3]]
    pws = device_pairs(ctx, g["codes"], [d[:2] for d in divs], alp)
    fwd = guide.constwo_batch(ctx, pws, thr)
    rev = guide.constwo_batch(ctx, pws[::-1], thr)[::-1]
    one = [guide.constwo_batch(ctx, [p], thr)[0] for p in pws[:3]]
    assert all(np.array_equal(a, b) for a, b in zip(fwd, rev)) and all(np.array_equal(a, b) for a, b in zip(fwd, one))
    ln = g["codes"].shape[0]
    for order in (fwd, fwd[::-1]):
        united = [(0, ln)]
        for r in order:
            united = cl.cmnrng(united, [tuple(x) for x in r.tolist()])
        assert united == [tuple(x) for x in g["united0"].tolist()]
    assert guide.constwo_batch(ctx, [], thr) == []

    class Tree:                                  # a small chunk size cuts the divisions into several launches: same result
        left, right, parent = g["tree_left"], g["tree_right"], g["tree_parent"]
    ctx.set_option("CONSREG_CHUNK", 4)
    try:
        got = guide.conserved_regions(ctx, g["codes"], Tree, alp.to_c()[0], thr, None, True)
    finally:
        ctx.set_option("CONSREG_CHUNK", None)
    assert np.array_equal(got, g["united1"].reshape(-1, 2))


# ---- the edges of the tiling ------------------------------------------------------------------------------------------------
ALP = op.AlnParam(u=3., v=10., u0=0., u1=0., ls=2, sh=100)
LISTS_PF = [((0, 1, 2, 3, 4, 5, 6, 7, 8), (9,)), ((5, 6, 7, 8, 9), (0, 1, 2, 3, 4)), ((2, 3, 4, 5, 6, 7, 8, 9), (0, 1))]
LISTS_NV = [((0,), (1,)), ((0, 1), (2,)), ((3,), (4, 5)), ((6, 7), (8, 9)), ((2, 3, 4), (5,))]


@pytest.fixture(scope="module")
def wide():
    """10 members x > 2 T + 1 columns with gaps; members 0 and 1 made free of gaps; and a family without any gap"""
    fam = op.encode(list(make_family(10, 480, 91, indel=0.02, sub=0.15).msa), op.PROTEIN)
    assert fam.shape[0] >= 2 * T + 1
    clean = fam.copy()
    for m in (0, 1):
        holes = clean[:, m] <= 1
        clean[holes, m] = 3 + (np.flatnonzero(holes) % 20)
    rng = np.random.default_rng(5)
    anc = rng.integers(3, 23, 2 * T + 1).astype(np.uint8)
    nogap = np.repeat(anc[:, None], 6, 1)
    hit = rng.random(nogap.shape) < 0.2
    nogap[hit] = rng.integers(3, 23, int(hit.sum()))
    return fam, clean, nogap


@pytest.mark.parametrize("length", [1, T - 1, T, T + 1, 2 * T + 1])
def test_lengths_around_the_tile(ctx, wide, length):
    fam, clean, nogap = wide
    seen = set()
    m, _ = check(ctx, fam[:length], LISTS_PF + LISTS_NV, ALP, 10.); seen |= set(m)
    m, _ = check(ctx, clean[:length], [((2, 3, 4, 5, 6, 7, 8, 9), (0, 1)), ((0, 1), (2, 3, 4, 5, 6, 7, 8, 9)), ((3, 4, 5, 6, 7, 8, 9), (0,))], ALP, 10.); seen |= set(m)
    m, _ = check(ctx, nogap[:length], [((0, 1, 2), (3, 4, 5)), ((0,), (1,)), ((1, 2, 3, 4, 5), (0,))], ALP, 10.); seen |= set(m)
    if length >= T - 1:                          # (one column of this family holds no gap)
        assert seen == {cl.NGP_ALB, cl.HLF_ALB, cl.RHF_ALB, cl.GPF_ALB, cl.NTV_ALB}


def test_gap_runs_across_a_tile_boundary(ctx, wide):
    """a member's gap run that begins in one tile and ends in the next (and one that covers a whole tile), read by _nv from both sides
    and by _hf from the gap profiles of a and the run lengths of b"""
    fam = wide[1][:2 * T + 40].copy()
    fam[T - 7:T + 9, 2] = 1                      # across the first boundary
    fam[T - 1:2 * T + 3, 3] = 1                  # a whole tile and both its boundaries
    fam[0:T + 1, 4] = 1                          # from the first column on: pregap's zero, then a run longer than a tile
    fam[2 * T - 1:2 * T + 1, 5] = 1
    modes, _ = check(ctx, fam, [((2,), (3,)), ((2, 4), (3,)), ((3,), (4, 5)), ((4,), (0,)), ((2, 3), (4, 5)), ((5,), (3,)),
                               ((2, 3, 4, 5, 6, 7, 8, 9), (0, 1)), ((0, 1), (2, 3, 4, 5, 6, 7, 8, 9)), ((2, 3, 4, 5, 6, 7), (0,))], ALP, 10.)
    assert modes.count(cl.NTV_ALB) >= 5 and cl.HLF_ALB in modes and cl.RHF_ALB in modes


def test_a_range_that_opens_in_one_tile_and_closes_in_the_next(ctx):
    rng = np.random.default_rng(17)
    ln = 2 * T + 30
    codes = rng.integers(3, 23, (ln, 6)).astype(np.uint8)          # unrelated members: nothing conserved ...
    for lo, hi in ((T - 20, T + 25), (2 * T - 3, 2 * T + 4), (40, 60)):
        codes[lo:hi] = codes[lo:hi, :1]                              # ... but for three identical blocks, two of them across a boundary
    codes[T + 30:T + 40, 2] = 1
    modes, out = check(ctx, codes, [((0, 1, 2), (3, 4, 5)), ((0, 1, 3, 4, 5), (2,)), ((0,), (1,))], ALP, 20.)
    for r in out:
        assert any(l < T < rr for l, rr in r) and any(l < 2 * T < rr for l, rr in r), r


def test_everything_and_nothing_conserved(ctx):
    rng = np.random.default_rng(23)
    ln = 2 * T + 1
    same = np.repeat(rng.integers(3, 23, ln).astype(np.uint8)[:, None], 5, 1)
    _, out = check(ctx, same, [((0, 1, 2), (3, 4)), ((0,), (1,))], ALP, 35.)
    assert out == [[(0, ln)], [(0, ln)]]
    alien = rng.integers(3, 23, (ln, 5)).astype(np.uint8)
    alien[:, 3:] = (alien[:, :2] - 3 + 7) % 20 + 3                 # never the same residue as its partner
    _, out = check(ctx, alien, [((0, 1), (3, 4)), ((0,), (3,))], ALP, 35.)
    assert out == [[], []]


def test_all_gap_columns_at_the_ends_of_a_tile(ctx, wide):
    """a son whose column is all gaps stays in place (extseq drops nothing): first and last column of the first two tiles, and the last column"""
    fam = wide[0][:2 * T + 1].copy()
    for c in (0, T - 1, T, 2 * T - 1, 2 * T):
        fam[c, 7:] = 1
    modes, _ = check(ctx, fam, [((0, 1, 2, 3, 4, 5, 6), (7, 8, 9)), ((7, 8, 9), (0, 1, 2, 3, 4, 5, 6)), ((0, 1), (9,)), ((8,), (9,))], ALP, 10.)
    assert cl.GPF_ALB in modes and cl.NTV_ALB in modes


def test_nothing_is_left_allocated(ctx):
    name, g = "prot16_pf", dict(FIX)["prot16_pf"]
    alp, thr = cl.alp_of(g), float(g["thr"][0])
    pws = device_pairs(ctx, g["codes"], [d[:2] for d in cl.fixture_divisions(g)], alp)
    guide.constwo_batch(ctx, pws, thr, want_colscore=True)
    c1 = ctx.mem_counters()
    guide.constwo_batch(ctx, pws, thr, want_colscore=True)
    c2 = ctx.mem_counters()
    # the second call is served from the context's pool and hands its block back: no hipMalloc, the pool as full as before
    assert c2["hip_malloc"] == c1["hip_malloc"] and c2["hip_free"] == c1["hip_free"]
    assert c2["pool_hits"] > c1["pool_hits"] and c2["pool_free_bytes"] == c1["pool_free_bytes"]
    del pws

    class Tree:
        left, right, parent = g["tree_left"], g["tree_right"], g["tree_parent"]
    prm, keep = alp.to_c()
    runs = []
    for _ in range(3):
        guide.conserved_regions(ctx, g["codes"], Tree, prm, thr)
        runs.append(ctx.mem_counters())
    # g2g_consreg frees its groups and pairs: whatever it took -- builders' slabs, twins, the kernel's block -- is back in the pool
    assert runs[2]["hip_malloc"] - runs[2]["hip_free"] == runs[1]["hip_malloc"] - runs[1]["hip_free"]
    assert runs[2]["pool_free_bytes"] == runs[1]["pool_free_bytes"]


def test_timing_switch(ctx):
    name, g = "prot16_pf", dict(FIX)["prot16_pf"]

    class Tree:
        left, right, parent = g["tree_left"], g["tree_right"], g["tree_parent"]
    ctx.set_option("CONSREG_TIMING", 1)
    try:
        guide.conserved_regions(ctx, g["codes"], Tree, cl.alp_of(g).to_c()[0], float(g["thr"][0]))
        assert float(ctx.get_option("CONSREG_KERNEL_MS")) > 0 and float(ctx.get_option("CONSREG_BUILD_MS")) > 0
    finally:
        ctx.set_option("CONSREG_TIMING", None)
