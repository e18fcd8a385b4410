"""k-mer composition distances on the GPU: g2g_kmer_dist_batch (csrc/g2g_kmer.hip: one workgroup sorts and counts the words of a
sequence in LDS; a wave intersects two lists) against the Python restatement of the reference's calcdist_kmer (tests/kmerlib.py)
-- the three integers of every pair equal, the distances bit-equal to g2g_kmer_dist_from_counts and to the restatement -- and
against the distances the REFERENCE computed (tests/golden/kmer) within the tolerance of tests/test_kmer_host.py.  Shapes: the
window edges, every size at which the sort changes (sort sizes are powers of two; above 1024 words a thread takes several
entries), the largest window and one more, duplicate-rich and extreme words, both pair forms, and the guide tree at the end."""
import numpy as np
import pytest

import kmerlib
import ktreelib
from kmerlib import DNA, PROTEIN, bits
from prrn_aln_amd import engine, guide
from prrn_aln_amd._lib import G2GError
from prrn_aln_amd.refine import KTree

pytestmark = pytest.mark.gpu
FIX = kmerlib.fixtures()
ELEM = {PROTEIN: np.arange(3, 23), DNA: np.array([2, 3, 5, 9])}
OTHER = {PROTEIN: np.array([0, 1, 2, 23, 24, 25, 200]), DNA: np.array([0, 1, 4, 6, 16, 10, 255])}


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


def same_bits(a, b):
    n = np.isnan(a)
    return a.shape == b.shape and np.array_equal(n, np.isnan(b)) and np.array_equal(bits(a[~n]), bits(b[~n]))


def check(ctx, seqs, molc, k=0, measure=-1, ia=None, ib=None):
    want_d, want_c = kmerlib.distance(seqs, molc, k, measure, ia, ib)
    got_d, got_c = guide.kmer_distance(ctx, seqs, molc, k, measure, ia, ib, want_counts=True)
    assert np.array_equal(got_c, want_c)
    assert same_bits(got_d, guide.kmer_dist_from_counts(got_c, molc, k, measure)) and same_bits(got_d, want_d)
    assert same_bits(guide.kmer_distance(ctx, seqs, molc, k, measure, ia, ib), got_d)          # (counts = NULL)
    return got_d, got_c


def random_seq(rng, molc, n, letters=None):
    return rng.choice(ELEM[molc] if letters is None else ELEM[molc][:letters], n).astype(np.uint8)


def family(rng, molc, n, many, rate=0.1, letters=None):
    anc = random_seq(rng, molc, n, letters)
    out = []
    for _ in range(many):
        s = anc.copy()
        m = rng.random(n) < rate
        s[m] = random_seq(rng, molc, int(m.sum()), letters)
        out.append(s)
    return out


@pytest.mark.parametrize("k", range(len(FIX)), ids=[n for n, _ in FIX])
def test_fixtures_from_the_reference(ctx, k):
    g = FIX[k][1]
    got, _ = check(ctx, kmerlib.split(g), int(g["molc"][0]), int(g["k"][0]), int(g["measure"][0]))
    assert kmerlib.close_to_reference(got, g["dist"])


@pytest.mark.parametrize("molc,k", [(PROTEIN, 1), (PROTEIN, 5), (PROTEIN, 6), (DNA, 3), (DNA, 10), (DNA, 15)])
def test_window_edges(ctx, molc, k):
    """lengths 0, 1, 2 k - 1 (no word), 2 k (one), 2 k + 1; a non-elementary residue at the first and at the last window position,
    two exactly k apart, k - 1 and k + 1 apart, runs, and inside the last k residues, which the scan never reads"""
    rng = np.random.default_rng(100 * molc + k)
    n = 6 * k + 9
    base = random_seq(rng, molc, n, 3)
    x = OTHER[molc]
    seqs = [base[:0], base[:1], base[:2 * k - 1], base[:2 * k], base[:2 * k + 1], base]

    def broken(at, code=None):
        s = base.copy()
        s[list(at)] = x[rng.integers(len(x))] if code is None else code
        return s

    last = n - k - 1                                                    # the last residue read
    seqs += [broken([0]), broken([last]), broken([last + 1]), broken(range(n - k, n)), broken([k - 1]), broken([k]),
             broken([5, 5 + k]), broken([5, 5 + k - 1]), broken([5, 5 + k + 1]), broken(range(4, 4 + k)), broken(range(4, 6 + k)),
             broken([0, last]), broken(range(0, n, k)), broken(range(0, n, k + 1)), broken(range(n)), broken([7], 1), broken([7], 0)]
    _, cnt = check(ctx, seqs, molc, k, 0)
    T = [kmerlib.profile(s, molc, k)[2] for s in seqs]                  # (the shapes are what they are meant to be)
    full = n - 2 * k + 1
    assert T[:6] == [0, 0, 0, 1, 2, full]
    # a flaw at the first or the last position read costs one word each, one behind the last read none
    assert T[6] == full - 1 and T[7] == full - 1 and T[17] == full - 2 and T[8] == full and T[9] == full
    assert T[18] == 0 and T[20] == 0 and 0 < T[19] < full              # a flaw every k residues leaves no word, every k + 1 some
    assert cnt[kmerlib.elem(5, 8), 0] == full                           # identical as far as the scan reads
    assert [int(c) for c in cnt[kmerlib.elem(5, 6)][1:]] == [full, full - 1]


@pytest.mark.parametrize("words", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 4097])
def test_sort_edges(ctx, words):
    """the number of word positions around every power of two: the sort size doubles behind it, and above 1024 a thread of the
    run compaction takes 2, 4, ... entries"""
    rng = np.random.default_rng(words)
    for molc, k, letters in ((PROTEIN, 3, 3), (DNA, 8, None)):
        n = words + 2 * k - 1
        seqs = family(rng, molc, n, 3, 0.05, letters) + [random_seq(rng, molc, n + 1, letters), random_seq(rng, molc, max(n - 1, 0), letters)]
        seqs[1][n // 2] = OTHER[molc][0]                                # invalid positions go behind the words
        _, cnt = check(ctx, seqs, molc, k, 0)
        assert cnt[kmerlib.elem(0, 2), 1] == words


def test_largest_window_and_one_more(ctx):
    """G2G_KMER_MAX_WINDOW = 16384 word positions: few distinct words (two letters), all distinct ones likely (DNA k = 15), a broken
    one; one position more is refused and the sequence named"""
    rng = np.random.default_rng(7)
    W = kmerlib.MAX_WINDOW
    k = 6
    n = W + 2 * k - 1
    a = random_seq(rng, PROTEIN, n, 2)
    b = a.copy()
    b[rng.random(n) < 0.01] = ELEM[PROTEIN][2]
    c = random_seq(rng, PROTEIN, n)
    c[::997] = 2
    _, cnt = check(ctx, [a, b, c, a[:300]], PROTEIN, k, 0)
    assert cnt[0, 1] == W and cnt[0, 2] == W and 0 < cnt[0, 0] < W
    k = 15
    n = W + 2 * k - 1
    fam = family(rng, DNA, n, 3, 0.01)
    _, cnt = check(ctx, fam, DNA, k, 1)
    assert (cnt[:, 1] == W).all()
    with pytest.raises(G2GError, match="sequence 1 has 16385 word positions"):
        guide.kmer_distance(ctx, [fam[0], np.append(fam[1], fam[1][:1]), fam[2]], DNA, k)
    inside = (np.concatenate([fam[1][:9], fam[1], fam[1][:9]]), 9, 9 + n)          # the window counts, not the buffer
    check(ctx, [fam[0], inside], DNA, k, 1)


def test_duplicates_and_extreme_words(ctx):
    rng = np.random.default_rng(9)
    # homopolymers: one key with count T; the largest words (all-T DNA at k = 15 is 4^15 - 1, all-V protein at k = 6 is 20^6 - 1)
    for molc, k, top in ((DNA, 15, 9), (PROTEIN, 6, 22), (DNA, 1, 9), (PROTEIN, 1, 22)):
        low = ELEM[molc][0]
        seqs = [np.full(300, top, np.uint8), np.full(200, top, np.uint8), np.full(250, low, np.uint8), np.full(2 * k, top, np.uint8),
                np.concatenate([np.full(150, low, np.uint8), np.full(150, top, np.uint8)])]
        w, c, T = kmerlib.profile(seqs[0], molc, k)
        assert list(w) == [(20 if molc == PROTEIN else 4) ** k - 1] and list(c) == [T] == [300 - 2 * k + 1]
        d, cnt = check(ctx, seqs, molc, k, 0)
        assert cnt[kmerlib.elem(0, 1), 0] == 200 - 2 * k + 1             # min(count) is the shorter one's T
        assert cnt[kmerlib.elem(0, 2), 0] == 0 and d[kmerlib.elem(0, 2)] == 100. and d[kmerlib.elem(0, 1)] == 0.
        assert cnt[kmerlib.elem(0, 3), 0] == 1
    # two and three letters: counts above 1 on both sides, so min matters
    for molc, k, letters in ((PROTEIN, 2, 2), (PROTEIN, 4, 3), (DNA, 5, 2), (DNA, 7, 3)):
        seqs = [random_seq(rng, molc, n, letters) for n in (500, 333, 777, 64, 1500)]
        _, cnt = check(ctx, seqs, molc, k, 2 if molc == PROTEIN else 6)
        pr = [kmerlib.profile(s, molc, k) for s in seqs]
        both = np.intersect1d(pr[0][0], pr[2][0])                       # s above the number of shared words: a count above 1 went in
        assert min(p[1].max() for p in pr) > 1 and cnt[kmerlib.elem(0, 2), 0] > len(both) > 0

def test_disjoint_identical_and_ordered_lists(ctx):
    rng = np.random.default_rng(13)
    k = 4
    lo = rng.choice(ELEM[PROTEIN][:5], 400).astype(np.uint8)            # every word of lo is below every word of hi
    hi = rng.choice(ELEM[PROTEIN][10:], 400).astype(np.uint8)
    mixed = np.concatenate([lo[:200], hi[:200]])
    seqs = [lo, hi, lo.copy(), mixed, hi[::-1].copy()]
    assert kmerlib.profile(lo, PROTEIN, k)[0].max() < kmerlib.profile(hi, PROTEIN, k)[0].min()
    d, cnt = check(ctx, seqs, PROTEIN, k, 0)
    assert cnt[kmerlib.elem(0, 1), 0] == 0 and cnt[kmerlib.elem(0, 2), 0] == cnt[kmerlib.elem(0, 2), 1] and d[kmerlib.elem(0, 2)] == 0.
    assert 0 < cnt[kmerlib.elem(0, 3), 0] < cnt[kmerlib.elem(0, 3), 1]


@pytest.mark.parametrize("nseq", [2, 3, 16, 17, 33, 66, 130])
def test_all_pairs_member_counts(ctx, nseq):
    """a workgroup of the all-pairs kernel takes 64 partners, a wave every fourth of them: 65 / 66 members begin a second chunk"""
    rng = np.random.default_rng(nseq)
    seqs = family(rng, PROTEIN, 150, nseq, 0.15)
    seqs = [s[: 150 - (3 * i) % 40] for i, s in enumerate(seqs)]
    check(ctx, seqs, PROTEIN, 3, -1)
    dna = [s[: 90 + (7 * i) % 50] for i, s in enumerate(family(rng, DNA, 140, nseq, 0.05))]
    check(ctx, dna, DNA, 0, -1)


@pytest.mark.parametrize("measure", range(7))
def test_every_measure(ctx, measure):
    rng = np.random.default_rng(measure)
    check(ctx, family(rng, PROTEIN, 200, 6, 0.1) + [random_seq(rng, PROTEIN, 9)], PROTEIN, 4, measure)
    check(ctx, family(rng, DNA, 200, 6, 0.03) + [random_seq(rng, DNA, 5)], DNA, 8, measure)


def test_pair_list_form(ctx):
    """(j, i) beside (i, j), repeats, (i, i), a list longer than the number of sequences, lists of very different lengths (the
    kernel streams the shorter one)"""
    rng = np.random.default_rng(21)
    seqs = family(rng, PROTEIN, 300, 7, 0.1) + [random_seq(rng, PROTEIN, 2000, 4), random_seq(rng, PROTEIN, 12), random_seq(rng, PROTEIN, 5)]
    n = len(seqs)
    ia = [0, 1, 0, 0, 3, 3, 7, 2, 8, 9, 9, 7, 6] + list(rng.integers(0, n, 40))
    ib = [1, 0, 1, 1, 3, 4, 2, 7, 8, 9, 0, 7, 6] + list(rng.integers(0, n, 40))
    d, cnt = check(ctx, seqs, PROTEIN, 3, 0, ia, ib)
    assert list(cnt[0]) == [cnt[1][0], cnt[1][2], cnt[1][1]] and list(cnt[2]) == list(cnt[0]) == list(cnt[3])
    assert d[4] == 0. and cnt[4][0] == cnt[4][1] == cnt[4][2] == 300 - 5          # qdiv(a, a)
    assert np.isnan(d[9]) and list(cnt[9]) == [0, 0, 0]                # a wordless member with itself
    all_d, all_c = guide.kmer_distance(ctx, seqs, PROTEIN, 3, 0, want_counts=True)
    for p, (a, b) in enumerate(zip(ia, ib)):
        if a < b:
            assert list(cnt[p]) == list(all_c[kmerlib.elem(a, b)]) and same_bits(d[p:p + 1], all_d[kmerlib.elem(a, b):][:1])
    one_d, one_c = check(ctx, seqs, PROTEIN, 3, 0, [5], [2])           # a single pair
    assert list(one_c[0][[0, 2, 1]]) == list(all_c[kmerlib.elem(2, 5)])
    with pytest.raises(G2GError, match="pair 1"):
        guide.kmer_distance(ctx, seqs, PROTEIN, 3, 0, [0, n], [1, 1])


def test_left_right_inside_a_longer_buffer(ctx):
    rng = np.random.default_rng(23)
    fam = family(rng, DNA, 400, 5, 0.05)
    buf = [(np.concatenate([random_seq(rng, DNA, 17 * i), s, random_seq(rng, DNA, 40 - 7 * i)]), 17 * i, 17 * i + len(s)) for i, s in enumerate(fam)]
    d, cnt = check(ctx, buf, DNA, 6, 6)
    d0, cnt0 = check(ctx, fam, DNA, 6, 6)
    assert np.array_equal(cnt, cnt0) and same_bits(d, d0)
    sub = [(s, 30, 330) for s in fam]
    d1, cnt1 = check(ctx, sub, DNA, 6, 6)
    assert (cnt1[:, 1] == 300 - 11).all() and not np.array_equal(cnt1, cnt0)
    check(ctx, [(fam[0], 10, 10), (fam[1], 400, 400), fam[2]], DNA, 6, 6)      # empty ranges


def same_tree(t, r):
    assert list(t.left) == list(r["left"]) and list(t.right) == list(r["right"]) and list(t.parent) == list(r["parent"])
    assert np.array_equal(bits(t.height), bits(r["height"])) and np.array_equal(bits(t.length), bits(r["length"]))


@pytest.mark.parametrize("k", [i for i, (n, _) in enumerate(FIX) if "edges" not in n], ids=[n for n, _ in FIX if "edges" not in n])
def test_guide_tree_of_the_fixtures(ctx, k):
    g = FIX[k][1]
    dist = guide.kmer_distance(ctx, kmerlib.split(g), int(g["molc"][0]), int(g["k"][0]), int(g["measure"][0]))
    assert not np.isnan(dist).any()
    t = KTree.from_dist(dist, with_weights=False)
    same_tree(t, ktreelib.tree_from_dist(dist))
    assert t.n_leaves == len(g["lens"]) and not any(t.vol)


def test_guide_tree_refuses_the_wordless_member(ctx):
    g = dict(FIX)["prot10_edges_k4_qcdiv"]
    dist = guide.kmer_distance(ctx, kmerlib.split(g), 1, 4, 2)
    assert np.isnan(dist[kmerlib.elem(0, 6)])
    with pytest.raises(G2GError, match="members 0 and 6"):
        KTree.from_dist(dist, with_weights=False)


def test_timing_option(ctx):
    rng = np.random.default_rng(31)
    ctx.set_option("KMER_TIMING", 1)
    try:
        check(ctx, family(rng, PROTEIN, 200, 5), PROTEIN)
        assert float(ctx.get_option("KMER_PROFILE_MS")) > 0 and float(ctx.get_option("KMER_PAIRS_MS")) > 0
    finally:
        ctx.set_option("KMER_TIMING", None)
