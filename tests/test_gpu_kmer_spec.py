"""k-mer composition distances over reduced alphabets and under spaced seeds on the GPU: g2g_kmer_dist_batch_spec
(csrc/g2g_kmer.hip: g2g_kmer_profile_spec_kernel stages the class table and the class digits in LDS and reads every word's digits
at the seed's offsets; sort, run compaction and the pair kernels are those of g2g_kmer_dist_batch) against the Python restatement
(tests/kmerspeclib.py) -- the three integers of every pair equal, the distances bit-equal to g2g_kmer_dist_from_counts_spec and to
the restatement -- and against the distances the REFERENCE computed (tests/golden/kmer_spec) within the tolerance of
tests/test_kmer_spec_host.py.  Shapes: the window edges counted with the seed's width, a bad residue under every position of a
seed, the class at the alphabet's edge, the largest words, the sizes at which the sort changes, the largest window and one more
(the class table lies in the dynamic LDS above 64 KB), both pair forms, and the guide tree at the end."""
import numpy as np
import pytest

import kmerlib
import kmerspeclib as ks
import ktreelib
from kmerlib import DNA, PROTEIN, bits
from prrn_aln_amd import engine, guide
from prrn_aln_amd._lib import G2GError
from prrn_aln_amd.refine import KTree

pytestmark = pytest.mark.gpu
FIX = ks.fixtures()
OLD = dict(kmerlib.fixtures())
PAT14 = ks.case(dict(FIX)["prot24_a14_k3_qcdiv"])["classes"]          # the 14-class pattern that fixture records; X is class 14
TAB14 = ks.classes_from_pattern(PAT14, PROTEIN)
W32 = "1" + "0" * 14 + "11" + "0" * 14 + "1"                           # width 32, weight 4
X = 2


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


def same_bits(a, b):
    n = np.isnan(a)
    return a.shape == b.shape and np.array_equal(n, np.isnan(b)) and np.array_equal(bits(a[~n]), bits(b[~n]))


def check(ctx, seqs, molc, k=0, measure=-1, nalpha=0, classes=None, seed=None, ia=None, ib=None):
    want_d, want_c = ks.distance(seqs, molc, k, measure, nalpha, classes, seed, ia, ib)
    got_d, got_c = guide.kmer_distance_spec(ctx, seqs, molc, k, measure, nalpha, classes, seed, ia, ib, want_counts=True)
    assert np.array_equal(got_c, want_c)
    assert same_bits(got_d, guide.kmer_dist_from_counts_spec(got_c, molc, k, measure, nalpha, seed)) and same_bits(got_d, want_d)
    assert same_bits(guide.kmer_distance_spec(ctx, seqs, molc, k, measure, nalpha, classes, seed, ia, ib), got_d)      # (counts = NULL)
    return got_d, got_c


def protein(rng, n, letters=20):
    return rng.integers(3, 3 + letters, n).astype(np.uint8)


def dna(rng, n):
    return rng.choice([2, 3, 5, 9], n).astype(np.uint8)


def family(rng, anc, many, rate, draw):
    out = []
    for _ in range(many):
        s = anc.copy()
        m = rng.random(len(s)) < rate
        s[m] = draw(rng, int(m.sum()))
        out.append(s)
    return out


@pytest.mark.parametrize("k", range(len(FIX)), ids=[n for n, _ in FIX])
def test_fixtures_from_the_reference(ctx, k):
    g = FIX[k][1]
    got, _ = check(ctx, ks.split(g), **ks.case(g))
    assert ks.close_to_reference(got, g["dist"])


@pytest.mark.parametrize("name", ["prot24_default", "dna24_k6_njuca"])
def test_default_spec_is_the_old_entry(ctx, name):
    """nalpha 0, no classes, no seed: the new profile kernel with the full alphabet's table against g2g_kmer_profile_kernel"""
    g = OLD[name]
    molc, k, measure = int(g["molc"][0]), int(g["k"][0]), int(g["measure"][0])
    seqs = kmerlib.split(g)
    d0, c0 = guide.kmer_distance(ctx, seqs, molc, k, measure, want_counts=True)
    d1, c1 = guide.kmer_distance_spec(ctx, seqs, molc, k, measure, want_counts=True)
    assert np.array_equal(c0, c1) and same_bits(d0, d1)
    assert kmerlib.close_to_reference(d1, g["dist"])


@pytest.mark.parametrize("molc,k,nalpha", [(PROTEIN, 4, 14), (PROTEIN, 7, 14), (PROTEIN, 6, 20), (DNA, 15, 4), (DNA, 1, 4)])
def test_all_ones_seed_is_the_continuous_seed(ctx, molc, k, nalpha):
    rng = np.random.default_rng(10 * k + molc)
    if molc == PROTEIN:
        seqs = family(rng, protein(rng, 300), 5, 0.1, protein) + [protein(rng, 2 * k), protein(rng, 2 * k - 1)]
        seqs[1][[5, 100]] = X
        classes = PAT14 if nalpha == 14 else None
    else:
        seqs = family(rng, dna(rng, 300), 5, 0.05, dna) + [dna(rng, 2 * k), dna(rng, 2 * k - 1)]
        seqs[1][[5, 100]] = 16
        classes = None
    d0, c0 = check(ctx, seqs, molc, k, 2, nalpha, classes)
    d1, c1 = check(ctx, seqs, molc, k, 2, nalpha, classes, "1" * k)
    assert np.array_equal(c0, c1) and same_bits(d0, d1)


@pytest.mark.parametrize("seed", ["1011", "110101", "11", "1", W32, "1" + "0" * 30 + "1"])
def test_window_edges_under_a_seed(ctx, seed):
    """lengths 0, 1, 2 width - 1 (no word), 2 width (one), 2 width + 1; a bad residue under every offset of the seed at the first
    word position, in the middle and at the last one -- under a '1' the word is lost, under a '0' it is kept; at the first and the
    last residue read; inside the last width residues, which the scan never reads"""
    rng = np.random.default_rng(len(seed))
    w = len(seed)
    ones = [o for o, ch in enumerate(seed) if ch == "1"]
    n = 6 * w + 9
    full = n - 2 * w + 1
    base = protein(rng, n, 3)
    seqs = [base[:0], base[:1], base[:2 * w - 1], base[:2 * w], base[:2 * w + 1], base]

    def broken(at, code=X):
        s = base.copy()
        s[list(at)] = code
        return s

    last = n - w - 1                                                    # the last residue read
    at = [p0 + o for p0 in (0, 2 * w + 3, full - 1) for o in range(w)]  # every offset of the first, a middle and the last word position
    seqs += [broken([p]) for p in at]
    seqs += [broken([last + 1]), broken(range(n - w, n)), broken([0, last]), broken(range(n)), broken([7], 1), broken([7], 0), broken([7], 200)]
    _, cnt = check(ctx, seqs, PROTEIN, 4, 0, 14, PAT14, seed)
    T = [ks.profile(s, TAB14, 14, 4, seed)[2] for s in seqs]
    assert T[:6] == [0, 0, 0, 1, 2, full]
    for i, p in enumerate(at):                                          # the words that examine residue p: one per '1' whose position exists
        lost = sum(1 for o in ones if 0 <= p - o < full)
        assert T[6 + i] == full - lost, (p, lost)
    if "0" in seed:
        zero = seed.index("0")
        assert T[6 + zero] == full - sum(1 for o in ones if o <= zero)  # under a '0' of the first position: that word is kept
    m = 6 + len(at)
    assert T[m] == full and T[m + 1] == full and T[m + 2] == full - 2 and T[m + 3] == 0
    assert T[m + 4] == T[m + 5] == T[m + 6] == full - sum(1 for o in ones if 0 <= 7 - o < full)      # gap, nil, a code the table does not hold
    assert cnt[kmerlib.elem(5, m), 0] == full                           # identical as far as the scan reads


def test_class_at_the_alphabets_edge_and_short_tables(ctx):
    """class nalpha - 1 is the last digit, class nalpha breaks the word; codes >= nclasses break it too"""
    rng = np.random.default_rng(3)
    tab = np.arange(256).astype(np.uint8)                               # class = code
    for nalpha, seed, k in ((14, None, 3), (14, "1011", 4), (2, None, 9), (20, "1101", 5), (7, None, 10)):
        seqs = [rng.integers(0, nalpha, 200).astype(np.uint8) for _ in range(4)]
        seqs[1] = np.where(rng.random(200) < 0.2, nalpha - 1, seqs[1]).astype(np.uint8)
        seqs[2] = np.where(rng.random(200) < 0.1, nalpha, seqs[2]).astype(np.uint8)
        seqs[3] = np.where(rng.random(200) < 0.1, 255, seqs[3]).astype(np.uint8)
        seqs.append(np.full(200, nalpha - 1, np.uint8))                 # the largest word, 200 - 2 width + 1 times
        seqs.append(np.full(200, nalpha, np.uint8))                     # no word at all
        _, cnt = check(ctx, seqs, PROTEIN, k, 0, nalpha, tab[:nalpha + 1], seed)
        full = 200 - 2 * ks.width_of(k, seed) + 1
        T = [int(cnt[kmerlib.elem(0, j), 2]) for j in range(1, 6)]
        assert T[0] == full and 0 < T[1] < full and 0 < T[2] < full and T[3] == full and T[4] == 0
        # a table that ends before the class nalpha - 1: those residues break the word like any unknown code
        _, short = check(ctx, seqs, PROTEIN, k, 0, nalpha, tab[:nalpha - 1], seed)
        assert short[kmerlib.elem(0, 4), 2] == 0 and short[kmerlib.elem(0, 1), 2] < full
        w, c, t = ks.profile(seqs[4], tab, nalpha, k, seed)
        assert list(w) == [nalpha ** len(ks.offsets(k, seed)) - 1] and list(c) == [full]


def test_extreme_words(ctx):
    """the largest word of every alphabet at the largest weight it allows: 4^15 - 1, 14^8 - 1 (a word of 8 over 14 classes needs the
    seed string: the continuous seed stops at k = 7, 14^8 <= 2^32 < 14^9), 14^7 - 1, 6^12 - 1 ... and duplicate-rich lists over two
    classes"""
    rng = np.random.default_rng(9)
    ident = np.arange(256).astype(np.uint8)
    for molc, nalpha, k, seed in ((DNA, 4, 0, "1" * 15), (DNA, 4, 0, "1" + "01" * 14), (PROTEIN, 14, 0, "1" * 8), (PROTEIN, 14, 7, None),
                                  (PROTEIN, 6, 11, None), (PROTEIN, 20, 0, "1001011011")):
        wt = len(ks.offsets(ks.resolve(molc, k)[0], seed))
        top = nalpha - 1
        if molc == DNA:
            classes = None
            enc = np.array([2, 3, 5, 9], np.uint8)
        else:
            classes, enc = ident[:nalpha], np.arange(nalpha).astype(np.uint8)
        seqs = [np.full(300, enc[top], np.uint8), np.full(200, enc[top], np.uint8), np.full(250, enc[0], np.uint8),
                np.concatenate([np.full(150, enc[0], np.uint8), np.full(150, enc[top], np.uint8)]), enc[rng.integers(0, nalpha, 400)]]
        tab = ks.table(classes, molc)
        w, c, T = ks.profile(seqs[0], tab, nalpha, ks.resolve(molc, k)[0], seed)
        assert list(w) == [nalpha ** wt - 1] and list(c) == [T] and T == 300 - 2 * ks.width_of(k, seed) + 1
        d, cnt = check(ctx, seqs, molc, k, 0, nalpha, classes, seed)
        assert cnt[kmerlib.elem(0, 1), 0] == 200 - 2 * ks.width_of(k, seed) + 1 and d[kmerlib.elem(0, 1)] == 0.
        assert cnt[kmerlib.elem(0, 2), 0] == 0 and d[kmerlib.elem(0, 2)] == 100.
    # Nalpha 2: few distinct words, counts above 1 on both sides, so the smaller count matters
    two = guide.kmer_classes("AG|CT", DNA)
    for k, seed in ((5, None), (12, None), (0, "1101"), (0, "1" * 15)):
        seqs = [dna(rng, n) for n in (500, 333, 777, 64, 1500)]
        _, cnt = check(ctx, seqs, DNA, k, 2, 2, two, seed)
        pr = [ks.profile(s, two, 2, ks.resolve(DNA, k)[0], seed) for s in seqs]
        if len(ks.offsets(k, seed)) <= 5:                               # 32 words at most
            both = np.intersect1d(pr[0][0], pr[2][0])
            assert min(p[1].max() for p in pr) > 1 and cnt[kmerlib.elem(0, 2), 0] > len(both) > 0


@pytest.mark.parametrize("words", [1023, 1024, 1025, 4097])
def test_sort_edges_under_a_width_32_seed(ctx, words):
    """the number of word positions around 1024, where the sort size doubles and a thread of the run compaction takes 2 entries, and
    above 4096 (8 entries); the digits reach 31 residues beyond the last word position"""
    rng = np.random.default_rng(words)
    n = words + 2 * 32 - 1
    seqs = family(rng, protein(rng, n, 4), 3, 0.05, lambda r, m: protein(r, m, 4)) + [protein(rng, n + 1, 4), protein(rng, n - 1, 4)]
    seqs[1][n // 2] = X                                                 # invalid positions go behind the words
    _, cnt = check(ctx, seqs, PROTEIN, 4, 0, 14, PAT14, W32)
    assert cnt[kmerlib.elem(0, 2), 1] == words and cnt[kmerlib.elem(0, 1), 2] == words - 4
    two = [dna(rng, n) for _ in range(3)]
    check(ctx, two, DNA, 0, 6, 2, "AG|CT", W32)                         # 16 words at most: long runs


def test_largest_window_and_one_more(ctx):
    """16384 word positions under a width-32 seed: 64 KB of keys, the wave sums, the class table and 16415 digits in LDS; one
    position more is refused and the sequence named"""
    rng = np.random.default_rng(7)
    W = kmerlib.MAX_WINDOW
    n = W + 2 * 32 - 1
    a = protein(rng, n, 20)
    b = a.copy()
    b[rng.random(n) < 0.01] = 3
    c = protein(rng, n, 2)
    c[::997] = X
    _, cnt = check(ctx, [a, b, c, a[:300]], PROTEIN, 4, 0, 14, PAT14, W32)
    assert cnt[0, 1] == W and cnt[0, 2] == W and 0 < cnt[0, 0] < W
    with pytest.raises(G2GError, match="sequence 1 has 16385 word positions"):
        guide.kmer_distance_spec(ctx, [a, np.append(b, b[:1]), c], PROTEIN, 4, 0, 14, PAT14, W32)
    inside = (np.concatenate([b[:9], b, b[:9]]), 9, 9 + n)              # the window counts, not the buffer
    check(ctx, [a, inside], PROTEIN, 4, 0, 14, PAT14, W32)
    k = 7                                                               # and the continuous seed over 14 classes at its largest k
    check(ctx, [a[:W + 2 * k - 1], b[:W + 2 * k - 1], c[:500]], PROTEIN, k, 2, 14, PAT14)


def test_left_right_inside_a_longer_buffer(ctx):
    rng = np.random.default_rng(23)
    fam = family(rng, protein(rng, 400), 5, 0.05, protein)
    buf = [(np.concatenate([protein(rng, 17 * i), s, protein(rng, 40 - 7 * i)]), 17 * i, 17 * i + len(s)) for i, s in enumerate(fam)]
    for seed in (None, "110101"):
        d, cnt = check(ctx, buf, PROTEIN, 4, 2, 14, PAT14, seed)
        d0, cnt0 = check(ctx, fam, PROTEIN, 4, 2, 14, PAT14, seed)
        assert np.array_equal(cnt, cnt0) and same_bits(d, d0)
        sub = [(s, 30, 330) for s in fam]
        _, cnt1 = check(ctx, sub, PROTEIN, 4, 2, 14, PAT14, seed)
        assert (cnt1[:, 1] == 300 - 2 * ks.width_of(4, seed) + 1).all() and not np.array_equal(cnt1, cnt0)
        check(ctx, [(fam[0], 10, 10), (fam[1], 400, 400), fam[2]], PROTEIN, 4, 2, 14, PAT14, seed)     # empty ranges


def test_pair_list_form(ctx):
    """(j, i) beside (i, j), repeats, (i, i), a wordless member: the pair list equals the all-pairs entries"""
    rng = np.random.default_rng(21)
    seqs = family(rng, protein(rng, 300), 7, 0.1, protein) + [protein(rng, 2000, 4), protein(rng, 12), protein(rng, 7)]
    n = len(seqs)
    ia = [0, 1, 0, 0, 3, 3, 7, 2, 8, 9, 9, 7, 6] + list(rng.integers(0, n, 40))
    ib = [1, 0, 1, 1, 3, 4, 2, 7, 8, 9, 0, 7, 6] + list(rng.integers(0, n, 40))
    args = (PROTEIN, 4, 2, 14, PAT14, "1011")
    d, cnt = check(ctx, seqs, *args, ia, ib)
    assert list(cnt[0]) == [cnt[1][0], cnt[1][2], cnt[1][1]] and list(cnt[2]) == list(cnt[0]) == list(cnt[3])
    assert d[4] == 0. and cnt[4][0] == cnt[4][1] == cnt[4][2] == 300 - 7          # qdiv(a, a)
    assert np.isnan(d[9]) and list(cnt[9]) == [0, 0, 0]                # a wordless member with itself
    all_d, all_c = guide.kmer_distance_spec(ctx, seqs, *args, want_counts=True)
    for p, (a, b) in enumerate(zip(ia, ib)):
        if a != b:
            e = kmerlib.elem(int(a), int(b))
            assert sorted(cnt[p][1:]) == sorted(all_c[e][1:]) and cnt[p][0] == all_c[e][0] and same_bits(d[p:p + 1], all_d[e:e + 1])
    with pytest.raises(G2GError, match="pair 1"):
        guide.kmer_distance_spec(ctx, seqs, *args, [0, n], [1, 1])


@pytest.mark.parametrize("name", ["prot24_a14_k4_seed1011_qpamd", "prot24_a6_k8_qpamd", "dna24_seed13_default"])
def test_guide_tree_of_the_fixtures(ctx, name):
    g = dict(FIX)[name]
    c = ks.case(g)
    seqs = ks.split(g)
    dist = guide.kmer_distance_spec(ctx, seqs, **c)
    assert not np.isnan(dist).any()
    t = KTree.from_dist(dist, with_weights=False)
    r = ktreelib.tree_from_dist(ks.distance(seqs, **c)[0])
    assert list(t.left) == list(r["left"]) and list(t.right) == list(r["right"]) and list(t.parent) == list(r["parent"])
    assert np.array_equal(bits(t.height), bits(r["height"])) and np.array_equal(bits(t.length), bits(r["length"]))
    assert t.n_leaves == len(g["lens"])


def test_timing_option(ctx):
    rng = np.random.default_rng(31)
    ctx.set_option("KMER_TIMING", 1)
    try:
        check(ctx, family(rng, protein(rng, 200), 5, 0.1, protein), PROTEIN, 4, -1, 14, PAT14, "1011")
        assert float(ctx.get_option("KMER_PROFILE_MS")) > 0 and float(ctx.get_option("KMER_PAIRS_MS")) > 0
    finally:
        ctx.set_option("KMER_TIMING", None)
