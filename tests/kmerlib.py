"""The reference's k-mer composition distance restated in plain Python -- calcdist_kmer (src/qdiv.cc:245-282): the words of
Kcomp::makeHash with the continuous seed (qdiv.cc:61-80, src/bitpat.cc:168-185), the sorted (word, count) profile, qdiv
(qdiv.cc:179-232, many == 1) with the seven DistMes closed forms (src/aln.h:54, src/divseq.cc:107-139), 100 x as kcmp_main stores
it.  It plays the role for g2g_kmer_dist_batch that tests/ktreelib.py plays for the tree: tools/make_kmer_golden.py checks it
against the reference itself, the tests check the library against it.

Integers come from numpy, doubles from Python floats and math.log (the C library's log, as the library's host code calls it; numpy's
vectorised log is another implementation)."""
import glob
import math
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmer")
PROTEIN, DNA = 1, 2
QFdiv, QFidn, QCdiv, QCidn, QJuCa, Qpamd, NJuCa = range(7)            # DistMes
OUTOFRANGE = 1024
MAX_WINDOW = 16384                                                    # G2G_KMER_MAX_WINDOW
NAN = float("nan")


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def elem(i, j):
    return j * (j - 1) // 2 + i if i < j else i * (i - 1) // 2 + j


def defaults(molc, k=0, measure=-1):
    """def_wcp_aa / def_wcp_nc, qdiv.cc:32-33"""
    return (k or (5 if molc == PROTEIN else 10)), (measure if measure != -1 else (Qpamd if molc == PROTEIN else QJuCa))


def digits(codes, molc):
    """the class of every residue, -1 where it is not elementary (ALA 3 .. VAL 22; A 2, C 3, G 5, T 9)"""
    tab = np.full(256, -1, np.int64)
    if molc == PROTEIN:
        tab[3:23] = np.arange(20)
    else:
        tab[[2, 3, 5, 9]] = np.arange(4)
    return tab[np.asarray(codes, np.uint8)]


def n_positions(n, k):
    return max(0, n - 2 * k + 1)


def profile(codes, molc, k, left=0, right=None):
    """(words sorted ascending, their counts, T): the scan reads left .. right - k - 1; a word is counted where the last k
    residues read were all elementary"""
    right = len(codes) if right is None else right
    d = digits(codes[left:right], molc)
    W = n_positions(right - left, k)
    if W == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    nalpha = 20 if molc == PROTEIN else 4
    word = np.zeros(W, np.int64)
    ok = np.ones(W, bool)
    for q in range(k):
        dq = d[q:q + W]
        ok &= dq >= 0
        word = word * nalpha + np.maximum(dq, 0)
    w, c = np.unique(word[ok], return_counts=True)
    return w, c.astype(np.int64), int(ok.sum())


def profile_scalar(codes, molc, k, left=0, right=None):
    """the same, the way Bitpat_wq does it: one residue at a time, a flaw restarts the word"""
    right = len(codes) if right is None else right
    nalpha = 20 if molc == PROTEIN else 4
    d = digits(codes, molc)
    cnt = {}
    good = 0
    queue = 0
    for p in range(left, right - k):
        if d[p] < 0:
            good, queue = 0, 0
            continue
        queue = (queue * nalpha + int(d[p])) % nalpha ** k
        good += 1
        if good >= k:
            cnt[queue] = cnt.get(queue, 0) + 1
    ws = sorted(cnt)
    return np.array(ws, np.int64), np.array([cnt[w] for w in ws], np.int64), sum(cnt.values())


def shared(pa, pb):
    """s, Ta, Tb of a pair of profiles"""
    _, xa, xb = np.intersect1d(pa[0], pb[0], assume_unique=True, return_indices=True)
    return int(np.minimum(pa[1][xa], pb[1][xb]).sum()), pa[2], pb[2]


def jukcan(nid):
    if nid <= 0.:
        return 0.
    nid = 1. - 4. / 3. * nid
    if nid <= 0.:
        return float(OUTOFRANGE)
    return -3. / 4. * math.log(nid)


def jukcanpro(nid):
    if nid <= 0.:
        return 0.
    nid = 1. - 20. / 19. * nid
    if nid <= 0.:
        return float(OUTOFRANGE)
    return -19. / 20. * math.log(nid)


def pamcorrect(x):
    if x <= 0:
        return 0.
    return 100. * x


def inner_log_argument(s, ta, tb, measure):
    """the argument of the logarithm jukcan / jukcanpro take, or None where the measure has none or the pair is out of range"""
    if min(ta, tb) == 0 or measure not in (QJuCa, NJuCa):
        return None
    f = float(s) / min(float(ta), float(tb))
    if measure == QJuCa:
        f = 0.18704 * math.log((0.00501 + f) / (0.00501 + 1.)) + 1.
    d = 1. - f
    if d <= 0.:
        return None
    a = 1. - (4. / 3. if measure == NJuCa else 20. / 19.) * d
    return a if a > 0. else None


def qdiv(s, ta, tb, measure):
    m = min(float(ta), float(tb))
    f = float(s) / m if m else NAN                                    # 0 / 0 in C; the NaN goes through every branch below
    d = 1. - f
    if measure == QFdiv:
        return d
    if measure == QFidn:
        return f
    if measure == NJuCa:
        return jukcan(d)
    f = 0.18704 * math.log((0.00501 + f) / (0.00501 + 1.)) + 1.
    d = 1. - f
    if measure == QCidn:
        return f
    if measure == QJuCa:
        return jukcanpro(d)
    if measure == Qpamd:
        return pamcorrect(d) / 100.
    return d


def dist_from_counts(counts, molc, k=0, measure=-1):
    _, measure = defaults(molc, k, measure)
    return np.array([100. * qdiv(int(c[0]), int(c[1]), int(c[2]), measure) for c in np.asarray(counts).reshape(-1, 3)], np.float64)


def _window(s):
    return s if isinstance(s, tuple) else (s, 0, None)


def counts_pairs(seqs, molc, k=0, ia=None, ib=None):
    """int32[npairs, 3] = s, Ta, Tb: all pairs in elem() order, or the index pairs"""
    k, _ = defaults(molc, k)
    prof = [profile(c, molc, k, l, r) for c, l, r in map(_window, seqs)]
    if ia is None:
        pairs = [(i, j) for j in range(len(seqs)) for i in range(j)]
    else:
        pairs = list(zip(map(int, ia), map(int, ib)))
    return np.array([shared(prof[a], prof[b]) for a, b in pairs], np.int32).reshape(-1, 3)


def distance(seqs, molc, k=0, measure=-1, ia=None, ib=None):
    """(dist, counts) as prrn_aln_amd.guide.kmer_distance(..., want_counts=True) returns them"""
    cnt = counts_pairs(seqs, molc, k, ia, ib)
    return dist_from_counts(cnt, molc, k, measure), cnt


def split(g):
    """the members of a fixture"""
    at = np.concatenate([[0], np.cumsum(g["lens"])])
    return [np.ascontiguousarray(g["codes"][at[i]:at[i + 1]]) for i in range(len(g["lens"]))]


def fixtures():
    out = []
    for f in sorted(glob.glob(os.path.join(GOLD, "*.npz"))):
        g = dict(np.load(f))
        out.append((os.path.splitext(os.path.basename(f))[0], g))
    return out


def close_to_reference(got, want):
    """the comparison with the reference's doubles: NaN and OUTOFRANGE positions equal, elsewhere 1e-9 relative (the C library's
    log on another machine, nothing else)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    oor = 100. * OUTOFRANGE
    if not np.array_equal(got == oor, want == oor):
        return False
    m = ~np.isnan(want)
    return bool(np.all(np.abs(got[m] - want[m]) <= 1e-9 * np.maximum(1., np.abs(want[m]))))
