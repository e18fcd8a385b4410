"""The reference's k-mer composition distance over a reduced alphabet and under a spaced seed, restated in plain Python: what
calcdist_kmer (src/qdiv.cc:245-282) computes once setqdiv(k, ap, bp, dm) (qdiv.cc:36-43) has been given a classification ap, a
seed bp, and WCPRM::Nalpha has been set.  tests/kmerlib.py is the corner of it with the full alphabet and the continuous seed;
this module plays the same role for g2g_kmer_dist_batch_spec: tools/make_kmer_spec_golden.py checks it against the reference
itself, the tests check the library against it.

  classes  ReducWord::ReducWord (src/bitpat.cc:78-86): in a pattern such as A|C|D|EQ|FY|... every non-letter starts the next class
           and a letter's residue code gets the current one.  A class >= nalpha breaks a word (Bitpat_wq::good), and so does a
           code the table does not hold.
  seed     None: the continuous seed of k.  Else a string of '1' / '0' (Bitpat::Bitpat, Bitpat_wq::word / flaw, bitpat.cc:99-131,
           168-202) of width len(seed): the scan reads left .. right - width - 1 (Kcomp::makeHash, qdiv.cc:61-80); after residue
           p >= left + width - 1 the word is the base-nalpha number of the classes at p - width + 1 + o, o the offsets of the '1's
           left to right, counted iff all of them are < nalpha.
  qdiv     qdiv.cc:202-231 with the row of param that (Nalpha, Ktuple) selects -- Ktuple, not the seed's weight.

Integers come from numpy, doubles from Python floats and math.log, as in kmerlib."""
import glob
import math
import os

import numpy as np

import kmerlib
from kmerlib import DNA, NAN, PROTEIN, QCidn, QFdiv, QFidn, QJuCa, Qpamd, NJuCa, bits, close_to_reference, elem, split  # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kmer_spec")
D420 = (0.18704, 0.00501)
PARAM = {(14, 3): (0.92042, 0.18677), (14, 4): (0.34576, 0.07108), (14, 5): (0.22333, 0.03164)}      # d314 d414 d514, qdiv.cc:181-186
BAD = 0xFF
# residue codes, src/cmn.h:110-112
CODE = {PROTEIN: dict({c: 3 + i for i, c in enumerate("ARNDCQEGHILKMFPSTWYV")}, X=2, B=23, Z=24),
        DNA: dict({c: 2 + i for i, c in enumerate("ACMGRSVTWYHKDBN")}, U=9)}


def classes_from_pattern(pattern, molc):
    """uint8[256]; codes no letter of the pattern names are BAD"""
    tab = np.full(256, BAD, np.uint8)
    cls = 0
    for ch in pattern:
        if not ch.isalpha():
            cls += 1
        elif ch.upper() in CODE[molc]:
            tab[CODE[molc][ch.upper()]] = cls
    return tab


def full_classes(molc):
    d = kmerlib.digits(np.arange(256), molc)
    return np.where(d < 0, BAD, d).astype(np.uint8)


def table(classes, molc):
    """classes: None (the full alphabet), a pattern string or a table of up to 256 entries -> uint8[256]"""
    if classes is None:
        return full_classes(molc)
    if isinstance(classes, str):
        return classes_from_pattern(classes, molc)
    tab = np.full(256, BAD, np.uint8)
    tab[:len(classes)] = classes
    return tab


def resolve(molc, k=0, measure=-1, nalpha=0):
    k, measure = kmerlib.defaults(molc, k, measure)
    return k, measure, (nalpha or (20 if molc == PROTEIN else 4))


def offsets(k, seed):
    return list(range(k)) if seed is None else [o for o, ch in enumerate(seed) if ch == "1"]


def width_of(k, seed):
    return k if seed is None else len(seed)


def n_positions(n, width):
    return max(0, n - 2 * width + 1)


def profile(codes, tab, nalpha, k, seed=None, left=0, right=None):
    """(words ascending, counts, T) of the window left .. right - 1"""
    right = len(codes) if right is None else right
    width = width_of(k, seed)
    W = n_positions(right - left, width)
    if W == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    c = tab[np.asarray(codes[left:right], np.uint8)].astype(np.int64)
    word = np.zeros(W, np.int64)
    ok = np.ones(W, bool)
    for o in offsets(k, seed):
        d = c[o:o + W]
        ok &= d < nalpha
        word = word * nalpha + np.where(d < nalpha, d, 0)
    w, n = np.unique(word[ok], return_counts=True)
    return w, n.astype(np.int64), int(ok.sum())


def profile_scalar(codes, tab, nalpha, k, seed=None, left=0, right=None):
    """the same the way Bitpat_wq does it, one residue at a time: a ring of the last width classes, BAD_RES where a residue was
    no good; the continuous seed keeps a 32-bit queue modulo nalpha^k and restarts at a flaw"""
    right = len(codes) if right is None else right
    width = width_of(k, seed)
    cnt = {}
    if seed is None:
        good = queue = 0
        for p in range(left, right - width):
            c = int(tab[codes[p]])
            if c >= nalpha:
                good = queue = 0
                continue
            queue = ((queue * nalpha + c) & 0xFFFFFFFF) % nalpha ** k
            good += 1
            if good >= k:
                cnt[queue] = cnt.get(queue, 0) + 1
    else:
        ring, qp, exam = [BAD] * width, 0, offsets(k, seed)
        for p in range(left, right - width):
            c = int(tab[codes[p]])
            ring[qp] = c if c < nalpha else BAD
            qp = (qp + 1) % width
            if c >= nalpha:
                continue                                              # makeHash calls flaw(), not word()
            w = 0
            for o in exam:
                d = ring[(qp + o) % width]
                if d == BAD:
                    w = None
                    break
                w = w * nalpha + d
            if w is not None:
                cnt[w] = cnt.get(w, 0) + 1
    ws = sorted(cnt)
    return np.array(ws, np.int64), np.array([cnt[w] for w in ws], np.int64), sum(cnt.values())


def row(nalpha, k):
    return PARAM.get((nalpha, k), D420)


def qdiv(s, ta, tb, measure, p0, p1):
    m = min(float(ta), float(tb))
    f = float(s) / m if m else NAN
    d = 1. - f
    if measure == QFdiv:
        return d
    if measure == QFidn:
        return f
    if measure == NJuCa:
        return kmerlib.jukcan(d)
    f = p0 * math.log((p1 + f) / (p1 + 1.)) + 1.
    d = 1. - f
    if measure == QCidn:
        return f
    if measure == QJuCa:
        return kmerlib.jukcanpro(d)
    if measure == Qpamd:
        return kmerlib.pamcorrect(d) / 100.
    return d


def log_arguments(s, ta, tb, measure, p0, p1):
    """the arguments of the logarithms a pair's distance takes: the fit's, and the one of jukcan / jukcanpro where the pair is in
    range"""
    out = []
    if min(ta, tb) == 0:
        return out
    f = float(s) / min(float(ta), float(tb))
    if measure in (QFdiv, QFidn):
        return out
    if measure != NJuCa:
        out.append((p1 + f) / (p1 + 1.))
        f = p0 * math.log((p1 + f) / (p1 + 1.)) + 1.
    d = 1. - f
    if measure in (QJuCa, NJuCa) and d > 0.:
        a = 1. - (4. / 3. if measure == NJuCa else 20. / 19.) * d
        if a > 0.:
            out.append(a)
    return out


def dist_from_counts(counts, molc, k=0, measure=-1, nalpha=0, seed=None):
    k, measure, nalpha = resolve(molc, k, measure, nalpha)
    p0, p1 = row(nalpha, k)
    return np.array([100. * qdiv(int(c[0]), int(c[1]), int(c[2]), measure, p0, p1) for c in np.asarray(counts).reshape(-1, 3)], np.float64)


def _window(s):
    return s if isinstance(s, tuple) else (s, 0, None)


def counts_pairs(seqs, molc, k=0, nalpha=0, classes=None, seed=None, ia=None, ib=None):
    """int32[npairs, 3] = s, Ta, Tb: all pairs in elem() order, or the index pairs"""
    k, _, nalpha = resolve(molc, k, -1, nalpha)
    tab = table(classes, molc)
    prof = [profile(c, tab, nalpha, k, seed, l, r) for c, l, r in map(_window, seqs)]
    if ia is None:
        pairs = [(i, j) for j in range(len(seqs)) for i in range(j)]
    else:
        pairs = list(zip(map(int, ia), map(int, ib)))
    return np.array([kmerlib.shared(prof[a], prof[b]) for a, b in pairs], np.int32).reshape(-1, 3)


def distance(seqs, molc, k=0, measure=-1, nalpha=0, classes=None, seed=None, ia=None, ib=None):
    """(dist, counts) as prrn_aln_amd.guide.kmer_distance_spec(..., want_counts=True) returns them"""
    cnt = counts_pairs(seqs, molc, k, nalpha, classes, seed, ia, ib)
    return dist_from_counts(cnt, molc, k, measure, nalpha, seed), cnt


def case(g):
    """the arguments a fixture records: molc, k, measure, nalpha, pattern, seed (None where it has none)"""
    return dict(molc=int(g["molc"][0]), k=int(g["k"][0]), measure=int(g["measure"][0]), nalpha=int(g["nalpha"][0]),
                classes=str(g["pattern"][0]), seed=str(g["seed"][0]) or None)


def fixtures():
    out = []
    for f in sorted(glob.glob(os.path.join(GOLD, "*.npz"))):
        out.append((os.path.splitext(os.path.basename(f))[0], dict(np.load(f))))
    return out
