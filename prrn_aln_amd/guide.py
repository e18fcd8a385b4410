"""The guide-tree stage on the GPU: pairwise alignment-score distances between the single
sequences of a family, as the reference's dpscore() computes them (src/phyl.cc:222-252):

    scr1[i]   = selfAlnScr(seq i)                                   (src/aln2.cc:54-64)
    score     = alnScoreD(seq i, seq j)                             (src/fwd2d1.cc:324-338 -> Fwd2d::forwardD)  <- the GPU part
    dist[i,j] = 100 * (1 - (score + u * |len_i - len_j| / 2) / sqrt(scr1[i] * scr1[j]))   (alnscore2dist, src/aln2.cc:325-333)

All DPs of the N (N - 1) / 2 pairs go to the device as ONE batch (g2g_alnscored_batch: the sequences are uploaded once, a
pair is two indices).  For families too large for one DP per pair, kmer_distance gives the reference's k-mer composition
distance (calcdist_kmer, src/qdiv.cc:245-282) in the same layout.  progressive / align_sequences (at the end) take the guide tree
of either to the first MSA.  There is no CPU fallback: without libg2g.so / a GPU the calls raise."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Sequence, Tuple

import numpy as np

from . import _abi
from ._lib import G2GError, last_error, lib


def self_score(codes: np.ndarray, simmtx: np.ndarray) -> float:
    """selfAlnScr of a single sequence: the diagonal entries summed in sequence order"""
    c = np.asarray(codes, np.intp)
    if len(c) == 0:
        return 0.0
    return float(np.cumsum(simmtx[c, c])[-1])          # cumsum adds left to right, like the reference's loop


def scores_to_dist(scores: np.ndarray, ia: Sequence[int], ib: Sequence[int], lens: Sequence[int], selfs: np.ndarray, u: float) -> np.ndarray:
    """alnscore2dist for the global mode with dpscore's denominator; returns 1 - score / denominator (dpscore stores 100 x)"""
    lens = np.asarray(lens, np.int64)
    ia = np.asarray(ia, np.intp); ib = np.asarray(ib, np.intp)
    dlen = np.abs(lens[ia] - lens[ib]).astype(np.float32)
    corr = (np.float32(u) * dlen / np.float32(2)).astype(np.float64)       # float arithmetic in the reference (alprm.u is a float)
    denome = np.sqrt(selfs[ia] * selfs[ib])
    return 1.0 - (np.asarray(scores, np.float64) + corr) / denome


def all_pairs(n: int) -> Tuple[np.ndarray, np.ndarray]:
    ia, ib = np.triu_indices(n, 1)
    return ia.astype(np.int32), ib.astype(np.int32)


def alnscored_batch(ctx, prm: "_abi.Params", seqs: Sequence[np.ndarray], ia: Sequence[int], ib: Sequence[int]):
    """alnScoreD for every index pair: (scores float64[npairs], status int32[npairs])"""
    L = lib()
    ds = (_abi.DSeq * len(seqs))()
    keep = []
    for k, s in enumerate(seqs):
        x = np.ascontiguousarray(s, np.uint8)
        keep.append(x)
        ds[k].res = x.ctypes.data_as(_abi.c_u8p)
        ds[k].len, ds[k].left, ds[k].right = len(x), 0, len(x)
    ia = np.ascontiguousarray(ia, np.int32); ib = np.ascontiguousarray(ib, np.int32)
    out = np.zeros(len(ia), np.float64)
    st = np.zeros(len(ia), np.int32)
    rc = L.g2g_alnscored_batch(ctx._h, C.byref(prm), len(seqs), ds, len(ia), ia.ctypes.data_as(C.POINTER(C.c_int32)),
                               ib.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(_abi.c_f64p), st.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise G2GError("g2g_alnscored_batch rc=%d: %s" % (rc, last_error()))
    return out, st


def msa_divergence(ctx, codes: np.ndarray):
    """g2g_msa_divergence: the divergence of every pair of members of an MSA ((len, many) uint8 codes, <= 1 = gap) as the
    reference's calcdistseq / pairdvn computes it (src/phyl.cc:344-385, src/divseq.cc:33-63) -- the distances its weighting tree
    is built from.  Returns (dist float64[npairs], counts int32[npairs, 4] = matched, mismatched, unpaired, gaps); pair (i < j)
    is entry j (j - 1) / 2 + i."""
    codes = np.ascontiguousarray(codes, np.uint8)
    if codes.ndim != 2:
        raise ValueError("codes must be (len, many)")
    ln, many = codes.shape
    npairs = max(many * (many - 1) // 2, 0)
    dist = np.zeros(npairs, np.float64)
    counts = np.zeros((npairs, 4), np.int32)
    rc = lib().g2g_msa_divergence(ctx._h, many, ln, codes.ctypes.data_as(_abi.c_u8p), dist.ctypes.data_as(_abi.c_f64p),
                                  counts.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise G2GError("g2g_msa_divergence rc=%d: %s" % (rc, last_error()))
    return dist, counts


def msa_divergence_groups(ctx, codes: np.ndarray, groups):
    """g2g_msa_divergence_groups: the divergence of every pair of GROUPS of members of an MSA as the group form of the reference's
    pairdvn computes it (src/divseq.cc:65-105) -- the distances the weighting tree over the groups is built from.  groups: one
    sequence of member indices per group, together a partition of the members; the order inside a group is significant.  Returns
    (dist float64[npairs], counts int32[npairs, 4]); group pair (k < l) is entry l (l - 1) / 2 + k."""
    codes = np.ascontiguousarray(codes, np.uint8)
    if codes.ndim != 2:
        raise ValueError("codes must be (len, many)")
    ln, many = codes.shape
    ss, keep = _subset_struct(groups)
    npairs = max(len(groups) * (len(groups) - 1) // 2, 0)
    dist = np.zeros(npairs, np.float64)
    counts = np.zeros((npairs, 4), np.int32)
    rc = lib().g2g_msa_divergence_groups(None if ctx is None else ctx._h, many, ln, codes.ctypes.data_as(_abi.c_u8p), C.byref(ss),
                                         dist.ctypes.data_as(_abi.c_f64p), counts.ctypes.data_as(C.POINTER(C.c_int32)))
    del keep
    if rc != 0:
        raise G2GError("g2g_msa_divergence_groups rc=%d: %s" % (rc, last_error()))
    return dist, counts


def _kmer_params(molc: int, k: int, measure: int) -> "_abi.KmerParams":
    kp = _abi.KmerParams()
    kp.molc, kp.k, kp.measure, kp.reserved = int(molc), int(k), int(measure), 0
    return kp


def kmer_dist_from_counts(counts: np.ndarray, molc: int, k: int = 0, measure: int = -1) -> np.ndarray:
    """g2g_kmer_dist_from_counts (host only): 100 x qdiv from the three integers (s, Ta, Tb) of each pair, the reference's
    closed forms in its operation order (src/qdiv.cc:202-231, 239)"""
    cnt = np.ascontiguousarray(counts, np.int32).reshape(-1, 3)
    dist = np.zeros(len(cnt), np.float64)
    kp = _kmer_params(molc, k, measure)
    rc = lib().g2g_kmer_dist_from_counts(C.byref(kp), len(cnt), cnt.ctypes.data_as(C.POINTER(C.c_int32)), dist.ctypes.data_as(_abi.c_f64p))
    if rc != 0:
        raise G2GError("g2g_kmer_dist_from_counts rc=%d: %s" % (rc, last_error()))
    return dist


def kmer_distance(ctx, seqs: Sequence, molc: int, k: int = 0, measure: int = -1, ia=None, ib=None, want_counts: bool = False):
    """g2g_kmer_dist_batch: the k-mer composition distance of the reference's calcdist_kmer (src/qdiv.cc:245-282), 100 x qdiv,
    between unaligned single sequences -- all pairs (pair (i < j) is entry j (j - 1) / 2 + i, the layout KTree.from_dist takes:
    the guide tree is KTree.from_dist(dist, with_weights=False)) or the index pairs (ia, ib).  k = 0 / measure = -1: the
    reference's defaults (protein k 5 with Qpamd, DNA k 10 with QJuCa).  A sequence is an array of residue codes, or a tuple
    (codes, left, right) for a range inside a longer buffer.  With want_counts: (dist, counts int32[npairs, 3] = s, Ta, Tb)."""
    return _kmer_batch(lib().g2g_kmer_dist_batch, ctx, _kmer_params(molc, k, measure), seqs, ia, ib, want_counts)


def _kmer_batch(entry, ctx, kp, seqs: Sequence, ia, ib, want_counts: bool):
    """the call both k-mer entries share: entry is the library function, kp its parameter structure"""
    if (ia is None) != (ib is None):
        raise ValueError("ia and ib come together")
    ds = (_abi.DSeq * max(len(seqs), 1))()
    keep = []
    for n, s in enumerate(seqs):
        s, left, right = s if isinstance(s, tuple) else (s, 0, None)
        x = np.ascontiguousarray(s, np.uint8)
        keep.append(x)
        ds[n].res = x.ctypes.data_as(_abi.c_u8p)
        ds[n].len, ds[n].left, ds[n].right = len(x), left, len(x) if right is None else right
    nseq = len(seqs)
    if ia is None:
        npairs = max(nseq * (nseq - 1) // 2, 0)
        pa = pb = None
    else:
        ia = np.ascontiguousarray(ia, np.int32); ib = np.ascontiguousarray(ib, np.int32)
        if ia.shape != ib.shape or ia.ndim != 1:
            raise ValueError("ia and ib are two index vectors of one length")
        npairs = len(ia)
        pa, pb = ia.ctypes.data_as(C.POINTER(C.c_int32)), ib.ctypes.data_as(C.POINTER(C.c_int32))
    dist = np.zeros(npairs, np.float64)
    counts = np.zeros((npairs, 3), np.int32)
    rc = entry(ctx._h, C.byref(kp), nseq, ds, npairs, pa, pb, dist.ctypes.data_as(_abi.c_f64p),
               counts.ctypes.data_as(C.POINTER(C.c_int32)) if want_counts else None)
    if rc != 0:
        raise G2GError("%s rc=%d: %s" % (entry.__name__, rc, last_error()))
    return (dist, counts) if want_counts else dist


def kmer_classes(pattern: str, molc: int) -> np.ndarray:
    """uint8[256] class table of a -A style classification such as "A|C|D|EQ|FY|..." (ReducWord::ReducWord, src/bitpat.cc:78-86):
    every non-letter starts the next class; a letter's residue code (the encoding of operator.encode) gets the current class;
    codes no letter names are 0xFF, which breaks a word.  No table is built in: the caller brings the pattern."""
    from .operator import _AA, _NT, PROTEIN
    enc = _AA if molc == PROTEIN else _NT
    tab = np.full(256, 0xFF, np.uint8)
    cls = 0
    for ch in pattern:
        if not ch.isalpha():
            cls += 1
        elif ch.upper() in enc:
            if cls > 0xFF:
                raise ValueError("more than 256 classes")
            tab[enc[ch.upper()]] = cls
    return tab


def _kmer_spec(molc: int, k: int, measure: int, nalpha: int, classes, seed):
    """(g2g_kmer_spec, what it points to)"""
    sp = _abi.KmerSpec()
    sp.molc, sp.k, sp.measure, sp.nalpha, sp.nclasses, sp.reserved = int(molc), int(k), int(measure), int(nalpha), 0, 0
    tab = None
    if classes is not None:
        tab = kmer_classes(classes, molc) if isinstance(classes, str) else np.ascontiguousarray(classes, np.uint8)
        if tab.ndim != 1 or not 1 <= len(tab) <= 256:
            raise ValueError("classes: a pattern string or a table of 1 .. 256 entries")
        sp.classes, sp.nclasses = tab.ctypes.data_as(_abi.c_u8p), len(tab)
    sp.seed = None if seed is None else seed.encode()
    return sp, tab


def kmer_dist_from_counts_spec(counts: np.ndarray, molc: int, k: int = 0, measure: int = -1, nalpha: int = 0, seed=None) -> np.ndarray:
    """g2g_kmer_dist_from_counts_spec (host only): kmer_dist_from_counts with the row of qdiv's fit parameters that belongs to
    (nalpha, k) -- nalpha 14 with k 3 / 4 / 5 has its own; k counts, not the seed's weight"""
    cnt = np.ascontiguousarray(counts, np.int32).reshape(-1, 3)
    dist = np.zeros(len(cnt), np.float64)
    sp, _ = _kmer_spec(molc, k, measure, nalpha, None, seed)
    rc = lib().g2g_kmer_dist_from_counts_spec(C.byref(sp), len(cnt), cnt.ctypes.data_as(C.POINTER(C.c_int32)), dist.ctypes.data_as(_abi.c_f64p))
    if rc != 0:
        raise G2GError("g2g_kmer_dist_from_counts_spec rc=%d: %s" % (rc, last_error()))
    return dist


def kmer_distance_spec(ctx, seqs: Sequence, molc: int, k: int = 0, measure: int = -1, nalpha: int = 0, classes=None, seed=None,
                       ia=None, ib=None, want_counts: bool = False):
    """g2g_kmer_dist_batch_spec: kmer_distance over a reduced alphabet and / or under a spaced seed -- the reference's qdiv with
    -R nalpha, -A classes and -B seed.  classes: a pattern string (kmer_classes) or a table classes[code]; a class >= nalpha breaks
    a word.  seed: a string of '1' / '0' (first and last '1', width <= 32, weight <= 15), None for the continuous seed of k.  The
    fit parameters go by (nalpha, k) even under a seed.  With the defaults it is kmer_distance."""
    sp, keep = _kmer_spec(molc, k, measure, nalpha, classes, seed)
    return _kmer_batch(lib().g2g_kmer_dist_batch_spec, ctx, sp, seqs, ia, ib, want_counts)


def alignb_ng_batch(ctx, prm: "_abi.Params", seqs: Sequence[np.ndarray], ia: Sequence[int], ib: Sequence[int]):
    """alignB_ng for every index pair: [(score, skeleton (n, 2) int32, status)]"""
    L = lib()
    ds = (_abi.DSeq * len(seqs))()
    keep = []
    for k, s in enumerate(seqs):
        x = np.ascontiguousarray(s, np.uint8)
        keep.append(x)
        ds[k].res = x.ctypes.data_as(_abi.c_u8p)
        ds[k].len, ds[k].left, ds[k].right = len(x), 0, len(x)
    ia = np.ascontiguousarray(ia, np.int32); ib = np.ascontiguousarray(ib, np.int32)
    n = len(ia)
    scr = np.zeros(n, np.float64); st = np.zeros(n, np.int32)
    skl = (C.POINTER(_abi.Skl) * max(n, 1))(); nskl = (C.c_int * max(n, 1))()
    rc = L.g2g_alignb_ng_batch(ctx._h, C.byref(prm), len(seqs), ds, n, ia.ctypes.data_as(C.POINTER(C.c_int32)),
                               ib.ctypes.data_as(C.POINTER(C.c_int32)), scr.ctypes.data_as(_abi.c_f64p), skl, nskl,
                               st.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc != 0:
        raise G2GError("g2g_alignb_ng_batch rc=%d: %s" % (rc, last_error()))
    out = []
    for k in range(n):
        a = np.zeros((nskl[k], 2), np.int32)
        if nskl[k] and skl[k]:
            a[:] = np.ctypeslib.as_array(C.cast(skl[k], C.POINTER(C.c_int32)), shape=(nskl[k] * 2,)).reshape(-1, 2)
            L.g2g_free(skl[k])
        out.append((float(scr[k]), a, int(st[k])))
    return out


def distance_matrix(ctx, prm: "_abi.Params", seqs: Sequence[np.ndarray], simmtx: np.ndarray) -> np.ndarray:
    """dpscore over all pairs: the condensed distance vector (pair order of all_pairs), 100 x as the reference stores it"""
    ia, ib = all_pairs(len(seqs))
    scores, st = alnscored_batch(ctx, prm, seqs, ia, ib)
    if (st != 0).any():
        raise G2GError("alnScoreD failed for %d pairs (first status %d)" % (int((st != 0).sum()), int(st[st != 0][0])))
    selfs = np.array([self_score(s, simmtx) for s in seqs])
    return 100.0 * scores_to_dist(scores, ia, ib, [len(s) for s in seqs], selfs, prm.u)


# ---- the conserved regions of an MSA (the step in front of prrn's default refinement) ----------------------------------------------
def _take_ranges(ptr, n) -> np.ndarray:
    out = np.zeros((n, 2), np.int32)
    if n and ptr:
        out[:] = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int32)), shape=(2 * n,)).reshape(-1, 2)
    if ptr:
        lib().g2g_free(ptr)
    return out


def _range_array(r):
    r = np.ascontiguousarray(r, np.int32).reshape(-1, 2)
    buf = (_abi.Range * max(1, len(r)))()
    if len(r):
        C.memmove(buf, r.ctypes.data, r.nbytes)
    return buf, len(r)


def constwo_batch(ctx, pwds: Sequence, thr: float = 35., want_colscore: bool = False):
    """g2g_constwo_batch <-> Ssrel::constwo (reference src/consreg.cc:438-450) on built pairs (operator.PwdM) whose two groups are
    juxtaposed sons of one MSA: [ranges (n, 2) int32] per pair -- columns [left, right) --, with want_colscore
    [(ranges, s float64[len])], s the score of every column.  ctx may be None only to have the arguments checked."""
    L = lib()
    n = len(pwds)
    hs = (C.c_void_p * max(1, n))(*[p._h for p in pwds])
    rng = (C.POINTER(_abi.Range) * max(1, n))()
    nr = (C.c_int * max(1, n))()
    st = (C.c_int * max(1, n))()
    col = (_abi.c_f64p * max(1, n))() if want_colscore else None
    rc = L.g2g_constwo_batch(ctx._h if ctx is not None else None, n, hs, float(thr), rng, nr, col, st)
    if rc != 0:
        raise G2GError("g2g_constwo_batch rc=%d: %s" % (rc, last_error()))
    out = []
    for k in range(n):
        r = _take_ranges(rng[k], nr[k])
        if want_colscore:
            ln = pwds[k].problem.a.len
            s = np.ctypeslib.as_array(col[k], shape=(ln,)).copy()
            L.g2g_free(col[k])
            out.append((r, s))
        else:
            out.append(r)
    return out


def conserved_regions(ctx, codes: np.ndarray, tree, prm: "_abi.Params", thr: float = 35., weight=None, dissim: bool = False) -> np.ndarray:
    """g2g_consreg <-> Ssrel::consreg(msd, dissim) (reference src/consreg.cc:484-518): the columns of an MSA ((len, many) uint8
    codes) that are conserved across EVERY branch of its weighting tree, as ranges (n, 2) int32 of columns [left, right); with
    dissim the complement in [0, len) -- the ranges prrn's default pipeline hands to its refinement.  tree: a refine.KTree /
    anything with left, right, parent (vol / cur are not read).  prm: the reference's localprm -- operator.AlnParam(u=3, v=10, u0=0,
    u1=0, tgapf=1, scale=1, k1=7, ls=2, sh=100, banded=1, simmtx=<the reference's matrix number 1>).to_c()[0]."""
    codes = np.ascontiguousarray(codes, np.uint8)
    if codes.ndim != 2:
        raise ValueError("codes must be (len, many)")
    ln, many = codes.shape
    nn = 2 * many - 1
    arrs = [np.ascontiguousarray(getattr(tree, k), np.int32) for k in ("left", "right", "parent")]
    vol = np.ascontiguousarray(getattr(tree, "vol", None) if getattr(tree, "vol", None) is not None else np.ones(nn), np.float64)
    cur = np.ascontiguousarray(getattr(tree, "cur", None) if getattr(tree, "cur", None) is not None else np.ones(nn), np.float64)
    t = _abi.Tree()
    t.n_nodes = len(arrs[0])
    t.left, t.right, t.parent = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in arrs)
    t.vol, t.cur = vol.ctypes.data_as(_abi.c_f64p), cur.ctypes.data_as(_abi.c_f64p)
    w = None if weight is None else np.ascontiguousarray(weight, np.float64)
    if w is not None and len(w) != many:
        raise ValueError("one weight per member")
    out = C.POINTER(_abi.Range)()
    nout = C.c_int(0)
    rc = lib().g2g_consreg(ctx._h if ctx is not None else None, C.byref(prm), float(thr), many, ln, codes.ctypes.data_as(_abi.c_u8p),
                           None if w is None else w.ctypes.data_as(_abi.c_f64p), C.byref(t), 1 if dissim else 0, C.byref(out), C.byref(nout))
    if rc != 0:
        raise G2GError("g2g_consreg rc=%d: %s" % (rc, last_error()))
    return _take_ranges(out, nout.value)


def ranges_intersect(a, b) -> np.ndarray:
    """g2g_ranges_combine(dissim = 0) <-> cmnrng(a, b, 0) (reference src/css.cc:261-282), host only"""
    ba, na = _range_array(a)
    bb, nb = _range_array(b)
    out = C.POINTER(_abi.Range)()
    nout = C.c_int(0)
    rc = lib().g2g_ranges_combine(ba, na, bb, nb, 0, 0, C.byref(out), C.byref(nout))
    if rc != 0:
        raise G2GError("g2g_ranges_combine rc=%d" % rc)
    return _take_ranges(out, nout.value)


def ranges_complement(a, length: int) -> np.ndarray:
    """g2g_ranges_combine(dissim = 1) <-> complerng (css.cc:313-336) of the ranges a inside [0, length), host only"""
    ba, na = _range_array(a)
    out = C.POINTER(_abi.Range)()
    nout = C.c_int(0)
    rc = lib().g2g_ranges_combine(ba, na, None, 0, 1, int(length), C.byref(out), C.byref(nout))
    if rc != 0:
        raise G2GError("g2g_ranges_combine rc=%d" % rc)
    return _take_ranges(out, nout.value)


# ---- fused groups and the per-range refinement plan (what prrn's default run decides before it refines) -----------------------------
@dataclass
class Relation:
    """A subset and the tree over its groups (the reference's Ssrel: ss + ktree).  groups[g]: int32 members of group g in the
    reference's order; leaf g of the tree is group g; origin[k]: the node of the given tree node k was copied from."""
    fused: bool
    groups: List[np.ndarray]
    left: np.ndarray
    right: np.ndarray
    parent: np.ndarray
    origin: np.ndarray
    vol: np.ndarray
    cur: np.ndarray


@dataclass
class FuseStats:
    tests: int = 0
    fused: int = 0
    launches: int = 0


@dataclass
class RefinePlan:
    """nothing_to_refine: the whole-MSA relation has fewer than two groups.  ranges (n, 2) int32 ascending; at_left / at_right: the
    range touches column 0 / len (where prrn keeps exgl / exgr); relations[i]: the range's own relation over `whole`."""
    nothing_to_refine: bool
    whole: Relation
    ranges: np.ndarray
    at_left: np.ndarray
    at_right: np.ndarray
    relations: List[Relation] = field(default_factory=list)
    stats: FuseStats = field(default_factory=FuseStats)


def _tree_struct(tree):
    arrs = [np.ascontiguousarray(getattr(tree, k), np.int32) for k in ("left", "right", "parent")]
    nn = len(arrs[0])
    vol = np.ascontiguousarray(getattr(tree, "vol", None) if getattr(tree, "vol", None) is not None else np.ones(nn), np.float64)
    cur = np.ascontiguousarray(getattr(tree, "cur", None) if getattr(tree, "cur", None) is not None else np.ones(nn), np.float64)
    if not (len(arrs[1]) == len(arrs[2]) == len(vol) == len(cur) == nn):
        raise ValueError("the tree's arrays must have one length")
    t = _abi.Tree()
    t.n_nodes = nn
    t.left, t.right, t.parent = (a.ctypes.data_as(C.POINTER(C.c_int32)) for a in arrs)
    t.vol, t.cur = vol.ctypes.data_as(_abi.c_f64p), cur.ctypes.data_as(_abi.c_f64p)
    return t, (arrs, vol, cur)


def _subset_struct(groups):
    if groups is None:
        return None, None
    start = np.zeros(len(groups) + 1, np.int32)
    start[1:] = np.cumsum([len(g) for g in groups])
    member = np.ascontiguousarray(np.concatenate([np.asarray(g, np.int32).reshape(-1) for g in groups]) if len(groups) else np.zeros(0, np.int32), np.int32)
    s = _abi.Subset()
    s.num, s.elms = len(groups), len(member)
    s.start, s.member = start.ctypes.data_as(_abi.c_i32p), member.ctypes.data_as(_abi.c_i32p)
    return s, (start, member)


def _msa_args(codes, weight):
    codes = np.ascontiguousarray(codes, np.uint8)
    if codes.ndim != 2:
        raise ValueError("codes must be (len, many)")
    w = None if weight is None else np.ascontiguousarray(weight, np.float64)
    if w is not None and len(w) != codes.shape[1]:
        raise ValueError("one weight per member")
    return codes, w


def _take_relation(r: "_abi.Relation") -> Relation:
    i32 = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).copy() if n and p else np.zeros(0, np.int32)
    f64 = lambda p, n: np.ctypeslib.as_array(p, shape=(n,)).copy() if n and p else np.zeros(0, np.float64)
    start, member = i32(r.ss.start, r.ss.num + 1), i32(r.ss.member, r.ss.elms)
    nn = r.n_nodes
    return Relation(bool(r.fused), [member[start[g]:start[g + 1]].copy() for g in range(r.ss.num)], i32(r.left, nn), i32(r.right, nn),
                    i32(r.parent, nn), i32(r.origin, nn), f64(r.vol, nn), f64(r.cur, nn))


def _relation_struct(rel: Relation):
    """(g2g_relation over numpy arrays, the arrays to keep alive): a Relation on its way back into the library"""
    s, keep_s = _subset_struct(rel.groups)
    arrs = [np.ascontiguousarray(a, np.int32) for a in (rel.left, rel.right, rel.parent, rel.origin)]
    vc = [np.ascontiguousarray(a, np.float64) for a in (rel.vol, rel.cur)]
    r = _abi.Relation()
    r.fused, r.ss, r.n_nodes = int(bool(rel.fused)), s, len(arrs[0])
    r.left, r.right, r.parent, r.origin = (a.ctypes.data_as(_abi.c_i32p) for a in arrs)
    r.vol, r.cur = (a.ctypes.data_as(_abi.c_f64p) for a in vc)
    return r, (keep_s, arrs, vc)


def plan_struct(plan: RefinePlan):
    """(g2g_refine_plan_t over numpy arrays, the arrays to keep alive) of what refine_plan returned, or of a plan made by hand.
    Nothing in it belongs to the library: it is not to be handed to g2g_refine_plan_free."""
    n = len(plan.ranges)
    if len(plan.relations) != n:
        raise ValueError("one relation per range")
    p = _abi.RefinePlan()
    p.status, p.nranges = (1 if plan.nothing_to_refine else 0), n
    p.whole, keep_w = _relation_struct(plan.whole)
    rng = (_abi.Range * max(1, n))(*[_abi.Range(int(l), int(r)) for l, r in np.asarray(plan.ranges, np.int32).reshape(-1, 2)])
    al, ar = (np.ascontiguousarray(a, np.int32) for a in (plan.at_left, plan.at_right))
    if len(al) != n or len(ar) != n:
        raise ValueError("at_left / at_right: one entry per range")
    rels = [_relation_struct(r) for r in plan.relations]
    rr = (_abi.Relation * max(1, n))(*[r for r, _ in rels])
    p.ranges, p.range_rel = C.cast(rng, C.POINTER(_abi.Range)), C.cast(rr, C.POINTER(_abi.Relation))
    p.at_left, p.at_right = al.ctypes.data_as(_abi.c_i32p), ar.ctypes.data_as(_abi.c_i32p)
    p.stats = _abi.FuseStats(plan.stats.tests, plan.stats.fused, plan.stats.launches, 0)
    return p, (keep_w, rng, al, ar, rels, rr)


def may_fuse_batch(ctx, pwds: Sequence, u: float = 3., v: float = 10.) -> Tuple[np.ndarray, np.ndarray]:
    """g2g_mayfuse_batch <-> ConservedT::mayfuse (reference src/consreg.cc:452-464) on built pairs (operator.PwdM) whose two groups
    are juxtaposed sons of one MSA: (fuse int32[n] 0 / 1, stop_col int32[n]: the column at which the walk broke, -1 when fused).
    ctx may be None only to have the arguments checked."""
    n = len(pwds)
    hs = (C.c_void_p * max(1, n))(*[p._h for p in pwds])
    fz = (C.c_int * max(1, n))()
    sc = (C.c_int * max(1, n))()
    st = (C.c_int * max(1, n))()
    rc = lib().g2g_mayfuse_batch(ctx._h if ctx is not None else None, n, hs, float(u), float(v), fz, sc, st)
    if rc != 0:
        raise G2GError("g2g_mayfuse_batch rc=%d: %s" % (rc, last_error()))
    return np.array(fz[:n], np.int32), np.array(sc[:n], np.int32)


def fuse_groups(ctx, codes: np.ndarray, tree, prm: "_abi.Params", groups=None, left: int = 0, right=None, weight=None):
    """g2g_consregss <-> Ssrel::consregss (reference src/consreg.cc:692-711) on the columns [left, right) of an MSA: subtrees of
    `tree` whose two sons are conserved from end to end are fused.  tree: over the groups (`groups`: a list of member lists, None =
    the members themselves).  Returns (Relation, FuseStats); Relation.fused False: nothing fused, the given relation again."""
    codes, w = _msa_args(codes, weight)
    ln, many = codes.shape
    t, keep_t = _tree_struct(tree)
    s, keep_s = _subset_struct(groups)
    out, stats = _abi.Relation(), _abi.FuseStats()
    rc = lib().g2g_consregss(ctx._h if ctx is not None else None, C.byref(prm), many, ln, codes.ctypes.data_as(_abi.c_u8p),
                             None if w is None else w.ctypes.data_as(_abi.c_f64p), C.byref(t), None if s is None else C.byref(s),
                             int(left), ln if right is None else int(right), C.byref(out), C.byref(stats))
    if rc != 0:
        raise G2GError("g2g_consregss rc=%d: %s" % (rc, last_error()))
    rel = _take_relation(out)
    lib().g2g_relation_free(C.byref(out))
    return rel, FuseStats(stats.tests, stats.fused, stats.launches)


def conserved_regions_groups(ctx, codes: np.ndarray, tree, prm: "_abi.Params", groups=None, thr: float = 35., weight=None, dissim: bool = False) -> np.ndarray:
    """g2g_consreg_groups <-> Ssrel::consreg over a relation with groups: conserved_regions with the leaves of `tree` standing for
    `groups` (a list of member lists; None: conserved_regions itself)."""
    codes, w = _msa_args(codes, weight)
    ln, many = codes.shape
    t, keep_t = _tree_struct(tree)
    s, keep_s = _subset_struct(groups)
    out = C.POINTER(_abi.Range)()
    nout = C.c_int(0)
    rc = lib().g2g_consreg_groups(ctx._h if ctx is not None else None, C.byref(prm), float(thr), many, ln, codes.ctypes.data_as(_abi.c_u8p),
                                  None if w is None else w.ctypes.data_as(_abi.c_f64p), C.byref(t), None if s is None else C.byref(s),
                                  1 if dissim else 0, C.byref(out), C.byref(nout))
    if rc != 0:
        raise G2GError("g2g_consreg_groups rc=%d: %s" % (rc, last_error()))
    return _take_ranges(out, nout.value)


def refine_plan(ctx, codes: np.ndarray, tree, prm: "_abi.Params", thr: float = 35., weight=None, groups=None) -> RefinePlan:
    """g2g_refine_plan <-> what IterMsa::preprrn decides before it refines (reference src/prrn5.cc:794-823): the fused groups of the
    whole MSA, the unconserved ranges over them, and every range's own groups and tree.  groups: g2g_refine_plan_groups -- the plan
    starts from these groups instead of single members, tree is the tree over them (KTree.from_msa_groups)."""
    codes, w = _msa_args(codes, weight)
    ln, many = codes.shape
    t, keep_t = _tree_struct(tree)
    out = _abi.RefinePlan()
    h, wp = ctx._h if ctx is not None else None, None if w is None else w.ctypes.data_as(_abi.c_f64p)
    if groups is None:
        rc = lib().g2g_refine_plan(h, C.byref(prm), float(thr), many, ln, codes.ctypes.data_as(_abi.c_u8p), wp, C.byref(t), C.byref(out))
        if rc != 0:
            raise G2GError("g2g_refine_plan rc=%d: %s" % (rc, last_error()))
    else:
        ss, keep_s = _subset_struct(groups)
        rc = lib().g2g_refine_plan_groups(h, C.byref(prm), float(thr), many, ln, codes.ctypes.data_as(_abi.c_u8p), wp, C.byref(t), C.byref(ss),
                                          C.byref(out))
        if rc != 0:
            raise G2GError("g2g_refine_plan_groups rc=%d: %s" % (rc, last_error()))
    n = out.nranges
    rng = np.zeros((n, 2), np.int32)
    if n:
        rng[:] = np.ctypeslib.as_array(C.cast(out.ranges, C.POINTER(C.c_int32)), shape=(2 * n,)).reshape(-1, 2)
    i32 = lambda p: np.ctypeslib.as_array(p, shape=(n,)).copy() if n else np.zeros(0, np.int32)
    plan = RefinePlan(out.status == 1, _take_relation(out.whole), rng, i32(out.at_left), i32(out.at_right),
                      [_take_relation(out.range_rel[i]) for i in range(n)], FuseStats(out.stats.tests, out.stats.fused, out.stats.launches))
    lib().g2g_refine_plan_free(C.byref(out))
    return plan


# ---- the progressive alignment over a guide tree (the step between the guide tree and the first MSA) -------------------------------
def progressive(ctx, seqs: Sequence[np.ndarray], tree, prm: "_abi.Params", max_batch: int = 0, aligner=None):
    """g2g_progressive <-> ProgMsa::prog_up (reference src/prrn5.h:85-105): the sequences (arrays of residue codes, taken whole) are
    merged up the guide tree -- leaves 0 .. n - 1 = the sequences; a refine.KTree, e.g. KTree.from_dist(dist, with_weights=False), or
    anything with left, right, parent -- in waves of independent merges, at most max_batch (0: the library's default, 64) DPs to a
    batch.  aligner: an _abi.ALIGN_FN standing in for g2g_align2_batch (tests; ctx may then be None).
    Returns (codes (len, n) uint8 with gap = 1, order int32[n]: the input index of every member, [merge dicts] in the order merged,
    stats dict)."""
    L = lib()
    n = len(seqs)
    ds = (_abi.DSeq * max(n, 1))()
    keep = []
    for k, s in enumerate(seqs):
        x = np.ascontiguousarray(s, np.uint8).reshape(-1)
        keep.append(x)
        ds[k].res = x.ctypes.data_as(_abi.c_u8p)
        ds[k].len, ds[k].left, ds[k].right = len(x), 0, len(x)
    T, _keep_t = _tree_struct(tree)
    O = _abi.ProgOpts()
    O.max_batch = int(max_batch)
    if aligner is not None:
        O.aligner = aligner
    out = _abi.c_u8p(); olen = C.c_int(); order = np.zeros(max(n, 1), np.int32)
    mg = C.POINTER(_abi.ProgMerge)(); nm = C.c_int(); st = _abi.ProgStats()
    rc = L.g2g_progressive(ctx._h if ctx is not None else None, C.byref(prm), n, ds, C.byref(T), C.byref(O), C.byref(out), C.byref(olen),
                           order.ctypes.data_as(_abi.c_i32p), C.byref(mg), C.byref(nm), C.byref(st))
    if rc != 0:
        raise G2GError("g2g_progressive rc=%d: %s" % (rc, last_error()))
    codes = np.ctypeslib.as_array(out, shape=(olen.value * n,)).reshape(olen.value, n).copy()
    L.g2g_free(out)
    merges = [{k: getattr(mg[i], k) for k, _ in _abi.ProgMerge._fields_ if k != "reserved"} for i in range(nm.value)]
    L.g2g_free(mg)
    stats = {k: getattr(st, k) for k, _ in _abi.ProgStats._fields_ if k != "reserved"}
    return codes, order[:n].copy(), merges, stats


def align_sequences(ctx, seqs: Sequence[np.ndarray], molc: int, alp, distance: str = "kmer", input_order: bool = True):
    """Unaligned sequences -> the start MSA, as makemsa chains it (reference src/prrn5.cc:961-995): the distances -- "kmer":
    kmer_distance with the reference's defaults, "dp": distance_matrix with the alignment's parameters --, the guide tree
    KTree.from_dist(dist, with_weights=False), and progressive.  alp: an operator.AlnParam.  Returns (codes (len, n) uint8, tree,
    order): with input_order the columns of codes are permuted back so that member k is sequence k (order is then 0 .. n - 1), else
    member k is sequence order[k].  Refinement stays a separate call: KTree.from_msa + refine.refine_planned."""
    from .refine import KTree
    if distance not in ("kmer", "dp"):
        raise ValueError('distance is "kmer" or "dp"')
    prm, sm = alp.to_c()
    dist = kmer_distance(ctx, seqs, molc) if distance == "kmer" else distance_matrix(ctx, prm, seqs, sm)
    tree = KTree.from_dist(dist, with_weights=False)
    codes, order, _merges, _stats = progressive(ctx, seqs, tree, prm)
    if input_order:
        back = np.empty_like(order)
        back[order] = np.arange(len(order), dtype=order.dtype)
        codes = np.ascontiguousarray(codes[:, back])
        order = np.arange(len(order), dtype=np.int32)
    return codes, tree, order
