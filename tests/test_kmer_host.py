"""The k-mer composition distance on the host (no GPU): the restatement (tests/kmerlib.py) against the distances the REFERENCE's
calcdist_kmer computed (tests/golden/kmer, tools/make_kmer_golden.py), the library's closed forms (g2g_kmer_dist_from_counts,
csrc/g2g_kmer.hip) bit for bit against the restatement, and the argument errors of g2g_kmer_dist_batch."""
import ctypes as C

import numpy as np
import pytest

import kmerlib
from kmerlib import DNA, PROTEIN, bits
from prrn_aln_amd import _abi, guide
from prrn_aln_amd._lib import G2GError, last_error, lib

FIX = kmerlib.fixtures()
ERR_ARG, ERR_NODEVICE = -1, -3


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = np.isnan(a)
    return a.shape == b.shape and np.array_equal(n, np.isnan(b)) and np.array_equal(bits(a[~n]), bits(b[~n]))


def test_fixture_set():
    """the cases of tools/make_kmer_golden.py: both molecules, k 3 .. 6 and 6 .. 15, six of the seven measures from the reference"""
    assert [n for n, _ in FIX] == ["dna24_default_close", "dna24_k15_qfidn", "dna24_k6_njuca", "prot10_edges_k4_qcdiv", "prot24_default",
                                   "prot24_k3_qfdiv", "prot24_k4_njuca", "prot24_k6_qcidn"]
    by = dict(FIX)
    d = by["dna24_default_close"]["dist"]
    assert (d == 102400.).any() and (d < 102400.).any()                # in range and out of range
    assert (by["prot24_k4_njuca"]["dist"] == 102400.).any()
    e = by["prot10_edges_k4_qcdiv"]
    assert list(e["lens"][[4, 6, 9]]) == [8, 7, 9] and int(np.isnan(e["dist"]).sum()) == 9 and (e["dist"] == 0.).any()
    for _, g in FIX:                                                    # elementary residues only: elsewhere the reference is undefined
        assert (kmerlib.digits(g["codes"], int(g["molc"][0])) >= 0).all()


@pytest.mark.parametrize("k", range(len(FIX)), ids=[n for n, _ in FIX])
def test_restatement_reproduces_the_reference(k):
    """(a) NaN and out-of-range positions equal, elsewhere 1e-9 relative: room for the C library's log on another machine and for
    nothing else (a wrong count moves f by 1 / T, about 1e-3)"""
    g = FIX[k][1]
    got, cnt = kmerlib.distance(kmerlib.split(g), int(g["molc"][0]), int(g["k"][0]), int(g["measure"][0]))
    assert kmerlib.close_to_reference(got, g["dist"])
    assert (cnt[:, 0] <= np.minimum(cnt[:, 1], cnt[:, 2])).all()


def test_vectorised_words_equal_the_residue_by_residue_scan():
    """kmerlib.profile (numpy over the window) against the queue of Bitpat_wq restated one residue at a time, with
    non-elementary residues everywhere, window edges and ranges inside a longer buffer"""
    rng = np.random.default_rng(3)
    for molc, k in ((PROTEIN, 3), (PROTEIN, 6), (DNA, 4), (DNA, 15)):
        for n in (0, 1, 2 * k - 1, 2 * k, 2 * k + 1, 5 * k, 200):
            codes = rng.choice([3, 4, 22] if molc == PROTEIN else [2, 3, 5, 9], n).astype(np.uint8)
            codes[rng.random(n) < 0.08] = rng.choice([0, 1, 2, 23, 24, 25] if molc == PROTEIN else [0, 1, 4, 6, 16], 1)[0]
            for left, right in ((0, n), (min(3, n), n), (0, max(n - 2, 0)), (min(5, n), max(n - 4, min(5, n)))):
                a, b = kmerlib.profile(codes, molc, k, left, right), kmerlib.profile_scalar(codes, molc, k, left, right)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
                if (kmerlib.digits(codes[left:right], molc) >= 0).all():
                    assert a[2] == kmerlib.n_positions(right - left, k)


def edge_counts():
    """s, Ta, Tb rows that reach every branch: no word (NaN), nothing shared, all shared (distance 0), out of range, in range"""
    rows = [(0, 0, 0), (0, 0, 7), (0, 9, 0), (0, 5, 9), (5, 5, 9), (9, 9, 9), (1, 1, 1), (1, 396, 396), (395, 396, 396), (200, 391, 396),
            (60, 391, 396), (3, 391, 396), (16384, 16384, 16384), (1, 16384, 16384), (16383, 16384, 16384)]
    rng = np.random.default_rng(11)
    for _ in range(300):
        ta, tb = (int(x) for x in rng.integers(1, 2000, 2))
        rows.append((int(rng.integers(0, min(ta, tb) + 1)), ta, tb))
    return np.array(rows, np.int32)


@pytest.mark.parametrize("molc", [PROTEIN, DNA])
@pytest.mark.parametrize("measure", [-1, 0, 1, 2, 3, 4, 5, 6])
def test_from_counts_is_bit_equal_to_the_restatement(molc, measure):
    """(b) same process, same log: no tolerance"""
    cnt = edge_counts()
    got = guide.kmer_dist_from_counts(cnt, molc, 0, measure)
    want = kmerlib.dist_from_counts(cnt, molc, 0, measure)
    assert same_bits(got, want)
    assert np.isnan(got[:3]).all() and not np.isnan(got[3:]).any()
    m = kmerlib.defaults(molc, 0, measure)[1]
    if m in (0, 2, 4, 5, 6):                                            # the distances: 0 where every word is shared
        assert got[5] == 0. and got[6] == 0. and got[12] == 0.
    else:                                                               # the identities: 100 there (log(1.) is 0)
        assert got[5] == 100. and got[6] == 100. and (m == 3 or got[3] == 0.)
    if m in (4, 6):
        assert got[3] == 102400.                                        # nothing shared: out of range
    if m == 0:
        assert got[3] == 100. and got[4] == 0.


def test_from_counts_on_the_fixtures():
    for name, g in FIX:
        molc, k, measure = int(g["molc"][0]), int(g["k"][0]), int(g["measure"][0])
        cnt = kmerlib.counts_pairs(kmerlib.split(g), molc, k)
        got = guide.kmer_dist_from_counts(cnt, molc, k, measure)
        assert same_bits(got, kmerlib.dist_from_counts(cnt, molc, k, measure)), name
        assert kmerlib.close_to_reference(got, g["dist"]), name


def _batch(ctx, molc, k, measure, seqs, ia=None, ib=None, npairs=None, reserved=0, dist=True, kp=True):
    L = lib()
    p = _abi.KmerParams(molc, k, measure, reserved)
    ds = (_abi.DSeq * max(len(seqs), 1))()
    keep = []
    for n, s in enumerate(seqs):
        s, left, right = s if isinstance(s, tuple) else (s, 0, len(s))
        x = np.ascontiguousarray(s, np.uint8)
        keep.append(x)
        ds[n].res = x.ctypes.data_as(_abi.c_u8p)
        ds[n].len, ds[n].left, ds[n].right = len(x), left, right
    n = len(seqs)
    if npairs is None:
        npairs = n * (n - 1) // 2 if ia is None else len(ia)
    out = np.zeros(max(npairs, 1), np.float64)
    pi = lambda v: None if v is None else np.ascontiguousarray(v, np.int32).ctypes.data_as(C.POINTER(C.c_int32))
    return L.g2g_kmer_dist_batch(ctx, C.byref(p) if kp else None, n, ds if seqs else None, npairs, pi(ia), pi(ib),
                                 out.ctypes.data_as(_abi.c_f64p) if dist else None, None)


def test_argument_errors():
    """(c) every one of them is found before the device is asked for: they come back the same with and without a GPU"""
    s = [np.full(40, 3, np.uint8)] * 3
    ok = dict(ctx=None, molc=PROTEIN, k=0, measure=-1, seqs=s)
    bad = lambda **kw: _batch(**dict(ok, **kw))
    assert bad(kp=False) == ERR_ARG and bad(dist=False) == ERR_ARG and bad(seqs=[]) == ERR_ARG
    assert bad(ia=[0], ib=None, npairs=1) == ERR_ARG                    # one index vector without the other
    assert bad(molc=0) == ERR_ARG and bad(molc=3) == ERR_ARG
    assert bad(k=7) == ERR_ARG and bad(k=-1) == ERR_ARG and bad(molc=DNA, k=16) == ERR_ARG
    assert "k outside" in last_error()
    assert bad(measure=7) == ERR_ARG and bad(measure=-2) == ERR_ARG
    assert "measure" in last_error()
    assert bad(reserved=1) == ERR_ARG
    assert bad(seqs=s[:1]) == ERR_ARG                                   # nseq < 2
    assert bad(npairs=2) == ERR_ARG and bad(npairs=4) == ERR_ARG        # all pairs of 3 are 3
    assert bad(seqs=[np.full(12, 3, np.uint8)] * 4097) == ERR_ARG and "4096" in last_error()
    assert bad(ia=[0, 3], ib=[1, 1]) == ERR_ARG and "pair 1" in last_error()
    assert bad(ia=[0, 1], ib=[1, -1]) == ERR_ARG
    assert bad(seqs=[s[0], (s[1], 5, 41), s[2]]) == ERR_ARG and "sequence 1" in last_error()      # right > len
    assert bad(seqs=[s[0], s[1], (s[2], 9, 8)]) == ERR_ARG and "sequence 2" in last_error()       # right < left
    # the window limit: 16384 word positions pass the argument checks, one more is refused with the sequence named
    k = 5
    long_ok, too_long = np.full(kmerlib.MAX_WINDOW + 2 * k - 1, 3, np.uint8), np.full(kmerlib.MAX_WINDOW + 2 * k, 3, np.uint8)
    assert bad(seqs=[s[0], too_long]) == ERR_ARG
    assert "sequence 1" in last_error() and "16385" in last_error() and "16384" in last_error()
    assert bad(seqs=[s[0], (too_long, 1, len(too_long))], k=k) == ERR_ARG and "no context" in last_error()   # the window counts, not the buffer
    assert bad(seqs=[s[0], long_ok]) == ERR_ARG and "no context" in last_error()
    # with every argument in order a NULL context is the last thing refused
    assert bad() == ERR_ARG and "no context" in last_error()
    assert bad(molc=DNA, k=15, measure=6, ia=[0, 1, 1, 2], ib=[1, 0, 1, 2]) == ERR_ARG and "no context" in last_error()


def test_without_a_device():
    """a context without a usable device answers G2G_ERR_NODEVICE -- after the argument checks -- and never computes on the host;
    where g2g_create gives no context at all (no HIP device visible) the Python entry raises"""
    L = lib()
    h = L.g2g_create(-1)
    s = [np.full(40, 3, np.uint8)] * 3
    try:
        if not h:
            from prrn_aln_amd import engine
            with pytest.raises(G2GError):
                guide.kmer_distance(engine.Context(), s, PROTEIN)
            return
        if L.g2g_device_ok(h):
            assert _batch(h, PROTEIN, 9, -1, s) == ERR_ARG              # (a device is here: the GPU tests take over)
            return
        assert _batch(h, PROTEIN, 9, -1, s) == ERR_ARG                  # the argument checks come first
        assert _batch(h, PROTEIN, 0, -1, s) == ERR_NODEVICE
    finally:
        if h:
            L.g2g_destroy(h)


def test_from_counts_errors():
    L = lib()
    kp = _abi.KmerParams(PROTEIN, 0, -1, 0)
    out = np.zeros(2, np.float64)
    cnt = np.array([[1, 2, 3], [4, 3, 5]], np.int32)
    pc, po = cnt.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(_abi.c_f64p)
    assert L.g2g_kmer_dist_from_counts(None, 2, pc, po) == ERR_ARG
    assert L.g2g_kmer_dist_from_counts(C.byref(kp), 2, None, po) == ERR_ARG and L.g2g_kmer_dist_from_counts(C.byref(kp), 2, pc, None) == ERR_ARG
    assert L.g2g_kmer_dist_from_counts(C.byref(kp), 2, pc, po) == ERR_ARG and "pair 1" in last_error()      # s > min(Ta, Tb)
    assert L.g2g_kmer_dist_from_counts(C.byref(kp), 1, pc, po) == 0 and out[0] == kmerlib.dist_from_counts(cnt[:1], PROTEIN)[0]
    assert L.g2g_kmer_dist_from_counts(C.byref(kp), 0, None, None) == 0
    for bad in (_abi.KmerParams(PROTEIN, 7, -1, 0), _abi.KmerParams(DNA, 0, 7, 0), _abi.KmerParams(0, 0, -1, 0)):
        assert L.g2g_kmer_dist_from_counts(C.byref(bad), 1, pc, po) == ERR_ARG
    with pytest.raises(G2GError):
        guide.kmer_dist_from_counts(cnt, PROTEIN)


def test_struct_size_matches_header():
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "p.c"), "w").write('#include <stdio.h>\n#include "g2g.h"\nint main(){printf("%zu\\n", sizeof(g2g_kmer_params));}')
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), "-o", os.path.join(td, "p"), os.path.join(td, "p.c")])
        assert int(subprocess.check_output([os.path.join(td, "p")]).decode()) == C.sizeof(_abi.KmerParams) == 16
