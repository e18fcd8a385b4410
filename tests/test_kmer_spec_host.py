"""The k-mer composition distance over reduced alphabets and under spaced seeds, on the host (no GPU): the restatement
(tests/kmerspeclib.py) against the distances the REFERENCE's calcdist_kmer computed (tests/golden/kmer_spec,
tools/make_kmer_spec_golden.py), the library's closed forms (g2g_kmer_dist_from_counts_spec, csrc/g2g_kmer.hip) bit for bit against
the restatement, guide.kmer_classes against the restatement's table, and the argument errors of g2g_kmer_dist_batch_spec."""
import ctypes as C

import numpy as np
import pytest

import kmerlib
import kmerspeclib as ks
from kmerlib import DNA, PROTEIN, bits
from prrn_aln_amd import _abi, guide
from prrn_aln_amd._lib import G2GError, last_error, lib

FIX = ks.fixtures()
ERR_ARG, ERR_NODEVICE = -1, -3
PAT14 = ks.case(dict(FIX)["prot24_a14_k3_qcdiv"])["classes"]          # the 14-class pattern that fixture records (X: class 14, no word)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = np.isnan(a)
    return a.shape == b.shape and np.array_equal(n, np.isnan(b)) and np.array_equal(bits(a[~n]), bits(b[~n]))


def test_fixture_set():
    """the cases of tools/make_kmer_spec_golden.py: the three fitted rows of Nalpha 14 under three fitted measures, the fall back
    to d420, Nalpha 6 and 20, seeds on both molecules, X residues under a seed and without, two DNA classes, the edges"""
    assert [n for n, _ in FIX] == ["dna24_a2_k12_qcdiv", "dna24_seed13_default", "prot10_edges_a14_k4_seed1011_qcdiv", "prot24_a14_k3_qcdiv",
                                   "prot24_a14_k4_qcidn", "prot24_a14_k4_seed1011_qpamd", "prot24_a14_k5_qpamd", "prot24_a14_k6_qcdiv",
                                   "prot24_a20_seed4_qpamd", "prot24_a6_k8_qpamd", "prot24_x3_a14_k4_qcdiv", "prot24_x3_a14_k4_seed1011_qcdiv"]
    by = dict(FIX)
    for name, g in FIX:
        c = ks.case(g)
        assert set(g) == {"molc", "k", "measure", "nalpha", "pattern", "seed", "lens", "codes", "dist"} and c["classes"], name
        if c["molc"] == DNA:                                            # the reference is undefined on N
            assert set(np.unique(g["codes"])) <= {2, 3, 5, 9}
    assert len(ks.case(by["dna24_seed13_default"])["seed"]) >= 13
    assert ks.case(by["prot24_a20_seed4_qpamd"])["seed"].count("1") == 4
    for n in ("prot24_x3_a14_k4_qcdiv", "prot24_x3_a14_k4_seed1011_qcdiv"):
        x = (by[n]["codes"] == 2).mean()
        assert 0.02 < x < 0.04
    e = by["prot10_edges_a14_k4_seed1011_qcdiv"]
    w = len(ks.case(e)["seed"])
    assert list(e["lens"][[4, 6, 9]]) == [2 * w, 2 * w - 1, 2 * w + 1] and int(np.isnan(e["dist"]).sum()) == 9 and (e["dist"] == 0.).any()


@pytest.mark.parametrize("k", range(len(FIX)), ids=[n for n, _ in FIX])
def test_restatement_reproduces_the_reference(k):
    """NaN and out-of-range positions equal, elsewhere 1e-9 relative (kmerlib.close_to_reference: room for the C library's log on
    another machine and for nothing else -- a wrong count moves f by 1 / T, about 1e-3, another row of param by far more)"""
    g = FIX[k][1]
    got, cnt = ks.distance(ks.split(g), **ks.case(g))
    assert ks.close_to_reference(got, g["dist"])
    assert (cnt[:, 0] <= np.minimum(cnt[:, 1], cnt[:, 2])).all()


def test_vectorised_words_equal_the_residue_by_residue_scan():
    """ks.profile (numpy over the window) against the ring of Bitpat_wq restated one residue at a time: bad residues everywhere,
    window edges, ranges inside a longer buffer; and the all-ones seed against the continuous one"""
    rng = np.random.default_rng(5)
    tab = ks.classes_from_pattern(PAT14, PROTEIN)
    for nalpha, k, seed in ((14, 3, None), (14, 4, "1011"), (6, 8, None), (14, 5, "110101"), (20, 2, "1" + "0" * 30 + "1"), (3, 4, "1111")):
        w = ks.width_of(k, seed)
        for n in (0, 1, 2 * w - 1, 2 * w, 2 * w + 1, 5 * w, 300):
            codes = rng.integers(3, 23, n).astype(np.uint8)
            codes[rng.random(n) < 0.06] = 2
            for left, right in ((0, n), (min(3, n), n), (0, max(n - 2, 0)), (min(5, n), max(n - 4, min(5, n)))):
                a, b = ks.profile(codes, tab, nalpha, k, seed, left, right), ks.profile_scalar(codes, tab, nalpha, k, seed, left, right)
                assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
                if seed == "1111":
                    c = ks.profile(codes, tab, nalpha, 4, None, left, right)
                    assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1]) and a[2] == c[2]
    # with the full alphabet and no seed it is kmerlib's
    codes = rng.integers(2, 24, 200).astype(np.uint8)
    a, b = ks.profile(codes, ks.full_classes(PROTEIN), 20, 5), kmerlib.profile(codes, PROTEIN, 5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def edge_counts():
    """s = 0, s = min(Ta, Tb), Ta = 0, and what lies between"""
    rows = [(0, 0, 0), (0, 0, 7), (0, 9, 0), (0, 5, 9), (5, 5, 9), (9, 9, 9), (1, 1, 1), (1, 396, 396), (395, 396, 396), (200, 391, 396),
            (60, 391, 396), (3, 391, 396), (16384, 16384, 16384), (1, 16384, 16384)]
    rng = np.random.default_rng(11)
    for _ in range(100):
        ta, tb = (int(x) for x in rng.integers(1, 2000, 2))
        rows.append((int(rng.integers(0, min(ta, tb) + 1)), ta, tb))
    for _, g in FIX:
        c = ks.case(g)
        rows += [tuple(r) for r in ks.counts_pairs(ks.split(g), c["molc"], c["k"], c["nalpha"], c["classes"], c["seed"])]
    return np.array(rows, np.int32)


COUNTS = edge_counts()
# (nalpha, k, seed): the rows d314, d414, d514, and d420 three ways; the last goes by k = 4, not by the weight 3
ROWS = [(14, 3, None), (14, 4, None), (14, 5, None), (14, 6, None), (20, 5, None), (14, 4, "1011")]


@pytest.mark.parametrize("measure", range(7))
@pytest.mark.parametrize("nalpha,k,seed", ROWS)
def test_from_counts_is_bit_equal_to_the_restatement(nalpha, k, seed, measure):
    """same process, same log: no tolerance"""
    got = guide.kmer_dist_from_counts_spec(COUNTS, PROTEIN, k, measure, nalpha, seed)
    want = ks.dist_from_counts(COUNTS, PROTEIN, k, measure, nalpha, seed)
    assert same_bits(got, want)
    assert np.isnan(got[:3]).all() and not np.isnan(got[3:114]).any()   # (the edges fixture has wordless members further on)
    if measure in (0, 2, 4, 5, 6):
        assert got[5] == 0. and got[6] == 0.                            # every word shared: log(1.) is 0
    p0, p1 = ks.row(nalpha, k)
    assert (p0, p1) == {3: (0.92042, 0.18677), 4: (0.34576, 0.07108), 5: (0.22333, 0.03164)}.get(k if nalpha == 14 else 0, (0.18704, 0.00501))


def test_rows_differ():
    """the four rows give four different distances for the same counts, and a seed's weight does not pick the row"""
    c = np.array([[60, 391, 396]], np.int32)
    d = [guide.kmer_dist_from_counts_spec(c, PROTEIN, k, 2, 14)[0] for k in (3, 4, 5, 6)]
    assert len(set(d)) == 4
    assert guide.kmer_dist_from_counts_spec(c, PROTEIN, 4, 2, 14, "1011")[0] == d[1]
    assert guide.kmer_dist_from_counts_spec(c, PROTEIN, 3, 2, 14, "1011")[0] == d[0]
    assert guide.kmer_dist_from_counts_spec(c, PROTEIN, 4, 2, 13)[0] == d[3] == guide.kmer_dist_from_counts_spec(c, PROTEIN, 4, 2, 20)[0]


@pytest.mark.parametrize("molc", [PROTEIN, DNA])
@pytest.mark.parametrize("measure", [-1, 0, 1, 2, 3, 4, 5, 6])
def test_default_spec_is_the_old_entry(molc, measure):
    for k in (0, 3, 6):
        assert same_bits(guide.kmer_dist_from_counts_spec(COUNTS, molc, k, measure), guide.kmer_dist_from_counts(COUNTS, molc, k, measure))


def test_from_counts_on_the_fixtures():
    for name, g in FIX:
        c = ks.case(g)
        cnt = ks.counts_pairs(ks.split(g), c["molc"], c["k"], c["nalpha"], c["classes"], c["seed"])
        got = guide.kmer_dist_from_counts_spec(cnt, c["molc"], c["k"], c["measure"], c["nalpha"], c["seed"])
        assert same_bits(got, ks.dist_from_counts(cnt, c["molc"], c["k"], c["measure"], c["nalpha"], c["seed"])), name
        assert ks.close_to_reference(got, g["dist"]), name


def test_kmer_classes():
    for name, g in FIX:
        c = ks.case(g)
        tab = guide.kmer_classes(c["classes"], c["molc"])
        assert tab.dtype == np.uint8 and tab.shape == (256,) and np.array_equal(tab, ks.classes_from_pattern(c["classes"], c["molc"])), name
        assert int(tab[tab != 0xFF].max()) >= c["nalpha"] - 1
    t = guide.kmer_classes("ag|ct", DNA)
    assert [int(t[c]) for c in (2, 5, 3, 9)] == [0, 0, 1, 1] and (np.delete(t, [2, 3, 5, 9]) == 0xFF).all()
    t = guide.kmer_classes("ILVM,de-KRH X", PROTEIN)                   # any non-letter starts the next class
    assert [int(t[c]) for c in (12, 13, 22, 15, 6, 9, 14, 4, 11, 2)] == [0, 0, 0, 0, 1, 1, 2, 2, 2, 3] and int((t != 0xFF).sum()) == 10
    assert (guide.kmer_classes("", PROTEIN) == 0xFF).all()


def _batch(ctx, molc=PROTEIN, k=0, measure=-1, nalpha=0, classes=None, nclasses=None, seed=None, seqs=(), ia=None, ib=None, npairs=None,
           reserved=0, dist=True, sp=True):
    L = lib()
    p = _abi.KmerSpec()
    p.molc, p.k, p.measure, p.nalpha, p.reserved = molc, k, measure, nalpha, reserved
    tab = None
    if classes is not None:
        tab = np.ascontiguousarray(classes, np.uint8)
        p.classes = tab.ctypes.data_as(_abi.c_u8p)
    p.nclasses = (0 if tab is None else len(tab)) if nclasses is None else nclasses
    p.seed = None if seed is None else seed.encode()
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
    return L.g2g_kmer_dist_batch_spec(ctx, C.byref(p) if sp else None, n, ds if seqs else None, npairs, pi(ia), pi(ib),
                                      out.ctypes.data_as(_abi.c_f64p) if dist else None, None)


S3 = [np.full(80, 3, np.uint8)] * 3
TAB14 = ks.classes_from_pattern(PAT14, PROTEIN)


def test_argument_errors():
    """every one of them is found before the device is asked for: they come back the same with and without a GPU"""
    ok = dict(ctx=None, seqs=S3)
    bad = lambda **kw: _batch(**dict(ok, **kw))
    refused = lambda word, **kw: bad(**kw) == ERR_ARG and word in last_error()
    passes = lambda **kw: refused("no context", **kw)                   # with every argument in order a NULL context is the last refusal
    assert passes() and passes(nalpha=20) and passes(molc=DNA, nalpha=4) and passes(nalpha=14, classes=TAB14)
    assert bad(sp=False) == ERR_ARG and bad(dist=False) == ERR_ARG and bad(seqs=[]) == ERR_ARG
    assert refused("molc", molc=0) and refused("molc", molc=3)
    # nalpha
    assert refused("nalpha", nalpha=1, classes=TAB14) and refused("nalpha", nalpha=21, classes=TAB14) and refused("nalpha", nalpha=-1, classes=TAB14)
    assert refused("nalpha", molc=DNA, nalpha=5, classes=TAB14) and passes(molc=DNA, nalpha=2, classes=TAB14, k=12)
    assert refused("needs classes", nalpha=14) and refused("needs classes", molc=DNA, nalpha=2)
    # nclasses
    assert refused("nclasses", nalpha=14, classes=TAB14, nclasses=0) and refused("nclasses", nalpha=14, classes=TAB14, nclasses=257)
    assert refused("nclasses", nalpha=14, classes=TAB14, nclasses=-1) and passes(nalpha=14, classes=TAB14, nclasses=1)
    assert passes(nalpha=14, classes=TAB14, nclasses=256)
    # the continuous seed: nalpha^(k + 1) <= 2^32.  14^8 <= 2^32 < 14^9; 20^7 <= 2^32 < 20^8; 6^12 <= 2^32 < 6^13; 2^16, 4^16 <= 2^32
    assert 14 ** 8 <= 2 ** 32 < 14 ** 9 and 20 ** 7 <= 2 ** 32 < 20 ** 8 and 6 ** 12 <= 2 ** 32 < 6 ** 13
    assert passes(nalpha=14, classes=TAB14, k=7) and refused("nalpha^(k + 1)", nalpha=14, classes=TAB14, k=8)
    assert refused("nalpha^(k + 1)", nalpha=14, classes=TAB14, k=9)
    assert passes(k=6) and refused("nalpha^(k + 1)", k=7)
    assert passes(nalpha=6, classes=TAB14, k=11) and refused("nalpha^(k + 1)", nalpha=6, classes=TAB14, k=12)
    assert passes(nalpha=2, classes=TAB14, k=15) and passes(molc=DNA, k=15)
    assert refused("k outside", k=16) and refused("k outside", k=-1) and refused("k outside", molc=DNA, k=16) and refused("k outside", k=16, seed="11")
    assert refused("measure", measure=7) and refused("measure", measure=-2)
    # seed strings
    for s in ("", "0110", "1012", "011", "110", "1 1", "1" * 33, "1" + "0" * 32 + "1"):
        assert refused("seed", seed=s), s
    assert refused("weight", seed="1" * 16) and refused("weight", molc=DNA, seed="1" * 16) and refused("weight", seed="1" + "01" * 15)
    assert passes(molc=DNA, seed="1" * 15) and passes(molc=DNA, seed="1" + "0" * 17 + "1" * 14)      # 4^15 < 2^32, width 32
    assert passes(seed="1" * 7) and refused("nalpha^weight", seed="1" * 8)                             # 20^7 < 2^32 <= 20^8
    assert passes(nalpha=14, classes=TAB14, seed="1" * 8) and refused("nalpha^weight", nalpha=14, classes=TAB14, seed="1" * 9)
    assert passes(nalpha=2, classes=TAB14, seed="1" * 15)
    assert passes(seed="1011", k=0) and passes(seed="1011", k=15) and passes(seed="1", k=1)
    assert refused("reserved", reserved=1)
    # the rest is g2g_kmer_dist_batch's
    assert bad(ia=[0], ib=None, npairs=1) == ERR_ARG and bad(seqs=S3[:1]) == ERR_ARG and bad(npairs=2) == ERR_ARG
    assert refused("4096", seqs=[np.full(12, 3, np.uint8)] * 4097)
    assert refused("pair 1", ia=[0, 3], ib=[1, 1]) and bad(ia=[0, 1], ib=[1, -1]) == ERR_ARG
    assert refused("sequence 1", seqs=[S3[0], (S3[1], 5, 81), S3[2]]) and refused("sequence 2", seqs=[S3[0], S3[1], (S3[2], 9, 8)])
    assert passes(molc=DNA, k=15, measure=6, ia=[0, 1, 1, 2], ib=[1, 0, 1, 2])


@pytest.mark.parametrize("seed,k", [("1" + "0" * 30 + "1", 0), ("1011", 0), (None, 5), (None, 1)])
def test_window_limit_counts_with_the_width(seed, k):
    """16384 word positions pass the argument checks, one more is refused with the sequence named; the window counts, not the
    buffer; under a seed the positions are (right - left) - 2 width + 1, whatever k"""
    w = ks.width_of(k, seed)
    long_ok, too_long = np.full(kmerlib.MAX_WINDOW + 2 * w - 1, 3, np.uint8), np.full(kmerlib.MAX_WINDOW + 2 * w, 3, np.uint8)
    assert _batch(None, k=k, seed=seed, seqs=[S3[0], too_long]) == ERR_ARG
    assert "sequence 1" in last_error() and "16385" in last_error() and "16384" in last_error() and "g2g_kmer_dist_batch_spec" in last_error()
    assert _batch(None, k=k, seed=seed, seqs=[S3[0], (too_long, 1, len(too_long))]) == ERR_ARG and "no context" in last_error()
    assert _batch(None, k=k, seed=seed, seqs=[S3[0], long_ok]) == ERR_ARG and "no context" in last_error()


def test_without_a_device():
    """a context without a usable device answers G2G_ERR_NODEVICE -- after the argument checks -- and never computes on the host;
    where g2g_create gives no context at all (no HIP device visible) the Python entry raises"""
    L = lib()
    h = L.g2g_create(-1)
    try:
        if not h:
            from prrn_aln_amd import engine
            with pytest.raises(G2GError):
                guide.kmer_distance_spec(engine.Context(), S3, PROTEIN, 4, nalpha=14, classes=PAT14, seed="1011")
            return
        assert _batch(h, nalpha=14, classes=TAB14, k=9, seqs=S3) == ERR_ARG      # the argument checks come first
        if L.g2g_device_ok(h):
            return                                                      # (a device is here: the GPU tests take over)
        assert _batch(h, nalpha=14, classes=TAB14, k=4, seed="1011", seqs=S3) == ERR_NODEVICE
    finally:
        if h:
            L.g2g_destroy(h)


def test_from_counts_spec_errors():
    L = lib()
    out = np.zeros(2, np.float64)
    cnt = np.array([[1, 2, 3], [4, 3, 5]], np.int32)
    pc, po = cnt.ctypes.data_as(C.POINTER(C.c_int32)), out.ctypes.data_as(_abi.c_f64p)

    def spec(molc=PROTEIN, k=0, measure=-1, nalpha=0, seed=None, reserved=0):
        p = _abi.KmerSpec()
        p.molc, p.k, p.measure, p.nalpha, p.reserved, p.seed = molc, k, measure, nalpha, reserved, seed
        return p

    f = L.g2g_kmer_dist_from_counts_spec
    assert f(None, 2, pc, po) == ERR_ARG
    assert f(C.byref(spec()), 2, None, po) == ERR_ARG and f(C.byref(spec()), 2, pc, None) == ERR_ARG
    assert f(C.byref(spec()), 2, pc, po) == ERR_ARG and "pair 1" in last_error() and "g2g_kmer_dist_from_counts_spec" in last_error()
    assert f(C.byref(spec(nalpha=14, k=4)), 1, pc, po) == 0 and out[0] == ks.dist_from_counts(cnt[:1], PROTEIN, 4, -1, 14)[0]   # no classes needed
    assert f(C.byref(spec()), 0, None, None) == 0
    for bad in (spec(k=7), spec(nalpha=14, k=8), spec(nalpha=21), spec(molc=DNA, measure=7), spec(molc=0), spec(seed=b"0110"), spec(reserved=1)):
        assert f(C.byref(bad), 1, pc, po) == ERR_ARG
    with pytest.raises(G2GError):
        guide.kmer_dist_from_counts_spec(cnt, PROTEIN)


def test_struct_size_matches_header():
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as td:
        open(os.path.join(td, "p.c"), "w").write('#include <stdio.h>\n#include <stddef.h>\n#include "g2g.h"\nint main(){printf("%zu %zu %zu %zu\\n", '
                                                 'sizeof(g2g_kmer_spec), offsetof(g2g_kmer_spec, classes), offsetof(g2g_kmer_spec, nclasses), '
                                                 'offsetof(g2g_kmer_spec, seed));}')
        subprocess.check_call(["gcc", "-I", os.path.join(root, "include"), "-o", os.path.join(td, "p"), os.path.join(td, "p.c")])
        got = [int(x) for x in subprocess.check_output([os.path.join(td, "p")]).decode().split()]
    K = _abi.KmerSpec
    assert got == [C.sizeof(K), K.classes.offset, K.nclasses.offset, K.seed.offset] == [40, 16, 24, 32]
