#!/usr/bin/env python3
"""Generate tests/golden/kmer_spec/*.npz from the REAL reference (oracle/_ref): k-mer composition distances over reduced alphabets
and under spaced seeds, as the reference's own calcdist_kmer(Seq**, int, IM_EVRY, Strlist*&) computes them (src/qdiv.cc:273-282)
once setqdiv(k, ap, bp, dm) (qdiv.cc:36-43) has been given a classification and a seed and WCPRM::Nalpha (src/qdiv.h:28-35) has
been set through the pointer setqdiv returns.  Called in oracle/_ref/libprrn_ref.so through ctypes by their mangled names; the
sequences are read by the reference's reader (ref_seq_read of oracle/ref_shim.cc).

The classification and the seed strings are the reference's own, read at run time from its data symbols DefConvPat and DefBitPat
(src/bitpat.cc:26-58) and recorded in the fixture: for protein with Nalpha 6 .. 20 the reference ignores a caller's pattern and
takes DefConvPat[Nalpha - 4] (ReducWord::ReducWord, bitpat.cc:67-73), for DNA without a pattern DefConvPat[0].  A DefBitPat entry
holds two seeds separated by a comma; the first is taken.  Data only: molc, k, measure, nalpha, pattern, seed, lens, codes, dist.

One process per case (the reference keeps the parameters in a process global and resetqdiv, qdiv.cc:45-57, swaps one molecule's
defaults for the other's: no protein case asks for Nalpha 4, k = 10 or QJuCa, no DNA case for Nalpha 20, k = 5 or Qpamd).  DNA
stays with A C G T: the reference reads table entries it never wrote for N.

Before a case is saved the restatement (tests/kmerspeclib.py) must reproduce the reference on it, and no in-range pair may have
a logarithm argument below 0.01, the fit's or the one of jukcan / jukcanpro (the tolerance of tests/test_kmer_spec_host.py rests
on that).
Usage: python tools/make_kmer_spec_golden.py [case]   (needs oracle/_ref, i.e. the reference's sources at build time)"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
GOLD = os.path.join(ROOT, "tests", "golden", "kmer_spec")
CALCDIST = "_Z13calcdist_kmerPP3SeqiiRP7Strlist"
SETQDIV = "_Z7setqdivjPKcS0_7DistMes"
IM_EVRY = 4
N_CONVPAT, N_BITPAT = 17, 16                                          # entries of DefConvPat / DefBitPat (MaxBitPat)


class WCPRM(C.Structure):
    _fields_ = [("Nalpha", C.c_uint), ("Ktuple", C.c_uint), ("distm", C.c_int), ("nBitPat", C.c_uint), ("sBitPat", C.c_char_p),
                ("reducap", C.c_char_p)]


def synth(n, length, seed, dna=False, x_rate=0., **kw):
    from make_kmer_golden import synth as plain
    fam = plain(n, length, seed, dna, **kw)
    if x_rate:
        rng = np.random.default_rng(seed)
        fam = ["".join("X" if rng.random() < x_rate else c for c in s) for s in fam]
    return fam


def edge_family(width, seed):
    """twins, and members of length 2 width - 1 (no word: NaN with everyone), 2 width (one word) and 2 width + 1"""
    f = synth(10, 120, seed, indel=0.03)
    return [f[0], f[1], f[1], f[2], f[3][:2 * width], f[4], f[5][:2 * width - 1], f[0], f[6], f[7][:2 * width + 1]]


def run(name, molc, k, measure, nalpha, seqs, pattern=None, bitpat=0):
    """pattern: a classification of the maker's own (DNA only); bitpat: the DefBitPat entry whose first seed is taken, 0 for none"""
    import kmerspeclib as ks
    import refdump
    L = refdump.RefLib(molc=molc).lib
    L.ref_seq_read.restype = C.c_void_p
    L.ref_seq_read.argtypes = [C.c_char_p]
    L.ref_seq_len.argtypes = [C.c_void_p]
    L.ref_seq_range.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ref_seq_codes.argtypes = [C.c_void_p, C.POINTER(C.c_ubyte)]
    calcdist = getattr(L, CALCDIST)
    calcdist.restype = C.POINTER(C.c_double)
    calcdist.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    convpat = (C.c_char_p * N_CONVPAT).in_dll(L, "DefConvPat")
    bitpats = (C.c_char_p * N_BITPAT).in_dll(L, "DefBitPat")
    kk, mm, na = ks.resolve(molc, k, measure, nalpha)
    assert not (molc == 1 and (na == 4 or kk == 10 or mm == ks.QJuCa)) and not (molc == 2 and (na == 20 or kk == 5 or mm == ks.Qpamd)), \
        "resetqdiv would rewrite this case"
    seed = bitpats[bitpat].decode().split(",")[0] if bitpat else ""
    if molc == 1:
        assert pattern is None and 6 <= na <= 20
        used = convpat[na - 4].decode()                               # aaPat = Nalpha - 6 + SEB6, SEB6 = 2
    else:
        used = pattern if pattern is not None else convpat[0].decode()
    keep = [pattern.encode() if pattern is not None else None, seed.encode() if seed else None]   # the reference keeps the pointers
    setq = getattr(L, SETQDIV)
    setq.restype = C.POINTER(WCPRM)
    setq.argtypes = [C.c_uint, C.c_char_p, C.c_char_p, C.c_int]
    wcp = setq(kk, keep[0], keep[1], mm)
    wcp.contents.Nalpha = na
    hs, codes = [], []
    with tempfile.TemporaryDirectory() as td:
        for n, s in enumerate(seqs):
            fn = os.path.join(td, "s%d.fa" % n)
            with open(fn, "w") as fd:
                fd.write(">s%d\n%s\n" % (n, s))
            h = L.ref_seq_read(fn.encode())
            assert h
            ln = L.ref_seq_len(h)
            l, r = C.c_int(), C.c_int()
            assert L.ref_seq_range(h, C.byref(l), C.byref(r)) == 1 and l.value == 0 and r.value == ln == len(s)
            buf = (C.c_ubyte * ln)()
            L.ref_seq_codes(h, buf)
            hs.append(h); codes.append(np.frombuffer(buf, np.uint8).copy())
    N = len(hs)
    arr = (C.c_void_p * N)(*hs)
    names = C.c_void_p()
    out = calcdist(arr, N, IM_EVRY, C.byref(names))
    npairs = N * (N - 1) // 2
    dist = np.array(out[:npairs], np.float64)
    assert wcp.contents.Nalpha == na and wcp.contents.Ktuple == kk and wcp.contents.distm == mm
    if molc == 2:
        assert all(set(np.unique(c)) <= {2, 3, 5, 9} for c in codes)
    want, cnt = ks.distance(codes, molc, k, measure, nalpha, used, seed or None)
    exact = np.array_equal(np.isnan(dist), np.isnan(want)) and np.array_equal(ks.bits(dist[~np.isnan(dist)]), ks.bits(want[~np.isnan(want)]))
    assert ks.close_to_reference(want, dist), "the restatement does not reproduce the reference on %s" % name
    p0, p1 = ks.row(na, kk)
    args = [a for c in cnt for a in ks.log_arguments(int(c[0]), int(c[1]), int(c[2]), mm, p0, p1)]
    assert not args or min(args) >= 0.01, "a pair of %s has a logarithm argument of %g" % (name, min(args))
    os.makedirs(GOLD, exist_ok=True)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), molc=np.array([molc], np.int32), k=np.array([k], np.int32),
                        measure=np.array([measure], np.int32), nalpha=np.array([nalpha], np.int32), pattern=np.array([used]),
                        seed=np.array([seed]), lens=np.array([len(c) for c in codes], np.int32), codes=np.concatenate(codes), dist=dist)
    oor = dist == 100. * ks.kmerlib.OUTOFRANGE
    fin = np.where(oor, np.nan, dist)
    print("%-30s %2d seqs, Nalpha %2d k %2d measure %d seed %-14s: %d NaN, %d out of range, finite %.4g .. %.4g, smallest log argument %s, restatement %s"
          % (name, N, na, kk, mm, seed or "-", int(np.isnan(dist).sum()), int(oor.sum()), np.nanmin(fin), np.nanmax(fin),
             "%.3g" % min(args) if args else "-", "bit-equal" if exact else "within 1e-9"))


JOBS = {
    # Nalpha 14 with k 3, 4, 5: the three rows the reference's author fitted, under three fitted measures
    "prot_a14_k3": lambda: run("prot24_a14_k3_qcdiv", 1, 3, 2, 14, synth(24, 400, 61, indel=0.02)),
    "prot_a14_k4": lambda: run("prot24_a14_k4_qcidn", 1, 4, 3, 14, synth(24, 400, 62, indel=0.02)),
    "prot_a14_k5": lambda: run("prot24_a14_k5_qpamd", 1, 5, 5, 14, synth(24, 400, 63, indel=0.02)),
    # the d420 row has p1 = 0.00501: a pair must share more than half a percent of its words, so these families are close
    "prot_a14_k6": lambda: run("prot24_a14_k6_qcdiv", 1, 6, 2, 14, synth(24, 400, 64, sub=0.03, indel=0.01)),
    "prot_a6_k8": lambda: run("prot24_a6_k8_qpamd", 1, 8, 5, 6, synth(24, 400, 65, sub=0.03, indel=0.01)),
    "prot_a20_seed": lambda: run("prot24_a20_seed4_qpamd", 1, 0, -1, 20, synth(24, 400, 66, sub=0.03, indel=0.01), bitpat=4),
    "prot_a14_seed": lambda: run("prot24_a14_k4_seed1011_qpamd", 1, 4, 5, 14, synth(24, 400, 67, indel=0.02), bitpat=3),
    "prot_x_seed": lambda: run("prot24_x3_a14_k4_seed1011_qcdiv", 1, 4, 2, 14, synth(24, 400, 68, x_rate=0.03, indel=0.02), bitpat=3),
    "prot_x_cont": lambda: run("prot24_x3_a14_k4_qcdiv", 1, 4, 2, 14, synth(24, 400, 68, x_rate=0.03, indel=0.02)),
    "dna_seed": lambda: run("dna24_seed13_default", 2, 0, -1, 4, synth(24, 400, 69, dna=True, sub=0.02, indel=0.005), bitpat=9),
    "dna_two": lambda: run("dna24_a2_k12_qcdiv", 2, 12, 2, 2, synth(24, 400, 70, dna=True, sub=0.01, indel=0.005), pattern="AG|CT"),
    "prot_edges": lambda: run("prot10_edges_a14_k4_seed1011_qcdiv", 1, 4, 2, 14, edge_family(4, 71), bitpat=3),
}

if __name__ == "__main__":
    if len(sys.argv) > 1:
        JOBS[sys.argv[1]]()
    else:
        for j in JOBS:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), j])
