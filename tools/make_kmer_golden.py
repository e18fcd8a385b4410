#!/usr/bin/env python3
"""Generate tests/golden/kmer/*.npz from the REAL reference (oracle/_ref): the k-mer composition distances of families of single
sequences as the reference's own calcdist_kmer(Seq**, int, IM_EVRY, Strlist*&) computes them (src/qdiv.cc:273-282; parameters
through setqdiv, qdiv.cc:36-43), called in oracle/_ref/libprrn_ref.so through ctypes by their mangled names; the sequences are
read by the reference's reader (ref_seq_read of oracle/ref_shim.cc).  Data only: molc, k, measure, lens, codes, dist.

The reference keeps the parameters in a process global (wcp) and resetqdiv (qdiv.cc:45-57) swaps one molecule's defaults for the
other's: one process per case, and no protein case asks for k = 10 or QJuCa, no DNA case for k = 5 or Qpamd.

Before a case is saved the restatement (tests/kmerlib.py) must reproduce the reference on it, and no in-range pair may have an
inner logarithm argument below 0.01 (the tolerance of tests/test_kmer_host.py rests on that).
Usage: python tools/make_kmer_golden.py [case]   (needs oracle/_ref, i.e. the reference's sources at build time)"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden", "kmer")
CALCDIST = "_Z13calcdist_kmerPP3SeqiiRP7Strlist"
SETQDIV = "_Z7setqdivjPKcS0_7DistMes"
IM_EVRY = 4


def synth(n, length, seed, dna=False, **kw):
    from prrn_aln_amd.synth import make_family, DNA
    fam = make_family(n, length, seed, **({"alphabet": DNA} if dna else {}), **kw)
    return [r.replace("-", "") for r in fam.msa]


def edge_family(k, seed):
    """twins, a member of length 2 k (one word) and a member of length 2 k - 1 (no word: NaN with everyone)"""
    f = synth(10, 120, seed, indel=0.03)
    return [f[0], f[1], f[1], f[2], f[3][:2 * k], f[4], f[5][:2 * k - 1], f[0], f[6], f[7][:2 * k + 1]]


def run(name, molc, k, measure, seqs):
    """k = 0 / measure = -1: the reference's defaults (setqdiv is not called at all)"""
    import kmerlib
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
    kk, mm = kmerlib.defaults(molc, k, measure)
    assert not (molc == 1 and (kk == 10 or mm == kmerlib.QJuCa)) and not (molc == 2 and (kk == 5 or mm == kmerlib.Qpamd)), "resetqdiv would rewrite this case"
    if k or measure != -1:
        setq = getattr(L, SETQDIV)
        setq.restype = C.c_void_p
        setq.argtypes = [C.c_uint, C.c_char_p, C.c_char_p, C.c_int]
        setq(kk, None, None, mm)
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
    # elementary residues only: the reference's behaviour on others is undefined (bitpat.cc:76-86)
    assert all((kmerlib.digits(c, molc) >= 0).all() for c in codes)
    want, cnt = kmerlib.distance(codes, molc, k, measure)
    exact = np.array_equal(np.isnan(dist), np.isnan(want)) and np.array_equal(kmerlib.bits(dist[~np.isnan(dist)]), kmerlib.bits(want[~np.isnan(want)]))
    assert kmerlib.close_to_reference(want, dist), "the restatement does not reproduce the reference on %s" % name
    args = [kmerlib.inner_log_argument(int(c[0]), int(c[1]), int(c[2]), mm) for c in cnt]
    args = [a for a in args if a is not None]
    assert not args or min(args) >= 0.01, "an in-range pair of %s has an inner logarithm argument of %g" % (name, min(args))
    os.makedirs(GOLD, exist_ok=True)
    np.savez_compressed(os.path.join(GOLD, name + ".npz"), molc=np.array([molc], np.int32), k=np.array([k], np.int32),
                        measure=np.array([measure], np.int32), lens=np.array([len(c) for c in codes], np.int32),
                        codes=np.concatenate(codes), dist=dist)
    oor = int((dist == 100. * kmerlib.OUTOFRANGE).sum())
    print("%-24s %2d seqs, %3d pairs, k %2d measure %d: %d NaN, %d out of range, finite %.4g .. %.4g, smallest inner log argument %s, restatement %s"
          % (name, N, npairs, kk, mm, int(np.isnan(dist).sum()), oor, np.nanmin(np.where(dist == 100. * kmerlib.OUTOFRANGE, np.nan, dist)),
             np.nanmax(np.where(dist == 100. * kmerlib.OUTOFRANGE, np.nan, dist)), "%.3g" % min(args) if args else "-",
             "bit-equal" if exact else "within 1e-9"))


JOBS = {
    "prot_default": lambda: run("prot24_default", 1, 0, -1, synth(24, 400, 51, indel=0.02)),
    "prot_k3_qfdiv": lambda: run("prot24_k3_qfdiv", 1, 3, 0, synth(24, 400, 52, indel=0.02)),
    "prot_k4_njuca": lambda: run("prot24_k4_njuca", 1, 4, 6, synth(24, 400, 54, sub=0.02, indel=0.01)),
    "prot_k6_qcidn": lambda: run("prot24_k6_qcidn", 1, 6, 3, synth(24, 400, 54, indel=0.02)),
    # a close family: in-range and out-of-range pairs both occur under the DNA default (k = 10, QJuCa).  (At sub = 0.01 .. 0.02 this
    # generator's families of 24 have no out-of-range pair at all; at 0.04 this one has 12.)
    "dna_default": lambda: run("dna24_default_close", 2, 0, -1, synth(24, 400, 57, dna=True, sub=0.04, indel=0.005)),
    "dna_k6_njuca": lambda: run("dna24_k6_njuca", 2, 6, 6, synth(24, 400, 56, dna=True, sub=0.01, indel=0.005)),
    "dna_k15_qfidn": lambda: run("dna24_k15_qfidn", 2, 15, 1, synth(24, 400, 57, dna=True, sub=0.01, indel=0.005)),
    "prot_edges": lambda: run("prot10_edges_k4_qcdiv", 1, 4, 2, edge_family(4, 58)),
}

if __name__ == "__main__":
    if len(sys.argv) > 1:
        JOBS[sys.argv[1]]()
    else:
        for j in JOBS:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), j])
