#!/usr/bin/env python3
"""Generate tests/golden/consreg/*.npz from the REAL reference (oracle/_ref): the conserved regions of small MSAs as the reference's
own Ssrel::consreg computes them (src/consreg.cc:484-518), and per division of the weighting tree the ranges of Ssrel::constwo
(:438-450) on sons the reference's mSeq::extseq extracted -- called in oracle/_ref/libprrn_ref.so through ctypes by their mangled
names.  A zero-filled block is a default Ssrel (consreg.h:99); set_localprm sets u, v, thr of consreg's own parameter block.  Data
only: codes, weights, the tree consreg built (read out of its Ktree), u, v, thr, similarity matrix number 1 as the reference holds
it, each division's member lists and ranges, the united ranges for dissim 0 and 1.

The reference keeps its parameters in process globals: one process per case.

Before a case is saved
  - similarity matrix 0 read the same way must equal what ref_dist_params reports;
  - the intersection of the divisions' ranges must be consreg's own result (so the tree read out is the tree it used);
  - the restatement (tests/consreglib.py, on the library's HOST-built PwdMs) must reproduce every per-division range list;
  - the case must pin something: at least 4 ranges in some division and a non-empty united result (except the case made to be empty).
Usage: python tools/make_consreg_golden.py [case]            (needs oracle/_ref, i.e. the reference's sources at build time)
       python tools/make_consreg_golden.py --time [repeats]  the reference's Ssrel::consreg on tests/golden/msa/prog256x1024.npz and
                                                             on a 16-member fixture, wall clock on one core, as one JSON line:
                                                             ms_median is consreg itself (tree included; it stops at the first empty
                                                             intersection), all_divisions_ms extseq + constwo of all 2 N - 3 divisions"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden", "consreg")
CONSREG = "_ZN5Ssrel7consregEP4mSeqi"
CONSTWO = "_ZN5Ssrel7constwoEPP4mSeq"
EXTSEQ = "_ZN4mSeq6extseqEPS_Piid"
SET_LOCALPRM = "_Z12set_localprmfff"
CPY_SEQ, CPY_NBR = 1, 2
INT_MAX = 2 ** 31 - 1
_AA = "ARNDCQEGHILKMFPSTWYV"


class Ref:
    def __init__(self, molc):
        import refdump
        self.R = refdump.RefLib(molc=molc, band=True)
        L = self.L = self.R.lib
        self.consreg = getattr(L, CONSREG)
        self.consreg.restype = C.c_void_p
        self.consreg.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        self.constwo = getattr(L, CONSTWO)
        self.constwo.restype = C.c_void_p
        self.constwo.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
        self.extseq = getattr(L, EXTSEQ)
        self.extseq.restype = C.c_void_p
        self.extseq.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_int), C.c_int, C.c_double]
        self.set_localprm = getattr(L, SET_LOCALPRM)
        self.set_localprm.restype = None
        self.set_localprm.argtypes = [C.c_float, C.c_float, C.c_float]
        L.ref_dist_params.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def matrix(self, no):
        """Simmtx::mtx of simmtxes.storedSimmtx[no] (simmtx.h:35-82): {double* mdmcomp; int current; Simmtx* stored[3]}, and in a
        Simmtx dim / rows at bytes 32 / 36 and the row pointers at byte 56"""
        base = C.addressof((C.c_char * 40).in_dll(self.L, "simmtxes"))
        sm = C.cast(base + 16 + 8 * no, C.POINTER(C.c_void_p))[0]
        assert sm, "the reference holds no similarity matrix number %d" % no
        dim = C.cast(sm + 32, C.POINTER(C.c_int))[0]
        rows = C.cast(sm + 36, C.POINTER(C.c_int))[0]
        rowp = C.cast(C.cast(sm + 56, C.POINTER(C.c_void_p))[0], C.POINTER(C.c_void_p))
        out = np.zeros((rows, dim), np.float64)
        for i in range(rows):
            out[i] = np.ctypeslib.as_array(C.cast(rowp[i], C.POINTER(C.c_double)), shape=(dim,))
        return out

    def matrix0_reported(self):
        uvst = (C.c_double * 4)(); sh = C.c_int(); dim = C.c_int(); rows = C.c_int()
        buf = (C.c_double * 4096)()
        assert self.L.ref_dist_params(uvst, C.byref(sh), buf, 4096, C.byref(dim), C.byref(rows)) == 0
        return np.array(buf[:rows.value * dim.value]).reshape(rows.value, dim.value)

    @staticmethod
    def ranges(p):
        """a RANGE list: entry 0 = {n, n} with n entries in all, the last one endrng"""
        a = C.cast(p, C.POINTER(C.c_int))
        n = a[0]
        assert a[1] == n and a[2 * (n - 1)] == INT_MAX
        return [(a[2 * k], a[2 * k + 1]) for k in range(1, n - 1)]

    def tree(self, ssrel, many):
        """Ssrel::ktree (consreg.h:95-96) -> Ktree::lead (phyl.h:402-418: byte 48) -> Knode[2 many - 1] (phyl.h:115-126: 80 bytes;
        left / right / parent pointers, tid at byte 24)"""
        kt = C.cast(C.addressof(ssrel) + 8, C.POINTER(C.c_void_p))[0]
        assert kt
        lead = C.cast(kt + 48, C.POINTER(C.c_void_p))[0]
        nn = 2 * many - 1
        out = np.full((3, nn), -1, np.int32)
        for k in range(nn):
            node = lead + 80 * k
            assert C.cast(node + 24, C.POINTER(C.c_int))[0] == k
            for f in range(3):
                p = C.cast(node + 8 * f, C.POINTER(C.c_void_p))[0]
                if p:
                    assert (p - lead) % 80 == 0 and 0 <= (p - lead) // 80 < nn
                    out[f, k] = (p - lead) // 80
        return out


def family(n, length, seed, dna=False, **kw):
    from prrn_aln_amd.synth import make_family, DNA
    return list(make_family(n, length, seed, **({"alphabet": DNA} if dna else {}), **kw).msa)


def ungapped(n, length, seed, sub=0.25):
    rng = np.random.default_rng(seed)
    anc = rng.integers(0, 20, length)
    rows = []
    for m in range(n):
        s = anc.copy()
        hit = rng.random(length) < sub * (0.3 + 1.4 * m / n)
        s[hit] = rng.integers(0, 20, int(hit.sum()))
        rows.append("".join(_AA[x] for x in s))
    return rows


def with_clean_members(rows, clean):
    """the members `clean` get a residue in every column (their gaps are filled from the member in front of them)"""
    rows = [list(r) for r in rows]
    for m in clean:
        for c in range(len(rows[m])):
            if rows[m][c] == "-":
                donors = [r[c] for r in rows if r[c] != "-"]
                rows[m][c] = donors[0] if donors else "A"
    return ["".join(r) for r in rows]


def with_outlier(rows, m, seed):
    """member m keeps its gaps and gets random residues: the division that isolates it has no conserved column"""
    rng = np.random.default_rng(seed)
    rows = list(rows)
    rows[m] = "".join(c if c == "-" else _AA[int(rng.integers(0, 20))] for c in rows[m])
    return rows


def run(name, molc, rows, u=-1., v=-1., thrs=(35., 20., 10., 5.), weight=None, want_empty=False, swapped_too=False, save=True):
    """swapped_too: every division in which one son is free of gaps is recorded a second time with its sons exchanged (not a division
    of the tree: div_in_tree 0), so that constwo's HLF and RHF branches both occur"""
    import consreglib as cl
    from prrn_aln_amd import operator as op
    ref = Ref(molc)
    m0 = ref.matrix(0)
    assert np.array_equal(m0, ref.matrix0_reported()), "matrix 0 read through the structure differs from ref_dist_params"
    simmtx = ref.matrix(1)
    codes = op.encode(rows, molc)
    ln, many = codes.shape
    names = ["m%d" % i for i in range(many)]
    for thr in thrs:
        ref.set_localprm(u, v, thr)
        uu, vv = (3. if u < 0 else u), (10. if v < 0 else v)
        sd = ref.R.group(names, rows, weight)
        assert ref.L.ref_group_many(sd) == many and ref.L.ref_group_len(sd) == ln
        united = []
        ssrel = (C.c_char * 256)()
        for dissim in (0, 1):
            p = ref.consreg(C.addressof(ssrel), sd, dissim)
            united.append(ref.ranges(p))
        tree = ref.tree(ssrel, many)
        g = dict(molc=np.array([molc], np.int32), max_code=np.array([25 if molc == 1 else 17], np.int32), u=np.array([uu]), v=np.array([vv]),
                 simmtx=simmtx)
        alp = cl.alp_of(g)
        divs, modes, in_tree = [], [], []
        inter = [(0, ln)]
        ok = True
        todo = [(l, 1) for l in cl.divisions(tree[0], tree[1], tree[2], many)]
        if swapped_too:
            todo += [((l[1], l[0]), 0) for l, _ in list(todo) if not (codes[:, l[0]] <= 1).any() or not (codes[:, l[1]] <= 1).any()]
        for lists, real in todo:
            sons = (C.c_void_p * 2)()
            for s in range(2):
                lst = (C.c_int * (len(lists[s]) + 1))(*(list(lists[s]) + [-1]))
                sons[s] = ref.extseq(sd, None, lst, CPY_SEQ + CPY_NBR, 1.0)
            rng = ref.ranges(ref.constwo(C.addressof(ssrel), sons))
            pw = cl.host_pair(codes, lists, alp, weight)
            mine = cl.scan(cl.colscores(pw.problem), cl.vthr_of(pw, thr))
            if mine != rng:
                ok = False
                print("%s thr %g: division %s | %s: restatement %s, reference %s (mode %d)" % (name, thr, lists[0], lists[1], mine, rng, pw.alnmode))
            divs.append((lists[0], lists[1], rng)); modes.append(pw.alnmode); in_tree.append(real)
            if real:
                inter = cl.cmnrng(inter, rng)
        assert ok, "the restatement does not reproduce the reference on %s" % name
        assert inter == united[0], "the divisions read from consreg's tree do not give consreg's result: %s against %s" % (inter, united[0])
        assert cl.complerng(ln, inter) == united[1], (cl.complerng(ln, inter), united[1])
        most = max(len(d[2]) for d in divs)
        pins = most >= 4 and (bool(united[0]) != want_empty)
        if pins or thr == thrs[-1]:
            break
    assert pins, "%s pins nothing: most ranges in a division %d, united %s" % (name, most, united[0])
    cat = lambda xs, dt: (np.concatenate([np.asarray(x, dt).reshape(-1) for x in xs]) if xs else np.zeros(0, dt))
    offs = lambda xs: np.concatenate([[0], np.cumsum([len(x) for x in xs])]).astype(np.int32)
    if save:
        os.makedirs(GOLD, exist_ok=True)
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), codes=codes, weight=np.asarray(weight if weight is not None else [], np.float64),
                            tree_left=tree[0], tree_right=tree[1], tree_parent=tree[2], thr=np.array([thr]), ndiv=np.array([len(divs)], np.int32),
                            div_l0=cat([d[0] for d in divs], np.int32), div_l0_off=offs([d[0] for d in divs]),
                            div_l1=cat([d[1] for d in divs], np.int32), div_l1_off=offs([d[1] for d in divs]),
                            div_rng=cat([d[2] for d in divs], np.int32).reshape(-1, 2), div_rng_off=offs([d[2] for d in divs]),
                            div_mode=np.array(modes, np.int32), div_in_tree=np.array(in_tree, np.int32), united0=np.asarray(united[0], np.int32).reshape(-1, 2),
                            united1=np.asarray(united[1], np.int32).reshape(-1, 2), **g)
    print("%-22s %2d x %3d, thr %4g: %2d divisions, modes %s, most ranges in a division %d, united %s"
          % (name, many, ln, thr, len(divs), {cl.MODE_NAME[m] + str(m): modes.count(m) for m in sorted(set(modes))}, most, united[0]))


def timed(repeats):
    """the reference's own Ssrel::consreg(msd, DISSIM) on one core: a fresh Ssrel per run, so the tree is built every time, as in prrn"""
    import consreglib as cl
    out = {}
    big = np.load(os.path.join(ROOT, "tests", "golden", "msa", "prog256x1024.npz"))["codes"]
    small = dict(cl.fixtures())["prot16_pf"]["codes"]
    ref = Ref(1)
    dec = np.array(list("?-X" + _AA + "BZ"))
    for name, codes in (("prog256x1024", big), ("prot16_pf", small)):
        rows = ["".join(dec[codes[:, m]]) for m in range(codes.shape[1])]
        sd = ref.R.group(["m%d" % i for i in range(len(rows))], rows)
        ts = []
        for r in range(repeats + 1):
            ssrel = (C.c_char * 256)()
            t0 = time.perf_counter()
            p = ref.consreg(C.addressof(ssrel), sd, 1)
            ts.append((time.perf_counter() - t0) * 1e3)
        ts = ts[1:]
        # every division, whatever the intersection: extseq of both sons + constwo, as consreg's loop does without its early stop
        tree = ref.tree(ssrel, codes.shape[1])
        t0 = time.perf_counter()
        ndiv = 0
        for lists in cl.divisions(tree[0], tree[1], tree[2], codes.shape[1]):
            sons = (C.c_void_p * 2)()
            for s in range(2):
                lst = (C.c_int * (len(lists[s]) + 1))(*(list(lists[s]) + [-1]))
                sons[s] = ref.extseq(sd, None, lst, CPY_SEQ + CPY_NBR, 1.0)
            ref.constwo(C.addressof(ssrel), sons)
            for s in range(2):
                ref.L.ref_group_free(sons[s])
            ndiv += 1
        all_ms = (time.perf_counter() - t0) * 1e3
        out[name] = {"all_divisions_ms": round(all_ms, 1), "divisions": ndiv, "members": codes.shape[1], "columns": codes.shape[0], "ms_median": round(float(np.median(ts)), 2), "ms_min_max": [round(min(ts), 2), round(max(ts), 2)],
                     "runs": repeats, "dissim_ranges": [list(r) for r in ref.ranges(p)]}
    print(json.dumps({"reference_consreg_one_core": out}))


W16 = [0.4 + 0.1 * ((7 * i) % 13) for i in range(12)]
JOBS = {
    "prot_ng": lambda: run("prot8_ng", 1, ungapped(8, 160, 71)),
    "prot_nv": lambda: run("prot6_nv", 1, family(6, 140, 72, indel=0.03, sub=0.15)),
    "prot_hf": lambda: run("prot12_hf", 1, with_clean_members(family(12, 200, 73, indel=0.02, sub=0.12), (0, 5, 9)), swapped_too=True),
    "prot_pf": lambda: run("prot16_pf", 1, family(16, 230, 74, indel=0.02, sub=0.12)),
    "dna": lambda: run("dna10", 2, family(10, 240, 75, dna=True, indel=0.02, sub=0.1)),
    "prot_weighted": lambda: run("prot12_weighted", 1, family(12, 180, 76, indel=0.02, sub=0.12), weight=W16),
    "prot_uv": lambda: run("prot10_u2_v6", 1, family(10, 220, 77, indel=0.02, sub=0.12), u=2., v=6.),
    "prot_empty": lambda: run("prot8_empty", 1, with_outlier(family(8, 220, 78, indel=0.015, sub=0.06), 3, 79), want_empty=True),
}

if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--time":
        timed(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    elif len(sys.argv) > 1:
        JOBS[sys.argv[1]]()
    else:
        for j in JOBS:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), j])
