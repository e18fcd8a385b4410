"""Inputs of tests/test_gpu_intron_nv.py: the committed goldens of the naive record type (DPunit_nv, mode NTV_ALB) with
synthetic exon-boundary annotations in the style of intronlib.annotate, the boundary rows chosen for the 64-row strips of
g2g_v8_ntv{2,3}_ib.  Expected scores and tracebacks never come from here: they are oracle/g2g_oracle.c's."""
from __future__ import annotations

import ctypes as C

import numpy as np

import intronlib as il

# (golden, rows, crg kind, Noll, interior column): each spans two 64-row strips; together every crg kind that occurs and both
# Noll values.  The interior column is one the plain optimal path visits in rows 62 .. 65, where a bonus of this size changes
# the score by more than cell (0, 0)'s share and, in three of the five, the traceback (found with the oracle)
NV = [("dna3x100_ls3_b2", 115, 120, 3, 66), ("dna_ls3_4x70_w21_s1", 83, 211, 3, 59), ("syn5x90_b3", 106, 121, 2, 78),
      ("syn5x90_b4", 108, 221, 2, 80), ("syn4x80_unw_b2", 72, 220, 2, 63)]
NTV_ALB = 10
# rows that get a boundary: the DP's first row, a row inside the first strip, the last two rows of the first strip, the first
# two of the second and (appended below) the last row
ROWS = [0, 31, 62, 63, 64, 65]
APH = [0, 1, 0, 2, 0, 1, 0]                                     # codon phase of each boundary (step 3)
INTERIOR = 40                                                   # a second interior column: in the band of rows 31 .. 65 in every golden above
BPH = [0, 1, 0, 0, 2]


def columns(d: dict, interior: int):
    al, ar, bl, br, lw, up = il.geometry(d)
    cols = sorted({0, min(up, br - 1), br - 1, INTERIOR, interior})    # first / last in-band column of row 0, the last column
    assert len(cols) == 5
    return cols


def annotate(d: dict, interior: int, variant: str = "plain") -> dict:
    """d with pfq_pos / pfq_dns / pfq_step on both sides and spb_fact > 0.  Variants: "stuck" -- two a-side boundaries inside
    the codon of row 63 (the reference's cursor never catches up: rows 64 and later get nothing; protein only); "early" -- a
    first a-side boundary before a.left's codon (a.left moved to row 2: the walk has to skip it)."""
    al, ar, bl, br, lw, up = il.geometry(d)
    assert al == 0 and bl == 0 and 65 < ar - 1 <= 127             # two 64-row strips
    step = 1 if int(d["a_molc"][0]) == 2 else 3                 # nucleotide columns / codons
    rows = ROWS + [ar - 1]
    apos = [m * step + (ph if step == 3 else 0) for m, ph in zip(rows, APH)]
    if variant == "stuck":
        assert step == 3
        k = rows.index(63)
        apos = apos[:k] + [63 * 3, 63 * 3 + 1] + apos[k + 1:]
    bpos = [n * step + (ph if step == 3 else 0) for n, ph in zip(columns(d, interior), BPH)]
    e = dict(d)
    e["a_pfq_pos"] = np.array(apos, np.int32); e["b_pfq_pos"] = np.array(bpos, np.int32)
    e["a_pfq_dns"] = np.array([0.5 + 0.25 * (i % 3) for i in range(len(apos))]); e["b_pfq_dns"] = np.array([1.0 + 0.5 * (j % 2) for j in range(len(bpos))])
    e["a_pfq_step"] = np.array([step], np.int32); e["b_pfq_step"] = np.array([step], np.int32)
    e["spb_fact"] = np.array([il.SPB_FACT])
    if variant == "early":
        e["a_left"] = np.array([2], e["a_left"].dtype)
    return e


def library_bonus_cells(L, holder):
    """[(m, n, h, mx)] as g2g_bonus_cells (host code of libg2g.so: the table the strips read) lists them"""
    L.g2g_bonus_cells.argtypes = [C.POINTER(type(holder.c)), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                  C.POINTER(C.c_double), C.POINTER(C.c_double)]
    cnt = L.g2g_bonus_cells(C.byref(holder.c), 0, None, None, None, None)
    cap = max(cnt, 1)
    m, n, bh, bx = (C.c_int32 * cap)(), (C.c_int32 * cap)(), (C.c_double * cap)(), (C.c_double * cap)()
    assert L.g2g_bonus_cells(C.byref(holder.c), cap, m, n, bh, bx) == cnt
    return [(m[k], n[k], bh[k], bx[k]) for k in range(cnt)]


class Held:
    """a g2g_problem made by the level-1 host builders, with what it points to"""

    def __init__(self, pwdm, keep):
        self.c, self.keep = pwdm.problem, (pwdm, keep)


def three_strips(dna: bool):
    """An annotated _nv DP of three 64-row strips (no committed golden is that tall): a division of four synthetic members
    (prrn_aln_amd/synth.py) through the level-1 host builders, as tests/test_gpu_fullsize.py builds its inputs -- (2, 2)
    protein members, crg22w, Noll 2; (1, 3) DNA members under -yl3, Noll 3.  Boundaries in the rows either side of both strip
    boundaries, in the first and the last row, in columns on the diagonal of those rows."""
    from prrn_aln_amd import operator as op, sweep
    from prrn_aln_amd.synth import DNA, make_family, tree_branches, tree_weights
    if dna:
        fam = make_family(4, 150, 2, alphabet=DNA, indel=0.012, max_indel=8)
        alp = op.AlnParam(ls=3, molc=op.DNA, max_code=17)
    else:
        fam = make_family(4, 150, 3)
        alp = op.AlnParam()
    codes = op.encode(fam.msa, alp.molc)
    w = np.asarray(tree_weights(fam.tree, 4))
    side = [s for s in tree_branches(fam.tree) if len(s) == (1 if dna else 2)][0]
    a, b, ia, ib = sweep.division_groups(codes, side)
    ga, gb = op.mSeq(a, alp, w[ia]), op.mSeq(b, alp, w[ib])
    pw = op.PwdM([ga, gb], alp)
    q = pw.problem
    assert pw.alnmode == NTV_ALB and q.a.left == 0 and q.b.left == 0 and 129 <= q.a.right <= 192
    step = 1 if dna else 3
    rows = [0, 63, 64, 65, 127, 128, q.a.right - 1]
    cols = sorted({0, min(q.up, q.b.right - 1), q.b.right - 1} | {m for m in rows[1:-1] if m != 65})
    apos = np.array([m * step + (ph if step == 3 else 0) for m, ph in zip(rows, APH)], np.int32)
    bpos = np.array([n * step + (ph if step == 3 else 0) for n, ph in zip(cols, [0, 0, 0, 0, 0, 1, 0])], np.int32)
    adns = np.array([0.5 + 0.25 * (i % 3) for i in range(len(apos))]); bdns = np.array([1.0 + 0.5 * (j % 2) for j in range(len(bpos))])
    for s, pos, dns in ((q.a, apos, adns), (q.b, bpos, bdns)):
        s.npfq = len(pos); s.pfq_step = step
        s.pfq_pos = pos.ctypes.data_as(C.POINTER(C.c_int32)); s.pfq_dns = dns.ctypes.data_as(C.POINTER(C.c_double))
    q.spb_fact = il.SPB_FACT
    return Held(pw, (ga, gb, apos, bpos, adns, bdns))
