"""Inputs of tests/test_gpu_intron_strips.py: the annotated reference goldens, synthetic exon-boundary annotations on
unannotated goldens of the gap-state record types, and a Python restatement of the walk that decides WHICH cells get the
intron-position bonus (reference src/fwd2c.h:367-370,378-379,446-452,472; PfqItr src/gsinfo.h:132-231).  The restatement is
used to check where the synthetic annotations put their cells -- never for an expected score or traceback: those come from
the committed goldens and from oracle/g2g_oracle.c."""
from __future__ import annotations

import glob
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INTRON = sorted(glob.glob(os.path.join(GOLD, "intron_*.npz")))
# the smallest unannotated goldens of each record type with gap state and at least 50 rows: (name, variant)
#   prot12x80_tgapf05_k1  RHF, Noll 2 (g2g_v2_hf2_ib)      prot12x80_tgapf05_k6  GPF, Noll 2 (g2g_v2_pf2_ib)
#   dna16x100_ls3_k7      GPF, Noll 3, -yl3 (g2g_v2_pf3_ib) dna16x100_ls3_k1      RHF, Noll 3, -yl3 (g2g_v2_hf3_ib)
# "stuck": two a-side boundaries inside one codon -- the reference's cursor never catches up, no later row gets a bonus
SYNTH = [("prot12x80_tgapf05_k1", "plain"), ("prot12x80_tgapf05_k6", "plain"), ("dna16x100_ls3_k7", "plain"),
         ("dna16x100_ls3_k1", "plain"), ("prot12x80_tgapf05_k6", "stuck")]
SPB_FACT = 20.0                 # SpbFact as the annotated reference goldens have it
# rows that get a boundary: first / last row of the 16- and of the 32-row strips of the 8-lanes-per-cell kernel and the rows
# either side of their boundaries, the DP's first and (appended below) last row
ROWS = [0, 15, 16, 31, 32, 33, 47, 48]
STUCK_ROW = 32


def load(name: str) -> dict:
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


def geometry(d: dict):
    return (int(d["a_left"][0]), int(d["a_right"][0]), int(d["b_left"][0]), int(d["b_right"][0]), int(d["wdw_lw"][0]), int(d["wdw_up"][0]))


def annotate(d: dict, variant: str = "plain") -> dict:
    """d with pfq_pos / pfq_dns / pfq_step on both sides and spb_fact > 0"""
    al, ar, bl, br, lw, up = geometry(d)
    assert al == 0 and bl == 0 and ar - al >= 50
    step = 1 if int(d["a_molc"][0]) == 2 else 3                 # nucleotide columns / codons
    rows = ROWS + [ar - 1]
    aph = [0, 1, 0, 2, 0, 1, 0, 0, 0]                           # codon phase of each boundary (step 3)
    apos = [m * step + (ph if step == 3 else 0) for m, ph in zip(rows, aph)]
    if variant == "stuck":
        assert step == 3
        k = rows.index(STUCK_ROW)
        apos = apos[:k] + [STUCK_ROW * 3, STUCK_ROW * 3 + 1] + apos[k + 1:]
    # column 0 / `up`: first / last in-band column of row 0; br - 1: last column of the last row; 39: cell (32, 39) lies on the
    # optimal path of prot12x80_tgapf05_k6 where a bonus of this size moves the traceback (found with the oracle)
    cols = sorted({0, 5, 22, 39, min(up, br - 1), br - 1})
    assert len(cols) == 6
    bph = [0, 1, 0, 0, 2, 0]
    bpos = [n * step + (ph if step == 3 else 0) for n, ph in zip(cols, bph)]
    e = dict(d)
    e["a_pfq_pos"] = np.array(apos, np.int32); e["b_pfq_pos"] = np.array(bpos, np.int32)
    e["a_pfq_dns"] = np.array([0.5 + 0.25 * (i % 3) for i in range(len(apos))]); e["b_pfq_dns"] = np.array([1.0 + 0.5 * (j % 2) for j in range(len(bpos))])
    e["a_pfq_step"] = np.array([step], np.int32); e["b_pfq_step"] = np.array([step], np.int32)
    e["spb_fact"] = np.array([SPB_FACT])
    return e


def unannotated(d: dict) -> dict:
    e = {k: v for k, v in d.items() if "pfq" not in k}
    e["spb_fact"] = np.array([0.0])
    return e


def _in_codon(pos, step, col):
    return pos == col if step == 1 else col * step <= pos < col * step + step


def bonus_cells(d: dict):
    """[(m, n, h, mx)]: the cells that receive the bonus, row-major"""
    al, ar, bl, br, lw, up = geometry(d)
    ap, bp = [int(x) for x in d["a_pfq_pos"]], [int(x) for x in d["b_pfq_pos"]]
    ad, bd = d["a_pfq_dns"], d["b_pfq_dns"]
    sa, sb, fact = int(d["a_pfq_step"][0]), int(d["b_pfq_step"][0]), float(d["spb_fact"][0])
    out = []
    ka = 0
    while ka < len(ap) and ap[ka] < al * sa:
        ka += 1
    for m in range(al, ar):
        if ka >= len(ap):
            break
        if not _in_codon(ap[ka], sa, m):
            continue
        n0, n9 = max(m + lw, bl), min(m + up + 1, br)
        kb = 0
        while kb < len(bp) and bp[kb] < n0 * sb:
            kb += 1
        for n in range(n0, n9):
            if kb >= len(bp):
                break
            if not _in_codon(bp[kb], sb, n):
                continue
            phase = sa == 1 or (ap[ka] - bp[kb]) % sa == 0
            v = fact * float(ad[ka]) * float(bd[kb])
            out.append((m, n, v if phase else 0.0, v if phase and (sa == 1 or ap[ka] % sa == 0) else 0.0))
            kb += 1
        ka += 1
    return out
