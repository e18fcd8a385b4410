"""The strips' column-score blocks (simblk_fill / simblk_fill_block, csrc/g2g_strip.h) against the oracle.

A strip in sweep mode makes PwdM::sim2 of its cells itself, 64 rows x 64 columns at a time.  v6 fills its blocks through the
block scorer (sim2_block, csrc/g2g_kernels.hip): the scorer is picked once per block, what depends on the column stays in
registers, what is wave-uniform is read with a lane per element, and the sums run in the reference's order.  v2, v3 / v3r, v7
and v8 call sim2 cell by cell.  Either way every DP must give the oracle's score bit for bit and its traceback, whatever scorer
the pair selects and whichever strip family fills the block.

Inputs: a synthetic family (prrn_aln_amd/synth.py) split into two groups; the first group is cut to its first 70
columns, so that the DP has two strips, the second with 6 rows, and 200 or more columns: block indices 0-3, the third buffer
reused, the last block partial.  The narrow-band case keeps both groups whole (sh = -10: a band of under two blocks over
six strips, both edges running through blocks).  CASES lists, per input, the scorer it was built for (checked on the CPU with the host
builders before it was committed, and asserted here) and the record type (alnmode 6 NGP -> v7, 7 / 8 half profiles -> v3 / v3r,
9 profiles -> v6 or v2, 10 NTV -> v8).  sim2 kinds 13 and 11 come with NGP pairs only (v7); 210 / 120 are the unweighted twins
of 211 / 121.  NOT covered: a second chunk of column residues (more than SB_CR = 32 members on b with a 12x / 22x / 32x
scorer).  The selection (advised_sim2) leaves 32x for 33 as soon as b has about as many members as the alphabet has elements
(34 x 32 and 34 x 33 members give 33 here, 33 x 2 and 40 x 3 give 321 with b the small group), and the matrix scorers belong
to groups of a few members, so no small family reaches it; 23 vector entries do cross the chunk of G2G_SIMBLK_VC entries when
that is smaller."""
import numpy as np
import pytest

import oraclelib
from prrn_aln_amd import engine, operator as op
from prrn_aln_amd.synth import DNA, PROTEIN, make_family, tree_weights

pytestmark = pytest.mark.gpu
GAP = 1

# name: (members of the first group, of the second, weighted, indel rate, DNA, AlnParam overrides, rows of the first group) -> (sim2_kind, alnmode)
CASES = {
    # profiles on both sides of the DP (_pf): v6 and v2
    "pf321_b2": ((12, 2, True, 0.01, False, {}, 70), (321, 9)),
    "pf321_b4": ((6, 4, True, 0.03, False, {}, 70), (321, 9)),
    "pf321_b5": ((6, 5, True, 0.03, False, {}, 70), (321, 9)),
    "pf321_b8": ((8, 8, True, 0.03, False, {}, 70), (321, 9)),
    "pf321_b9": ((10, 9, True, 0.03, False, {}, 70), (321, 9)),
    "pf320_b5": ((6, 5, False, 0.03, False, {}, 70), (320, 9)),
    "pf320_b9": ((10, 9, False, 0.03, False, {}, 70), (320, 9)),
    "pf321_narrow": ((6, 5, True, 0.03, False, {"sh": -10}, None), (321, 9)),
    "pf321_ls3": ((6, 5, True, 0.03, False, {"ls": 3}, 70), (321, 9)),
    "pf221": ((6, 2, True, 0.03, False, {}, 70), (221, 9)),
    "pf220": ((6, 2, False, 0.03, False, {}, 70), (220, 9)),
    "pf33": ((34, 32, True, 0.01, False, {}, 70), (33, 9)),
    "pf330": ((24, 24, True, 0.01, True, {}, 70), (330, 9)),
    # a profile against residues (_hf): v3 / v3r with a scorer they cannot read in place
    # (the gap-free pair of members, cut to 70 columns, becomes b: 317 rows in five strips, two blocks, the second partial)
    "hf321": ((2, 16, True, 0.01, False, {}, 70), (321, 8)),
    "hf320": ((2, 16, False, 0.01, False, {}, 70), (320, 8)),
    # no gaps on either side (NGP): v7
    "ngp231": ((3, 9, True, 0.0, False, {}, 70), (231, 6)),
    "ngp230": ((3, 9, False, 0.0, False, {}, 70), (230, 6)),
    "ngp231_dna": ((3, 9, True, 0.0, True, {}, 70), (231, 6)),
    "ngp33": ((34, 32, True, 0.0, False, {}, 70), (33, 6)),
    "ngp330": ((24, 24, True, 0.0, True, {}, 70), (330, 6)),
    "ngp321": ((33, 2, True, 0.0, False, {}, 70), (321, 6)),
    "ngp13": ((1, 9, True, 0.0, False, {}, 70), (13, 6)),
    "ngp11": ((1, 1, True, 0.0, False, {}, 70), (11, 6)),
    # small groups with gaps (NTV): v8
    "ntv221": ((2, 3, True, 0.01, False, {}, 70), (221, 10)),
    "ntv220": ((2, 3, False, 0.01, False, {}, 70), (220, 10)),
    "ntv121": ((1, 3, True, 0.01, False, {}, 70), (121, 10)),
    "ntv120": ((1, 3, False, 0.01, False, {}, 70), (120, 10)),
    "ntv211": ((3, 1, True, 0.01, False, {}, 70), (211, 10)),
    "ntv210": ((3, 1, False, 0.01, False, {}, 70), (210, 10)),
    "ntv221_ls3": ((2, 3, True, 0.01, False, {"ls": 3}, 70), (221, 10)),
}
# forced selection (the options of tests/test_gpu_paths.py) -> the family g2g_batch_paths must report, per alnmode
CONFIGS = {
    "v6": ({"G2G_V6_MIN_STRIPS": "0"}, {9: 6}),
    "v2": ({"G2G_FORCE_V2": "1"}, {9: 2, 7: 2, 8: 2}),
    "default": ({}, {7: 3, 8: 3, 6: 7, 10: 8}),
    "v3lds": ({"G2G_NO_AREG": "1"}, {7: 3, 8: 3}),
}
RUNS = [(c, n) for c, (_, fam) in CONFIGS.items() for n, (_, (_, mode)) in CASES.items() if mode in fam]


def build_case(name):
    """-> (PwdM, its two groups): the host builders only, no device"""
    (na, nb, weighted, indel, dna, akw, rows), _ = CASES[name]
    fam = make_family(na + nb, 210, 5, alphabet=DNA if dna else PROTEIN, indel=indel, max_indel=6)
    alp = op.AlnParam(molc=op.DNA, max_code=17, **akw) if dna else op.AlnParam(**akw)
    codes = op.encode(fam.msa, alp.molc)
    w = np.asarray(tree_weights(fam.tree, na + nb)) if weighted else None
    gs = []
    for idx, cut in ((list(range(na)), rows), (list(range(na, na + nb)), None)):
        g = codes[:, idx]
        g = np.ascontiguousarray(g[(g != GAP).any(axis=1)][:cut])
        gs.append(op.mSeq(g, alp, None if w is None else w[idx]))
    return op.PwdM(gs, alp), gs


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def L():
    return oraclelib.load()


@pytest.fixture(scope="module")
def built(L):
    """name -> (PwdM, groups, the oracle's (score, cells, traceback)): built once, read by every run"""
    out = {}

    def get(name):
        if name not in out:
            pw, gs = build_case(name)

            class H:
                c = pw.problem
            out[name] = (pw, gs, oraclelib.forward(L, H))
        return out[name]
    return get


@pytest.fixture(autouse=True)
def _fresh_options(ctx):
    ctx.reset_options()
    yield
    ctx.reset_options()


def geometry(q):
    """(rows, rows of the last strip, columns, blocks of the first strip, columns of its last block)"""
    rows, cols = q.a.right - q.a.left, q.b.right - max(q.b.left, q.a.left + q.lw)
    return rows, rows % 64, q.b.right - q.b.left, (cols + 63) // 64, cols % 64


@pytest.mark.parametrize("config,name", RUNS, ids=["%s-%s" % r for r in RUNS])
def test_block_scorer(ctx, built, monkeypatch, config, name):
    opts, fams = CONFIGS[config]
    for k in {k for o, _ in CONFIGS.values() for k in o}:
        monkeypatch.delenv(k, raising=False)
    for k, v in opts.items():
        ctx.set_option(k, v)
    pw, _, (oscr, ocells, otr) = built(name)
    q = pw.problem
    kind, mode = CASES[name][1]
    assert (q.sim2_kind, pw.alnmode) == (kind, mode), (name, q.sim2_kind, pw.alnmode)
    assert q.noll == (3 if CASES[name][0][5].get("ls") == 3 else 2)
    rows, last, cols, blocks, tail = geometry(q)
    assert rows > 64 and 0 < last < 64 and tail != 0, (name, rows, last, cols, blocks, tail)
    assert (cols >= 200 and blocks >= 4) or mode == 8, (name, cols, blocks)
    if "narrow" in name:                                   # the band is narrower than two blocks: both its edges run through blocks
        assert q.up - q.lw + 1 < 128 and rows > 128

    class H:
        c = q
    batch = ctx.prepare([H])
    try:
        chosen = batch.paths()
        batch.run()
        (scr, cells, tr, st), = batch.fetch()
        ran = batch.paths()
    finally:
        batch.free()
    assert st == 0
    assert chosen == ran == [fams[mode]], (name, config, chosen, ran)
    assert scr == oscr, (name, config, kind, scr, oscr)
    assert np.array_equal(tr, otr)
