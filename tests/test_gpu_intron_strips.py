"""The intron-position bonus (forwardB, reference src/fwd2c.h:446-452) on the strip kernels: annotated DPs run on the
bonus-aware instantiations of v7 (no gap state) and v2 (gap state), and g2g_batch_paths says so.  Expected values are the
committed reference goldens and oracle/g2g_oracle.c (pinned bit-exact on the annotated goldens by tests/test_oracle_golden.py),
never this library's own output.  Runs only on the GPU box (-m gpu)."""
import os

import numpy as np
import pytest

import intronlib as il
import oraclelib
from prrn_aln_amd import _abi, engine

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return oraclelib.load()


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def gold():
    """the seven annotated reference goldens: (name, arrays, expected generation)"""
    assert len(il.INTRON) == 7
    out = []
    for f in il.INTRON:
        d = dict(np.load(f))
        mode = int(d["alnmode"][0])
        assert mode in (6, 7)                               # NGP_ALB (single sequences), HLF_ALB (group against sequence): both modes v7 / v2 take
        out.append((os.path.basename(f)[:-4], d, 7 if mode == 6 else 2))
    assert [g for _, _, g in out].count(7) == 5 and [g for _, _, g in out].count(2) == 2
    return out


@pytest.fixture(scope="module")
def synth(L):
    """synthetic annotations on gap-state goldens: (name, annotated arrays, oracle score, oracle trace, oracle score and trace
    without the annotation) -- computed once, shared"""
    out = []
    for name, variant in il.SYNTH:
        d = il.load(name)
        e = il.annotate(d, variant)
        scr, _, tr = oraclelib.forward(L, _abi.problem_from_arrays(e))
        scr0, _, tr0 = oraclelib.forward(L, _abi.problem_from_arrays(il.unannotated(d)))
        assert scr0 == d["scr"][0] and np.array_equal(tr0, d["vmf_trace"])          # the oracle on the plain input: the golden
        out.append((name + ":" + variant, e, scr, tr, scr0, tr0))
    return out


def run(ctx, arrays):
    """(paths after prepare, paths after run, results, g2g_result::rr of every result) of one batch"""
    hs = [_abi.problem_from_arrays(d) for d in arrays]
    batch = ctx.prepare(hs)
    try:
        p0 = batch.paths()
        batch.run()
        res = batch.fetch()
        return p0, batch.paths(), res, batch.last_rr
    finally:
        batch.free()


def check_gold(gold, res, rr):
    """score, rr and traceback records of the golden"""
    assert len(res) == len(gold) and len(rr) == len(gold)
    for (name, d, _), (scr, cells, tr, st), r in zip(gold, res, rr):
        assert st == 0 and scr == d["scr"][0], (name, st, scr, float(d["scr"][0]))
        assert list(r) == [int(x) for x in d["homscore_rr"]], (name, r, d["homscore_rr"])
        assert np.array_equal(tr, d["vmf_trace"]), name


def check_synth(synth, res):
    for (name, e, scr, tr, _, _), (gscr, cells, gtr, st) in zip(synth, res):
        assert st == 0 and gscr == scr, (name, st, gscr, scr)
        assert np.array_equal(gtr, tr), name


def test_goldens_on_the_strips(ctx, gold):
    """1. default options: score, rr and traceback records equal the goldens, the single-sequence pairs report v7, the
    group-against-sequence cases v2"""
    hs = [_abi.problem_from_arrays(d) for _, d, _ in gold]
    batch = ctx.prepare(hs)
    want = [g for _, _, g in gold]
    assert batch.paths() == want
    batch.run()
    res = batch.fetch()
    rr = batch.last_rr
    assert batch.paths() == want
    batch.free()
    check_gold(gold, res, rr)


def test_synthetic_annotations_cover_the_cases(synth):
    """2a. where the synthetic annotations put their cells (the walk restated in intronlib.bonus_cells), and that they matter"""
    differs = 0
    for name, e, scr, tr, scr0, tr0 in synth:
        al, ar, bl, br, lw, up = il.geometry(e)
        cells = il.bonus_cells(e)
        at = {(m, n) for m, n, _, _ in cells}
        rows = {m for m, _ in at}
        if name.endswith(":stuck"):
            # two a-side boundaries in the codon of row 32: the second is never reached, rows 33, 47, 48 and the last get nothing
            assert rows == {0, 15, 16, 31, 32}
        else:
            assert rows == set(il.ROWS) | {ar - 1}                  # first / last rows of 16- and 32-row strips, either side of their boundaries
            assert (ar - 1, br - 1) in at                           # last in-band column of the last row
        assert ar - al >= 3 * 32 + 1                                # three or more strips, 16 or 32 rows each
        assert (0, 0) in at and max(0 + lw, bl) == 0                # first in-band column of row 0
        assert (0, min(up, br - 1)) in at                           # last in-band column of row 0
        if int(e["a_pfq_step"][0]) == 3:
            assert any(h == 0 and mx == 0 for _, _, h, mx in cells)     # phase mismatch
            assert any(h > 0 and mx == 0 for _, _, h, mx in cells)      # in phase, off the codon start
        assert any(h > 0 and mx > 0 for _, _, h, mx in cells)
        assert scr != scr0, name                                    # the annotation changes every score ...
        differs += not np.array_equal(tr, tr0)
    assert differs >= 1                                             # ... and at least one traceback


def test_synthetic_annotations_on_gap_state_dps(ctx, synth):
    """2b. _hf / _pf, Noll 2 and 3, with synthetic annotations: bit-equal to the oracle, on v2"""
    p0, p1, res, _ = run(ctx, [e for _, e, _, _, _, _ in synth])
    assert p0 == [2] * len(synth) and p1 == p0
    check_synth(synth, res)


def test_synthetic_annotations_16_row_strips(gold, synth):
    """2c. the same with 16-row strips (the workgroup size a full sweep picks)"""
    c = engine.Context(options={"V2_THREADS": "128"})
    try:
        p0, p1, res, rr = run(c, [e for _, e, _, _, _, _ in synth] + [d for _, d, g in gold if g == 2])
    finally:
        c.close()
    assert p1 == [2] * len(p1)
    check_synth(synth, res[:len(synth)])
    check_gold([g for g in gold if g[2] == 2], res[len(synth):], rr[len(synth):])


@pytest.mark.parametrize("opt", ["NO_STRIP_BONUS", "FORCE_V1"])
def test_same_inputs_on_v1(gold, synth, opt):
    """3. the same inputs with the strips' bonus switched off / everything on g2g_forward_kernel: same results, path 1"""
    c = engine.Context(options={opt: "1"})
    try:
        p0, p1, res, rr = run(c, [d for _, d, _ in gold] + [e for _, e, _, _, _, _ in synth])
    finally:
        c.close()
    assert p0 == [1] * len(p0) and p1 == p0
    check_gold(gold, res[:len(gold)], rr[:len(gold)])
    check_synth(synth, res[len(gold):])


def test_mixed_batch(ctx, gold, synth):
    """4. annotated and unannotated DPs of the same record types in one batch: the unannotated ones run where they run alone
    and equal their goldens, the annotated ones are as above"""
    plain_names = ["syn2x120_pair", "prot12x80_tgapf05_k1", "prot12x80_tgapf05_k6", "dna16x100_ls3_k7", "dna16x100_ls3_k1"]
    plain = [il.load(n) for n in plain_names]
    alone = []
    for d in plain:
        b = ctx.prepare([_abi.problem_from_arrays(d)])
        alone += b.paths()
        b.free()
    # (2 among them: v6 takes `_pf` DPs only in batches of 35 strips per CU and more -- a sweep; in a batch this small they run
    #  on v2 whether annotated or not, on the instantiation without the bonus)
    assert alone[0] == 7 and all(g in (2, 3, 6) for g in alone[1:])        # never v1
    arrays, idx = [], {"g": [], "s": [], "p": []}
    groups = (("g", [d for _, d, _ in gold]), ("s", [e for _, e, _, _, _, _ in synth]), ("p", plain))
    for k in range(max(len(x) for _, x in groups)):                           # interleaved
        for key, x in groups:
            if k < len(x):
                idx[key].append(len(arrays))
                arrays.append(x[k])
    p0, p1, res, rr = run(ctx, arrays)
    assert p1 == p0
    assert [p1[i] for i in idx["g"]] == [g for _, _, g in gold]
    assert [p1[i] for i in idx["s"]] == [2] * len(synth)
    assert [p1[i] for i in idx["p"]] == alone
    check_gold(gold, [res[i] for i in idx["g"]], [rr[i] for i in idx["g"]])
    check_synth(synth, [res[i] for i in idx["s"]])
    for d, i, n in zip(plain, idx["p"], plain_names):
        scr, cells, tr, st = res[i]
        assert st == 0 and scr == d["scr"][0] and np.array_equal(tr, d["vmf_trace"]), n


@pytest.mark.parametrize("victim", [0, 1])
def test_recovery_of_annotated_dps(gold, synth, victim):
    """The recovery path with annotated DPs (test hook INJECT_STALL, as tests/test_gpu_edges.py uses it): the victim's first strip
    waits for a flag nobody writes, loses its wait and is re-run inside g2g_batch_run.  Victim 1 is re-run on the strips (a
    one-DP batch in which the hook names nobody) and reports that kernel; victim 0 is DP 0 of its retry batch too, stalls
    again and ends on g2g_forward_kernel, the last resort: g2g_batch_paths reports 1 for it.  Results: the goldens / the oracle."""
    g = [x for x in gold if x[0] in ("intron_ce13a1_ce13a2", "intron_ce13a_msa_ce13a1")]
    s = [x for x in synth if x[0] == "prot12x80_tgapf05_k6:plain"]
    order = [g[0][1], s[0][1], g[1][1]]                               # v7-bonus, v2-bonus (_pf), v2-bonus (_hf)
    c = engine.Context(options={"INJECT_STALL": str(victim), "WAIT_LIMIT_MS": "300"})
    try:
        p0, p1, res, rr = run(c, order)
        cnt = c.counters()
    finally:
        c.close()
    assert p0 == [7, 2, 2]
    assert p1 == ([1, 2, 2] if victim == 0 else [7, 2, 2])
    assert cnt["recovered_dps"] == (2 if victim == 0 else 1) and cnt["recovered_on_v1"] == (1 if victim == 0 else 0)
    check_gold(g, [res[0], res[2]], [rr[0], rr[2]])
    check_synth(s, [res[1]])


def test_ce13a_table_spans_strips(gold):
    """5. configs[0]'s 518 x 520 DP is 9 strips of 64 rows on v7 and its bonus table has cells in at least three of them: the per-row
    index is exercised across strips (the DP itself runs in test 1)"""
    d = [d for n, d, _ in gold if n == "intron_ce13a1_ce13a2"][0]
    al, ar, bl, br, lw, up = il.geometry(d)
    assert (ar - al, br - bl) == (518, 520) and (ar - al + 63) // 64 == 9
    cells = il.bonus_cells(d)
    assert len({(m - al) // 64 for m, _, _, _ in cells}) >= 3
    assert any(h > 0 and mx > 0 for _, _, h, mx in cells) and any(h > 0 and mx == 0 for _, _, h, mx in cells)
