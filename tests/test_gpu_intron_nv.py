"""The intron-position bonus (forwardB, reference src/fwd2c.h:446-452) on the strips of the naive record type: annotated
DPunit_nv DPs (mode NTV_ALB) run on g2g_v8_ntv{2,3}_ib, and g2g_batch_paths says so.  Expected scores and tracebacks are
oracle/g2g_oracle.c's (it restates the bonus inside the generic forwardB) and, for the unannotated twins, the committed
goldens -- never this library's own output.  The GPU cases run only on the GPU box (-m gpu); the annotation checks are CPU."""
import ctypes as C

import numpy as np
import pytest

import intron_nvlib as nv
import intronlib as il
import oraclelib
from prrn_aln_amd import _abi, engine

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    return oraclelib.load()


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


@pytest.fixture(scope="module")
def synth(L):
    """the five goldens annotated: (name, plain arrays, annotated arrays, oracle score, oracle trace) -- computed once, shared"""
    out = []
    for name, rows, crg, noll, col in nv.NV:
        d = il.load(name)
        assert int(d["alnmode"][0]) == nv.NTV_ALB and int(d["a_right"][0]) == rows
        assert int(d["crg2_kind"][0]) == crg and int(d["Noll"][0]) == noll
        e = nv.annotate(d, col)
        scr, _, tr = oraclelib.forward(L, _abi.problem_from_arrays(e))
        scr0, _, tr0 = oraclelib.forward(L, _abi.problem_from_arrays(il.unannotated(d)))
        assert scr0 == d["scr"][0] and np.array_equal(tr0, d["vmf_trace"])          # the oracle on the plain input: the golden
        out.append((name, d, e, scr, tr))
    return out


@pytest.fixture(scope="module")
def tall(L):
    """two three-strip DPs (nv.three_strips): (problem, oracle score, oracle trace, oracle score without the annotation)"""
    out = []
    for dna in (False, True):
        h = nv.three_strips(dna)
        scr, _, tr = oraclelib.forward(L, h)
        h.c.spb_fact = 0.0
        scr0, _, _ = oraclelib.forward(L, h)
        h.c.spb_fact = il.SPB_FACT
        out.append((h, scr, tr, scr0))
    return out


def holders(synth, tall):
    return [_abi.problem_from_arrays(e) for _, _, e, _, _ in synth] + [h for h, _, _, _ in tall]


def run(ctx, hs):
    """(paths after prepare, paths after run, results) of one batch"""
    batch = ctx.prepare(hs)
    try:
        p0 = batch.paths()
        batch.run()
        res = batch.fetch()
        return p0, batch.paths(), res
    finally:
        batch.free()


def check(want, res):
    """want: [(name, oracle score, oracle trace)]"""
    assert len(res) == len(want)
    for (name, scr, tr), (gscr, cells, gtr, st) in zip(want, res):
        assert st == 0 and gscr == scr, (name, st, gscr, scr)
        assert np.array_equal(gtr, tr), name


def wanted(synth, tall):
    return [(name, scr, tr) for name, _, _, scr, tr in synth] + [("three strips %d" % k, scr, tr) for k, (_, scr, tr, _) in enumerate(tall)]


def test_annotations_cover_the_cases(synth, tall, L):
    """where the annotations put their cells (the walk restated in intronlib.bonus_cells / g2g_bonus_cells), and that they
    matter: every score differs from its plain twin, at least one traceback does"""
    differs = 0
    for name, d, e, scr, tr in synth:
        al, ar, bl, br, lw, up = il.geometry(e)
        cells = il.bonus_cells(e)
        at = {(m, n) for m, n, _, _ in cells}
        assert {m for m, _ in at} == set(nv.ROWS) | {ar - 1}
        assert 64 < ar - al <= 128                                  # two 64-row strips
        assert any(m == 63 for m, _ in at) and any(m == 64 for m, _ in at)       # either side of the strip boundary
        assert (0, 0) in at and max(0 + lw, bl) == 0                # first in-band column of row 0
        assert (0, min(up, br - 1)) in at                           # last in-band column of row 0
        assert (ar - 1, br - 1) in at                               # last cell of the last row
        if int(e["a_pfq_step"][0]) == 3:
            assert any(h == 0 and mx == 0 for _, _, h, mx in cells)     # phase mismatch
            assert any(h > 0 and mx == 0 for _, _, h, mx in cells)      # in phase, off the codon start
        assert any(h > 0 and mx > 0 for _, _, h, mx in cells)
        assert scr != d["scr"][0], name
        differs += not np.array_equal(tr, d["vmf_trace"])
    assert differs >= 1
    from prrn_aln_amd import build
    lib = C.CDLL(build.build_lib())
    for h, scr, tr, scr0 in tall:
        q = h.c
        at = {(m, n) for m, n, _, _ in nv.library_bonus_cells(lib, h)}
        assert 128 < q.a.right - q.a.left <= 192                    # three strips
        assert {m for m, _ in at} == {0, 63, 64, 65, 127, 128, q.a.right - 1}
        assert (0, 0) in at and (0, min(q.up, q.b.right - 1)) in at and (q.a.right - 1, q.b.right - 1) in at
        assert scr != scr0


def test_edge_annotations():
    """5. an a-side table whose first boundary lies before a.left's codon, and one whose cursor gets stuck (two boundaries in
    one codon): the table the strips read (g2g_bonus_cells on the _nv problem, host code) is the restated walk's"""
    from prrn_aln_amd import build
    lib = C.CDLL(build.build_lib())
    seen = set()
    for name, rows, crg, noll, col in nv.NV:
        d = il.load(name)
        for variant in ("early", "stuck"):
            if variant == "stuck" and int(d["a_molc"][0]) == 2:     # (a codon of one column holds one boundary)
                continue
            e = nv.annotate(d, col, variant)
            want = il.bonus_cells(e)
            assert nv.library_bonus_cells(lib, _abi.problem_from_arrays(e)) == want and want
            got_rows = {m for m, _, _, _ in want}
            if variant == "early":
                assert int(e["a_pfq_pos"][0]) < int(e["a_left"][0]) * int(e["a_pfq_step"][0])
                assert got_rows == (set(nv.ROWS) | {rows - 1}) - {0}
            else:
                assert got_rows == {0, 31, 62, 63}                  # nothing after the codon with two boundaries
            seen.add(variant)
    assert seen == {"early", "stuck"}


@gpu
def test_default_options(ctx, synth, tall):
    """1. default options: every annotated _nv DP reports 8 after prepare and after run; score bit for bit and traceback
    records are the oracle's.  (Before the v8 strips knew the bonus these DPs reported 1.)"""
    hs = holders(synth, tall)
    p0, p1, res = run(ctx, hs)
    assert p0 == [8] * len(hs) and p1 == p0
    check(wanted(synth, tall), res)


@gpu
@pytest.mark.parametrize("opt", ["NO_STRIP_BONUS", "FORCE_V1"])
def test_same_inputs_on_v1(synth, tall, opt):
    """2. the same inputs with the strips' bonus switched off / everything on g2g_forward_kernel: path 1, the same results"""
    c = engine.Context(options={opt: "1"})
    try:
        hs = holders(synth, tall)
        p0, p1, res = run(c, hs)
    finally:
        c.close()
    assert p0 == [1] * len(hs) and p1 == p0
    check(wanted(synth, tall), res)


@gpu
def test_mixed_batch(ctx, synth, L):
    """3. annotated _nv DPs, their unannotated twins and annotated DPs of other record types interleaved in one batch: each
    reports the path it reports alone, the twins run on v8 and equal their goldens"""
    v7d = [d for d in (dict(np.load(f)) for f in il.INTRON) if int(d["alnmode"][0]) == 6][0]       # annotated reference golden, DPunit
    v2e = il.annotate(il.load("prot12x80_tgapf05_k1"))                                            # synthetic annotation, _hf
    v2scr, _, v2tr = oraclelib.forward(L, _abi.problem_from_arrays(v2e))
    other = [v7d, v2e]
    alone = []
    for d in other:
        b = ctx.prepare([_abi.problem_from_arrays(d)])
        alone += b.paths()
        b.free()
    assert alone == [7, 2]
    groups = (("a", [e for _, _, e, _, _ in synth]), ("p", [d for _, d, _, _, _ in synth]), ("o", other))
    arrays, idx = [], {"a": [], "p": [], "o": []}
    for k in range(len(synth)):                                       # interleaved
        for key, x in groups:
            if k < len(x):
                idx[key].append(len(arrays))
                arrays.append(x[k])
    p0, p1, res = run(ctx, [_abi.problem_from_arrays(d) for d in arrays])
    assert p1 == p0
    assert [p1[i] for i in idx["a"]] == [8] * len(synth)
    assert [p1[i] for i in idx["p"]] == [8] * len(synth)
    assert [p1[i] for i in idx["o"]] == alone
    check([(name, scr, tr) for name, _, _, scr, tr in synth], [res[i] for i in idx["a"]])
    check([(name + " (plain)", d["scr"][0], d["vmf_trace"]) for name, d, _, _, _ in synth], [res[i] for i in idx["p"]])
    check([("v7", v7d["scr"][0], v7d["vmf_trace"]), ("v2", v2scr, v2tr)], [res[i] for i in idx["o"]])


@gpu
@pytest.mark.parametrize("victim", [0, 1])
def test_recovery_of_annotated_nv_dps(synth, victim):
    """4. the recovery path (test hook INJECT_STALL, as tests/test_gpu_intron_strips.py uses it): the victim's first strip waits
    for a flag nobody writes, loses its wait and is re-run inside g2g_batch_run.  Victim 1 is re-run on the strips (a one-DP
    batch in which the hook names nobody) and reports 8; victim 0 is DP 0 of its retry batch too, stalls again and ends on
    g2g_forward_kernel: g2g_batch_paths reports 1 for it.  Results: the oracle's."""
    pick = [synth[0], synth[2], synth[4]]                             # Noll 3; Noll 2 weighted; Noll 2 unweighted
    c = engine.Context(options={"INJECT_STALL": str(victim), "WAIT_LIMIT_MS": "300"})
    try:
        p0, p1, res = run(c, [_abi.problem_from_arrays(e) for _, _, e, _, _ in pick])
        cnt = c.counters()
    finally:
        c.close()
    assert p0 == [8, 8, 8]
    assert p1 == ([1, 8, 8] if victim == 0 else [8, 8, 8])
    assert cnt["recovered_dps"] == (2 if victim == 0 else 1) and cnt["recovered_on_v1"] == (1 if victim == 0 else 0)
    check([(name, scr, tr) for name, _, _, scr, tr in pick], res)
