"""Wide, gap-rich groups on the GPU: the fixtures of tests/golden/wide (tests/widelib.py names the cases and the constant each
K sits next to) through the DP on every kernel selection, calcSpScore on its three walkers, and the device builders -- plus
builder-only groups at the member counts g2g_device_derive changes path at.  Expected values are the REFERENCE's (the fixtures);
tests/test_host_builders.py and tests/test_oracle_golden.py hold the host builders and the oracle to the same fixtures on the CPU.
Equal doubles, equal integer arrays, status 0."""
import numpy as np
import pytest

import widelib
from prrn_aln_amd import _abi, engine, operator as op
from test_gpu_builders import same_problem
from test_gpu_paths import CONFIGS, _setenv
from test_host_builders import groups_from_golden, params_from_golden

pytestmark = pytest.mark.gpu

# cases with a side of more than 64 gap classes alive in one column: g2g_device_derive refuses, the host builds
OVERFLOW = ("K65", "K189", "K190", "K70xK66", "hf65")
# What every case runs on by default, Noll 2 / Noll 3, in the numbers of g2g_batch_paths: 1 g2g_forward_kernel (v1), 2 the
# 8-lanes-per-cell strips (v2), 3 the one-lane-per-cell strips v3 -- choose_kernel's generations 0, 1 and 2 / 3.  g2g_batch_paths
# gives v3 with LDS lists and v3r one number; a list longer than the G2G_V3_NA register slots of v3r tells them apart.
V1, V2, V3 = 1, 2, 3
V3R_SLOTS = 16                                                       # G2G_V3_NA, terminator included
DEFAULT_PATH = {"K61": (V2, V2), "K62": (V2, V2), "K64": (V2, V2), "K65": (V2, V2), "K189": (V1, V1), "K190": (V1, V1),
                "K70xK66": (V1, V1), "hf65": (V2, V2), "hf20": (V3, V2), "m257": (V2, V2), "m300": (V2, V2)}


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


@pytest.fixture(autouse=True)
def _fresh_options(ctx):
    ctx.reset_options()
    yield
    ctx.reset_options()


@pytest.fixture(scope="module")
def wide():
    return widelib.load()


@pytest.fixture(scope="module")
def host(wide):
    """name -> PwdM built on the host from the fixture's groups"""
    out = {}
    for name, d in wide:
        alp = params_from_golden(d)
        out[name] = op.PwdM(list(groups_from_golden(d, alp)), alp)
    return out


def _batch_pwdm(ctx, items):
    alp = params_from_golden(items[0][1])
    return op.PwdM.batch(ctx, [list(groups_from_golden(d, alp)) for _, d in items], alp)


@pytest.fixture(scope="module")
def built(ctx, wide):
    """name -> PwdM from g2g_pwdm_create_batch: one call per Noll for the cases the device takes, one call per overflowing case"""
    out = {}
    for noll in (2, 3):
        items = [(n, d) for n, d in wide if d["Noll"][0] == noll and widelib.case_of(n) not in OVERFLOW]
        assert len({float(d["alnprm_ls"][0]) for _, d in items}) == 1
        out.update(zip([n for n, _ in items], _batch_pwdm(ctx, items)))
    for n, d in wide:
        if widelib.case_of(n) in OVERFLOW:
            out[n] = _batch_pwdm(ctx, [(n, d)])[0]
    return out


def _forward_all(ctx, wide):
    hs = [_abi.problem_from_arrays(d) for _, d in wide]
    batch = ctx.prepare(hs)
    try:
        chosen = batch.paths()
        batch.run()
        res = batch.fetch()
        ran = batch.paths()
    finally:
        batch.free()
    bad = [(n, st, scr, float(d["scr"][0])) for (n, d), (scr, cells, tr, st) in zip(wide, res)
           if st != 0 or scr != d["scr"][0] or not np.array_equal(tr, d["vmf_trace"])]
    return chosen, ran, bad


def test_dp_default_selection(ctx, wide):
    """All wide fixtures in one batch with nothing forced: the reference's score and Vmf chain, on the generation choose_kernel
    falls through to: g2g_forward_kernel (not forced), v2 and v3 with LDS lists are all reached.  Recorded from the run
    (Noll 2 / Noll 3):
      K61 K62 K64 K65 m257 m300    v2 / v2    (lists of 42 .. 67 entries: beyond v6's 16 slots, inside v2's LDS budget)
      K189 K190 K70xK66            v1 / v1    (v2_lds_bytes beyond V2_LDS_MAX: g2g_forward_kernel by default, capa 191 .. 192 and 72 x 68)
      hf65                         v2 / v2    (v3-LDS would need more than V2_LDS_MAX)
      hf20                         v3-LDS / v2 (under a third of V2_LDS_MAX with 6 records per cell, above it with 9)"""
    chosen, ran, bad = _forward_all(ctx, wide)
    print([(n, g) for (n, _), g in zip(wide, chosen)])
    assert not bad, bad
    assert chosen == ran
    for (n, d), g in zip(wide, chosen):
        assert g == DEFAULT_PATH[widelib.case_of(n)][int(d["Noll"][0]) - 2], (n, g)
        if g == V3:                                                  # v3 with LDS lists: v3r cannot hold this row list
            assert max(x.max() for x in widelib.fixture_list_lengths(d, "a_")) + 1 > V3R_SLOTS, n
    assert {V1, V2, V3} <= set(chosen)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_dp_forced_paths(ctx, monkeypatch, wide, name):
    """the same batch under every forced selection of tests/test_gpu_paths.py: a forced kernel that cannot take a case hands it
    to one that can, and the result does not change"""
    _setenv(monkeypatch, CONFIGS[name], ctx)
    chosen, ran, bad = _forward_all(ctx, wide)
    assert not bad, (bad, chosen)
    assert chosen == ran
    if name == "v1":
        assert set(chosen) == {V1}


def _check_fstat(wide, fs):
    for (n, d), f in zip(wide, fs):
        assert f[2] == 0, (n, f)
        assert f[0] == d["fstat_val"][0] and f[1] == d["fstat_gap"][0], (n, f, float(d["fstat_val"][0]), float(d["fstat_gap"][0]))
        if len(f) > 4:
            assert tuple(f[4:7]) == (d["fstat_mch"][0], d["fstat_mmc"][0], d["fstat_unp"][0]), (n, f)


@pytest.mark.parametrize("opts", [{}, {"NO_SPLANES": "1"}, {"NO_SPSTREAM": "1"}], ids=["lanes_walk", "stream_scalar_walk", "unstreamed_walk"])
def test_calcspscore(ctx, wide, host, opts):
    """calcSpScore along the reference's own skeletons gives the reference's fstat on all three walkers: lists of 62 entries
    stay on the lanes (K61), 63 and more go back to the scalar walker (K62 ...), capa + 1 = 192 keeps the running lists in LDS
    (K189), 193 moves them to HBM (K190)"""
    for k, v in opts.items():
        ctx.set_option(k, v)
    pws = [host[n] for n, _ in wide]
    skls = [d["align2_skl"] for _, d in wide]
    _check_fstat(wide, op.calcSpScore_batch(ctx, pws, skls))
    _check_fstat(wide, op.calcSpScore_batch(ctx, pws, skls, stats=True))


@pytest.mark.parametrize("opts", [{}, {"NO_SCORE_BATCH": "1"}], ids=["one_resident_batch", "general_route"])
def test_align2_score_batch(ctx, wide, host, opts):
    """g2g_align2_score_batch: the DP and calcSpScore of the current and of the new alignment -- here both the reference's"""
    for k, v in opts.items():
        ctx.set_option(k, v)
    got = op.align2_score_batch(ctx, [host[n] for n, _ in wide], [d["align2_skl"] for _, d in wide])
    for (n, d), (scr, skl, st, fc, fn) in zip(wide, got):
        assert st == 0 and scr == d["align2_scr"][0] and np.array_equal(skl, d["align2_skl"]), (n, st, scr)
        for f in (fc, fn):
            assert f[2] == 0 and f[0] == d["fstat_val"][0] and f[1] == d["fstat_gap"][0], (n, f)


def test_device_builders_at_the_edges(wide, host, built):
    """g2g_pwdm_create_batch on the fixtures' groups == the host build (which equals the reference's dump), and the DEVICE built
    what it is meant to take: 61, 62 and 64 classes alive in a column and 257 / 300 members carry twins; 65 and more classes
    are refused (no twins on that side) and the host's arrays come back all the same"""
    for n, d in wide:
        g, h = built[n], host[n]
        assert g.swp == h.swp, n
        same_problem(g.problem, h.problem, n)
        sh, sg = op.spparams(h), op.spparams(g)
        assert (sh.vab, sh.basic_gep, sh.diffu, sh.diff_u) == (sg.vab, sg.basic_gep, sg.diffu, sg.diff_u), n
        assert not h.problem.a.dev and not h.problem.b.dev
        if widelib.case_of(n) in OVERFLOW:
            assert not g.problem.a.dev, n
        else:
            assert g.problem.a.dev, n
            assert g.problem.b.dev or not g.problem.b.dels, n


def test_dp_on_device_built_inputs(ctx, wide, built):
    """align2 on the PwdMs of g2g_pwdm_create_batch (inputs resident where the device built them) == the reference's align2"""
    res = op.align2_batch(ctx, [built[n] for n, _ in wide])
    for (n, d), (scr, skl, st) in zip(wide, res):
        assert st == 0 and scr == d["align2_scr"][0] and np.array_equal(skl, d["align2_skl"]), (n, st, scr)


def _many_members(many, at, length, c0, random_gaps=False):
    """a staircase over the member indices `at` of a group of `many`; random_gaps: the other members carry a run of 1 .. 3
    columns somewhere in columns 5 .. 59 with probability 0.6 (at most four classes alive there)"""
    b = widelib.base(21, length)
    if not random_gaps:
        return widelib.stair_at(many, at, c0, b)
    rng = np.random.default_rng(many)
    run = {i: j + 1 for j, i in enumerate(sorted(at))}
    rows = []
    for i in range(many):
        if i in run:
            rows.append(widelib.member(rng, b, c0, run[i]))
        elif rng.random() < 0.6:
            rows.append(widelib.member(rng, b, int(rng.integers(8, 60)), int(rng.integers(1, 4))))
        else:
            rows.append(widelib.member(rng, b))
    return rows


BUILDER_ONLY = {
    # name: (members, gapped indices, columns, c0, random short gaps, taken by the device)
    "m4096": (4096, [0, 63, 64, 255, 256, 257, 511, 512, 1023, 1024, 2047, 2048, 3000, 3071, 3072, 4000, 4031, 4032, 4094, 4095], 40, 35, False, True),
    "m4097": (4097, [0, 63, 64, 255, 256, 257, 511, 512, 1023, 1024, 2047, 2048, 3000, 3071, 3072, 4000, 4095, 4096], 40, 35, False, False),
    "m1000_random": (1000, list(range(3, 1000, 25)), 120, 112, True, True),
}


@pytest.mark.parametrize("name", list(BUILDER_ONLY))
def test_device_builders_member_counts(ctx, name):
    """no DP: 4096 members are the most g2g_device_derive takes (`many > 4096` is refused and built on the host), and a
    1000-member group with scattered short gaps under a 40-step staircase keeps 40 classes alive at once"""
    many, at, length, c0, rnd, taken = BUILDER_ONLY[name]
    alp = op.AlnParam()
    rows = _many_members(many, at, length, c0, rnd)
    one = [widelib.member(np.random.default_rng(3), widelib.base(21, length)[2:length - 3])]
    h = op.PwdM([op.mSeq(rows, alp), op.mSeq(one, alp)], alp)
    g = op.PwdM.batch(ctx, [[op.mSeq(rows, alp), op.mSeq(one, alp)]], alp)[0]
    assert not h.swp and h.problem.a.many == many and h.problem.a.has_gfq and h.problem.a.gfq.hetero == len(at) + 1
    t = widelib.list_lengths(h.problem.a)[1]
    assert t[c0] == len(at) == t.max()
    assert g.swp == h.swp
    same_problem(g.problem, h.problem, name)
    assert bool(g.problem.a.dev) == taken
