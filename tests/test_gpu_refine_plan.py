"""g2g_refine_planned end to end on the GPU: prrn's default refinement (fused groups, one loop per unconserved column range, last
range first) with the plan made on the device (g2g_refine_plan: the fuse tests and the grouped consreg) and every DP and calcSpScore
on the device -- on tests/golden/refine_plan: the TRACED cases walk the reference's trajectory range by range, the GROUPED cases end
in the reference's alignment with its per-range group and division counts, and take, step for step, the numbers the CPU-checker run
of tests/test_refine_plan_host.py takes.  The new ground for the kernels is what they are driven over: column slices, sides made of
several fused groups, relations of two and three groups."""
import numpy as np
import pytest

import fuselib as fl
import refinelib
import refineplanlib as rp
from prrn_aln_amd import engine, guide, refine
from test_refine_plan_host import GROUPED, TRACED, host_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


def device_run(ctx, case, **kw):
    """plan = None: the plan is made on the device with the reference's plan parameters, the refinement runs over it"""
    prm, _sm = case.alp.to_c()
    pprm, _psm = case.alp_plan.to_c()
    c0 = ctx.counters()
    out = refine.refine_planned(ctx, case.codes, case.tree, prm, case.thr, case.weight, plan=None, plan_prm=pprm, **kw)
    c1 = ctx.counters()
    # g2g_batch_paths is not reachable through this entry: the scheduler's own counters say that no wait gave up and no DP was re-run
    assert c1["wait_timeouts"] == c0["wait_timeouts"] and c1["recovered_dps"] == c0["recovered_dps"], ctx.last_timeout()
    assert out[3]["wait_timeouts"] == 0 and out[3]["recovered_dps"] == 0
    assert c1["runs"] > c0["runs"] or not out[1]
    return out


def device_plan(ctx, case):
    return guide.refine_plan(ctx, case.codes, case.tree, case.alp_plan.to_c()[0], case.thr, case.weight)


@pytest.mark.parametrize("path", TRACED, ids=[rp.fixture_id(p) for p in TRACED])
def test_traced_cases_on_the_device(ctx, path):
    case = rp.Case(path)
    rp.same_plan(device_plan(ctx, case), case.plan())
    final, steps, ranges, stats = device_run(ctx, case, want_moves=True, window=16)
    refinelib.check_against_trace(case.merged_trace(), final, steps, stats)
    at = 0
    ran = [r for r in sorted(ranges, key=lambda r: -r["range"]) if r["nsteps"]]
    assert len(ran) == len(case.f["trace"])
    for rs, t in zip(ran, case.f["trace"]):
        assert rs["range"] == t["range"] and rs["first_step"] == at and rs["cycle"] == t["cycle"]
        assert [s["branch"] for s in steps[at:at + rs["nsteps"]]] == t["branches"] and rs["accepted"] == len(t["accepted"])
        at += rs["nsteps"]
    assert at == len(steps)
    rp.check_ranges_against_print(case, ranges)
    assert stats["batches"] < len(steps)                                 # the DPs really ran in batches


@pytest.mark.parametrize("path", GROUPED, ids=[rp.fixture_id(p) for p in GROUPED])
def test_grouped_cases_on_the_device(ctx, path):
    case, h_final, h_steps, h_ranges, h_stats = host_run(path)
    rp.same_plan(device_plan(ctx, case), case.plan())
    final, steps, ranges, stats = device_run(ctx, case, window=16)
    assert np.array_equal(final, case.final)
    rp.check_ranges_against_print(case, ranges)
    rp.same_steps(steps, h_steps)                                        # branch, skipped, accepted; scr, val_new, val_old with ==
    for a, b in zip(ranges, h_ranges):
        assert {k: v for k, v in a.items() if k != "gain"} == {k: v for k, v in b.items() if k != "gain"} and a["gain"] == b["gain"]


def test_the_window_does_not_change_the_result(ctx):
    case, h_final, h_steps, h_ranges, h_stats = host_run([p for p in GROUPED if "prot8x300" in p][0])
    f1, s1, r1, st1 = device_run(ctx, case, window=1)
    f8, s8, r8, st8 = device_run(ctx, case, window=8)
    assert np.array_equal(f1, f8) and np.array_equal(f1, case.final)
    rp.same_steps(s1, s8)
    rp.same_steps(s1, h_steps)
    assert st1["divisions_wasted"] == 0 and st1["batches"] >= st8["batches"]


def test_the_library_makes_the_plan_when_none_is_given(ctx):
    """plan == NULL in the C call: g2g_refine_plan with the parameters of the call, then the refinement over it -- against the
    restated plan under the same parameters, run with the CPU checker scoring"""
    case = rp.Case([p for p in GROUPED if "prot6x260" in p][0])
    prm, _sm = case.alp.to_c()
    pl = rp.plan_object(fl.plan(case.codes, case.tree5, case.alp, case.thr, case.weight))
    h = refine.refine_planned(None, case.codes, case.tree, prm, case.thr, case.weight, pl, scorer=refinelib.oracle_scorer(), window=8)
    d = refine.refine_planned(ctx, case.codes, case.tree, prm, case.thr, case.weight, window=8)
    assert np.array_equal(h[0], d[0])
    rp.same_steps(h[1], d[1])
    assert [{k: v for k, v in r.items()} for r in h[2]] == [{k: v for k, v in r.items()} for r in d[2]]
    assert any(r["nsteps"] for r in d[2]) and any(r["groups"] < 2 for r in d[2])
