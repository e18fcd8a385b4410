"""g2g_refine_planned on the CPU: prrn's default refinement (IterMsa::preprrn, reference src/prrn5.cc:785-839) -- fused groups that move
as one block, one Prrn per unconserved column range from the last range to the first, all Prrns on one rand() state -- with the plan
as tests/fuselib.py restates it and the CPU CHECKER in the scorer's seat (refinelib.oracle_scorer).  tests/golden/refine_plan holds
what the reference did: TRACED cases (nothing fuses; every branch, align2 and accepted move of every range) and GROUPED cases (the
final alignment and the line the reference prints per Prrn).  tests/test_gpu_refine_plan.py runs the same cases on the GPU."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import refinelib
import refineplanlib as rp
from prrn_aln_amd import guide, refine
from prrn_aln_amd import operator as op
from prrn_aln_amd._lib import G2GError, lib

G2G_ERR_ARG, G2G_ERR_MODE = -1, -2
TRACED = rp.fixtures("traced")
GROUPED = rp.fixtures("grouped")
_RUNS = {}


def host_run(path):
    """one CPU-checker run per fixture, shared (the GPU test compares its steps with it)"""
    if path not in _RUNS:
        case = rp.Case(path)
        _RUNS[path] = (case,) + rp.run_host(case, want_moves=True, window=8)
    return _RUNS[path]


def test_the_fixture_set():
    assert len(TRACED) >= 2 and len(GROUPED) >= 4
    assert lib().g2g_refine_planned and callable(refine.refine_planned) and callable(guide.plan_struct)


@pytest.mark.parametrize("path", TRACED, ids=[rp.fixture_id(p) for p in TRACED])
def test_traced_cases_walk_the_reference_trajectory_range_by_range(path):
    case = rp.Case(path)
    rec = []
    scorer, _inner = rp.weight_recording_scorer(rec)
    final, steps, ranges, stats = rp.run_host(case, scorer=scorer, want_moves=True, window=1)
    # the ranges one after the other, last range first: branches, (scr, val) of every DP with ==, the moves, the final MSA
    refinelib.check_against_trace(case.merged_trace(), final, steps, stats)
    at = 0
    order = sorted(ranges, key=lambda r: -r["range"])
    assert len(case.f["trace"]) == len([r for r in order if r["nsteps"]])
    for rs, t in zip([r for r in order if r["nsteps"]], case.f["trace"]):
        assert rs["range"] == t["range"] and rs["first_step"] == at and rs["cycle"] == t["cycle"]
        assert [s["branch"] for s in steps[at:at + rs["nsteps"]]] == t["branches"]
        assert rs["accepted"] == len(t["accepted"])
        at += rs["nsteps"]
    assert at == len(steps) == stats["divisions"]
    # the member weights that reached the builders are the reference's doubles (window 1: one DP per scorer call, in order)
    ref = [a for t in case.f["trace"] for a in t["align2"]]
    assert len(rec) == len(ref)
    for (wa, wb), a in zip(rec, ref):
        assert wa == a["wa"] and wb == a["wb"]
    rp.check_ranges_against_print(case, ranges)


@pytest.mark.parametrize("path", TRACED[:1], ids=[rp.fixture_id(p) for p in TRACED[:1]])
def test_windows_do_not_change_a_traced_trajectory(path):
    case, final, steps, ranges, stats = host_run(path)
    refinelib.check_against_trace(case.merged_trace(), final, steps, stats)
    assert stats["batches"] < len(steps)


@pytest.mark.parametrize("path", GROUPED, ids=[rp.fixture_id(p) for p in GROUPED])
def test_grouped_cases_end_in_the_reference_alignment(path):
    case, final, steps, ranges, stats = host_run(path)
    assert np.array_equal(final, case.final)
    assert [r["range"] for r in ranges] == list(range(len(case.f["ranges"])))
    assert [[r["left"], r["right"]] for r in ranges] == case.f["ranges"]
    rp.check_ranges_against_print(case, ranges)          # groups, divisions (= rep), the columns afterwards, |gain - (sps - initsp)| <= 0.11
    assert stats["accepted"] == sum(r["accepted"] for r in ranges) == sum(1 for s in steps if s["accepted"]) == len(stats["moves"])
    # on_accept hands over MEMBER lists: both sides together are every member once, a fused group stays on one side
    pl = case.restated()
    many = case.codes.shape[1]
    acc = iter(stats["moves"])
    for rs in sorted(ranges, key=lambda r: -r["range"]):
        groups = pl["per_range"][rs["range"]][1][0]
        for s in steps[rs["first_step"]:rs["first_step"] + rs["nsteps"]]:
            if s["accepted"]:
                br, la, lb, skl = next(acc)
                assert br == s["branch"] and sorted(la + lb) == list(range(many)) and (len(la), len(lb)) == (s["na"], s["nb"])
                for g in groups:
                    assert set(g) <= set(la) or set(g) <= set(lb)


def test_a_trivial_plan_is_g2g_refine():
    """one range [0, len), nothing fused: the shared loop gives g2g_refine's own steps and final MSA (and the reference's trajectory)"""
    path = os.path.join(refinelib.GOLD, "refine_prot12x80_s3.json")
    f, tree, alp, start = refinelib.load(path)
    f0, s0, st0 = refine.refine_native(None, start, tree, alp, window=8, scorer=refinelib.oracle_scorer(), want_moves=True)
    refinelib.check_against_trace(f, f0, s0, st0)
    prm, _sm = alp.to_c()
    plan = rp.trivial_plan(tree, start.shape[1], start.shape[0])
    f1, s1, rs, st1 = refine.refine_planned(None, start, tree, prm, plan=plan, weight=np.asarray(tree.vol[:tree.n_leaves]), window=8,
                                            scorer=refinelib.oracle_scorer(), want_moves=True)
    assert np.array_equal(f0, f1)
    rp.same_steps(s0, s1)
    assert [(s["na"], s["nb"], s["swp"], s["delta"]) for s in s0] == [(s["na"], s["nb"], s["swp"], s["delta"]) for s in s1]
    assert all(a[:3] == b[:3] and np.array_equal(a[3], b[3]) for a, b in zip(st0["moves"], st1["moves"]))
    assert {k: v for k, v in st0.items() if k != "moves"} == {k: v for k, v in st1.items() if k != "moves"}
    assert len(rs) == 1 and rs[0]["nsteps"] == len(s1) and rs[0]["groups"] == 12 and rs[0]["accepted"] == st1["accepted"]


# ---- sharding: two gloo ranks, each scoring half of every window of every range ---------------------------------------------------
WORKER = r"""
import os, sys, json, hashlib
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np, torch.distributed as dist
import refinelib, refineplanlib as rp
from prrn_aln_amd._lib import G2GError
from prrn_aln_amd.refine import torch_exchange
rank = int(os.environ["RANK"])
dist.init_process_group("gloo", rank=rank, world_size=int(os.environ["WORLD_SIZE"]))
case = rp.Case({fixture!r})
fail = int(os.environ.get("FAIL_RANK", "-1")) == rank
res = {{"rank": rank}}
try:
    final, steps, ranges, stats = rp.run_host(case, window=8, exchange=torch_exchange(), slot_cap=1024,
                                              scorer=refinelib.oracle_scorer(fail_after=2 if fail else -1))
    res.update(ok=True, digest=hashlib.sha1(final.tobytes()).hexdigest(), scored_here=stats["divisions_scored_here"],
               dps=sum(1 for s in steps if not s["skipped"]), ranges=[r["nsteps"] for r in ranges])
except G2GError as e:
    res.update(ok=False, error=str(e))
dist.barrier(); dist.destroy_process_group()
print(json.dumps(res))
"""


def _run_ranks(fixture, extra_env):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), **extra_env)
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER.format(root=root, fixture=fixture)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE))
    outs = []
    for p in procs:
        out, err = p.communicate(timeout=600)
        assert p.returncode == 0, err.decode()[-2000:]
        outs.append(json.loads(out.decode().strip().splitlines()[-1]))
    return outs


SHARDED = [p for p in GROUPED if "prot6x260" in p][0]


def test_two_ranks_end_with_the_msa_of_one():
    case, final, steps, ranges, stats = host_run(SHARDED)
    import hashlib
    outs = _run_ranks(SHARDED, {})
    assert all(o["ok"] for o in outs), outs
    assert outs[0]["digest"] == outs[1]["digest"] == hashlib.sha1(final.tobytes()).hexdigest()
    assert outs[0]["ranges"] == outs[1]["ranges"] == [r["nsteps"] for r in ranges]
    assert all(0 < o["scored_here"] < o["dps"] for o in outs), outs          # the work really was split


def test_a_rank_local_scorer_failure_returns_the_same_error_on_both_ranks():
    outs = _run_ranks(SHARDED, {"FAIL_RANK": "1"})
    assert not any(o["ok"] for o in outs), outs
    codes = [o["error"].split("rc=")[1].split(":")[0] for o in outs]
    assert codes[0] == codes[1] != "0", outs
    assert "rank 1 failed" in outs[0]["error"]


# ---- refusals, each before any scoring ----------------------------------------------------------------------------------------------
def _counting_scorer():
    calls = []
    inner = refinelib.oracle_scorer()

    def cb(*a):
        calls.append(a[1])
        return inner(*a)
    from prrn_aln_amd import _abi
    return _abi.SCORE_FN(cb), calls, inner


def _refused(case, plan, code, match, prm=None, scorer="count", **kw):
    sc, calls, _keep = _counting_scorer()
    p, _sm = case.alp.to_c()
    with pytest.raises(G2GError, match=r"rc=%d.*%s" % (code, match)):
        refine.refine_planned(None, case.codes, case.tree, prm if prm is not None else p, case.thr, case.weight, plan,
                              **(dict(scorer=sc) if scorer == "count" else {}), **kw)
    assert calls == []


def test_malformed_plans_are_refused():
    case = rp.Case(SHARDED)
    good = case.plan()
    n = len(good.ranges)
    assert n >= 3
    # overlapping ranges
    bad = case.plan()
    bad.ranges = good.ranges.copy()
    bad.ranges[1, 0] = good.ranges[0, 1] - 1
    _refused(case, bad, G2G_ERR_ARG, "range 1")
    # ranges that leave the columns
    bad = case.plan()
    bad.ranges = good.ranges.copy()
    bad.ranges[n - 1, 1] = case.codes.shape[0] + 1
    _refused(case, bad, G2G_ERR_ARG, "range %d" % (n - 1))
    # a subset that drops a member
    bad = case.plan()
    r = next(i for i, rel in enumerate(bad.relations) if len(rel.groups) >= 2)
    bad.relations[r].groups = [g.copy() for g in bad.relations[r].groups]
    bad.relations[r].groups[0] = bad.relations[r].groups[0][:-1] if len(bad.relations[r].groups[0]) > 1 else bad.relations[r].groups[1]
    _refused(case, bad, G2G_ERR_ARG, "relation of range %d" % r)
    # a tree of the wrong size
    bad = case.plan()
    rel = bad.relations[r]
    for k in ("left", "right", "parent", "origin", "vol", "cur"):
        setattr(rel, k, getattr(rel, k)[:-2])
    _refused(case, bad, G2G_ERR_ARG, "2 \\* num - 1")
    # a tree that is no tree, and an origin out of range
    bad = case.plan()
    bad.relations[r].parent = bad.relations[r].parent.copy()
    bad.relations[r].parent[0] = 0
    _refused(case, bad, G2G_ERR_ARG, "relation of range %d" % r)
    bad = case.plan()
    bad.relations[r].origin = bad.relations[r].origin.copy()
    bad.relations[r].origin[0] = 10 ** 6
    _refused(case, bad, G2G_ERR_ARG, "origin")


def test_modes_the_plan_refuses_are_refused():
    case = rp.Case(SHARDED)
    for kw, what in ((dict(tgapf=0.5), "terminal-gap"), (dict(u0=1.0), "ether"), (dict(banded=0), "banded")):
        alp = op.AlnParam(ls=case.alp.ls, molc=case.alp.molc, max_code=case.alp.max_code, **kw)
        prm, _sm = alp.to_c()
        _refused(case, case.plan(), G2G_ERR_MODE, what, prm=prm)


def test_no_context_needs_a_plan_and_a_scorer():
    case = rp.Case(SHARDED)
    _refused(case, case.plan(), G2G_ERR_ARG, "context", scorer=None)
    _refused(case, None, G2G_ERR_ARG, "context")


def test_an_empty_leaf_group_is_refused():
    """a hand-made 4 x 12 MSA: member 3 has no residue inside the range [4, 8), and is a leaf group of the range's relation"""
    rows = ["ACDEFGHIKLMN", "ACDEFGHIKLMN", "ACDQFGHIKLMN", "ACDE----KLMN"]
    codes = op.encode(rows, 1)
    tree = refine.KTree([-1, -1, -1, -1, 0, 4, 5], [-1, -1, -1, -1, 1, 2, 3], [4, 4, 5, 6, 5, 6, -1],
                        [0.2, 0.2, 0.3, 0.3, 0.4, 0.7, 1.0], [0.5, 0.5, 0.4, 0.3, 0.6, 0.7, 1.0])
    rel = rp.trivial_plan(tree, 4, 12).whole
    plan = guide.RefinePlan(False, rel, np.array([[4, 8]], np.int32), np.array([0], np.int32), np.array([0], np.int32), [rel])
    sc, calls, _keep = _counting_scorer()
    prm, _sm = op.AlnParam().to_c()
    with pytest.raises(G2GError, match=r"rc=%d.*group 3 of range 0" % G2G_ERR_MODE):
        refine.refine_planned(None, codes, tree, prm, plan=plan, scorer=sc)
    assert calls == []
    # over the whole MSA every leaf group has residues: the same relation runs
    rel2 =guide.RefinePlan(False, rel, np.array([[0, 12]], np.int32), np.array([1], np.int32), np.array([1], np.int32), [rel])
    final, steps, ranges, stats = refine.refine_planned(None, codes, tree, prm, plan=rel2, scorer=sc)
    assert ranges[0]["nsteps"] == len(steps) > 0


# ---- results without work -----------------------------------------------------------------------------------------------------------
def test_nothing_to_refine_hands_the_input_back():
    case = rp.Case(SHARDED)
    plan = case.plan()
    plan.nothing_to_refine = True
    sc, calls, _keep = _counting_scorer()
    prm, _sm = case.alp.to_c()
    final, steps, ranges, stats = refine.refine_planned(None, case.codes, case.tree, prm, case.thr, case.weight, plan, scorer=sc)
    assert np.array_equal(final, case.codes) and steps == [] and ranges == [] and stats["divisions"] == 0 and calls == []
    # ... and so does a plan without ranges
    empty = guide.RefinePlan(False, plan.whole, np.zeros((0, 2), np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), [])
    final, steps, ranges, stats = refine.refine_planned(None, case.codes, case.tree, prm, case.thr, case.weight, empty, scorer=sc)
    assert np.array_equal(final, case.codes) and steps == [] and ranges == [] and calls == []


def test_ranges_of_fewer_than_two_groups_are_skipped():
    case = rp.Case(SHARDED)
    plan = case.plan()
    many = case.codes.shape[1]
    one = guide.Relation(True, [np.arange(many, dtype=np.int32)], np.array([-1], np.int32), np.array([-1], np.int32), np.array([-1], np.int32),
                         np.array([plan.whole.parent.tolist().index(-1)], np.int32), np.array([1.0]), np.array([1.0]))
    plan.relations = [one for _ in plan.relations]
    sc, calls, _keep = _counting_scorer()
    prm, _sm = case.alp.to_c()
    final, steps, ranges, stats = refine.refine_planned(None, case.codes, case.tree, prm, case.thr, case.weight, plan, scorer=sc)
    assert np.array_equal(final, case.codes) and steps == [] and calls == []
    assert len(ranges) == len(plan.ranges) and all(r["nsteps"] == 0 and r["groups"] == 1 and r["divisions"] == 0 for r in ranges)
    assert [[r["left"], r["right"], r["out_left"], r["out_right"]] for r in ranges] == [[l, r, l, r] for l, r in plan.ranges.tolist()]
