"""Test-side helpers for g2g_refine_planned (prrn's default refinement: fused groups, one loop per unconserved column range): loading
tests/golden/refine_plan/*.json, the plan as tests/fuselib.py restates it turned into the object the product takes, and a run of the
C++ loop with the CPU CHECKER in the GPU's seat (refinelib.oracle_scorer), so that everything but the plan-making runs without a GPU.

A fixture holds (tools/make_refine_plan_golden.py says which binary gave which field): the start rows, the member tree and the member
weights, the parameters of the plan (the reference's localprm with its similarity matrix) and of the DPs (molc, ls), the attack ranges
and the `Prrn` lines the reference printed, the final rows, and for a TRACED case per range the branches, every align2 and every
accepted move."""
from __future__ import annotations

import ctypes as C
import glob
import json
import os

import numpy as np

import consreglib as cl
import fuselib as fl
import refinelib
from prrn_aln_amd import _abi, guide, refine
from prrn_aln_amd import operator as op
from prrn_aln_amd._lib import lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refine_plan")
GAIN_BOUND = 0.11          # the two printed numbers are rounded to 0.1 each: 0.05 + 0.05, and slack for the sum's own rounding


def fixtures(kind=None):
    out = []
    for p in sorted(glob.glob(os.path.join(GOLD, "*.json"))):
        if kind is None or os.path.basename(p).startswith(kind + "_"):
            out.append(p)
    return out


def fixture_id(path):
    return os.path.basename(path)[:-5]


class Case:
    """one fixture, ready to run"""

    def __init__(self, path):
        f = self.f = json.load(open(path))
        self.name = f["name"]
        self.molc = f["molc"]
        self.codes = op.encode(f["rows"], f["molc"])
        self.final = op.encode(f["final_rows"], f["molc"])
        t = f["tree"]
        self.tree = refine.KTree(t["left"], t["right"], t["parent"], t["vol"], t["cur"])
        self.tree5 = tuple(np.asarray(t[k], np.int32 if k in ("left", "right", "parent") else np.float64) for k in ("left", "right", "parent", "vol", "cur"))
        self.weight = np.asarray(f["weight"], np.float64)
        self.thr = float(f["thr"])
        # the plan's parameters: the reference's localprm (consreg.cc:39-40) and similarity matrix number 1
        self.alp_plan = cl.alp_of(dict(molc=[f["molc"]], max_code=[f["max_code"]], u=[f["plan_u"]], v=[f["plan_v"]], simmtx=np.asarray(f["plan_simmtx"], np.float64)))
        # the DPs': prrn's alignment defaults
        self.alp = op.AlnParam(ls=f["ls"], molc=f["molc"], max_code=f["max_code"])
        self._plan = None

    def restated(self):
        """tests/fuselib.py's plan of the start MSA (a dict)"""
        if self._plan is None:
            self._plan = fl.plan(self.codes, self.tree5, self.alp_plan, self.thr, self.weight)
        return self._plan

    def plan(self):
        return plan_object(self.restated())

    def printed(self):
        """the reference's `Prrn` lines by range index: {r: dict(left1, right1, sps, initsp, groups, rep)}"""
        return {int(p["range"]): p for p in self.f["prrn"]}

    def merged_trace(self):
        """a traced case's ranges in processing order as ONE dict with the keys refinelib.check_against_trace reads"""
        f = self.f
        out = dict(rows=f["rows"], molc=f["molc"], final_rows=f["final_rows"], branches=[], align2=[], accepted=[])
        for t in f["trace"]:
            for k in ("branches", "align2", "accepted"):
                out[k] += t[k]
        return out


def _relation(fused, rel, origin):
    groups, tl, tr, tp, vol, cur = rel
    return guide.Relation(bool(fused), [np.asarray(g, np.int32) for g in groups], np.asarray(tl, np.int32), np.asarray(tr, np.int32),
                          np.asarray(tp, np.int32), np.asarray(origin, np.int32), np.asarray(vol, np.float64), np.asarray(cur, np.float64))


def plan_object(pl):
    """fuselib.plan's dict as the guide.RefinePlan the product takes"""
    return guide.RefinePlan(bool(pl["nothing"]), _relation(*pl["whole"]), np.asarray(pl["ranges"], np.int32).reshape(-1, 2),
                            np.asarray(pl["at_left"], np.int32), np.asarray(pl["at_right"], np.int32), [_relation(*r) for r in pl["per_range"]])


def trivial_plan(tree, many, ln):
    """one range [0, len), nothing fused: what g2g_refine refines"""
    rel = guide.Relation(False, [np.array([m], np.int32) for m in range(many)], np.asarray(tree.left, np.int32), np.asarray(tree.right, np.int32),
                         np.asarray(tree.parent, np.int32), np.arange(2 * many - 1, dtype=np.int32), np.asarray(tree.vol, np.float64), np.asarray(tree.cur, np.float64))
    return guide.RefinePlan(False, rel, np.array([[0, ln]], np.int32), np.array([1], np.int32), np.array([1], np.int32), [rel])


def same_relation(a, b):
    assert a.fused == b.fused and len(a.groups) == len(b.groups)
    assert all(np.array_equal(x, y) for x, y in zip(a.groups, b.groups))
    for k in ("left", "right", "parent", "origin"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in ("vol", "cur"):
        assert np.array_equal(getattr(a, k).view(np.int64), getattr(b, k).view(np.int64)), k


def same_plan(a, b):
    assert a.nothing_to_refine == b.nothing_to_refine
    same_relation(a.whole, b.whole)
    assert np.array_equal(a.ranges, b.ranges) and np.array_equal(a.at_left, b.at_left) and np.array_equal(a.at_right, b.at_right)
    assert len(a.relations) == len(b.relations)
    for x, y in zip(a.relations, b.relations):
        same_relation(x, y)


def weight_recording_scorer(record, **kw):
    """refinelib.oracle_scorer, noting before each DP the member weights of both sides of its PwdM: record gets (weights of a, of b)"""
    inner = refinelib.oracle_scorer(**kw)
    L = lib()

    def cb(user, n, pw, cur, ncur, scr, skl, nskl, raw_cur, val_new):
        for i in range(n):
            p = L.g2g_pwdm_problem(pw[i]).contents
            record.append(tuple([side.weight[k] for k in range(side.many)] if side.weight else [] for side in (p.a, p.b)))
        return inner(user, n, pw, cur, ncur, scr, skl, nskl, raw_cur, val_new)
    return _abi.SCORE_FN(cb), inner


def run_host(case, plan=None, **opts):
    """g2g_refine_planned with the CPU checker scoring: (final, steps, ranges, stats)"""
    scorer = opts.pop("scorer", None) or refinelib.oracle_scorer()
    plan = case.plan() if plan is None else plan
    prm, _sm = case.alp.to_c()                  # (_sm: the matrix prm points into)
    return refine.refine_planned(None, case.codes, case.tree, prm, case.thr, case.weight, plan, scorer=scorer, **opts)


def check_ranges_against_print(case, ranges, gain=True):
    """per range: groups and divisions (the reference's countaln) as printed; a range without a printed line ran nothing"""
    pr = case.printed()
    for rs in ranges:
        p = pr.get(rs["range"])
        if p is None:
            assert rs["nsteps"] == 0 and rs["groups"] < 2, rs
            continue
        assert (rs["groups"], rs["divisions"]) == (p["groups"], p["rep"]), (rs, p)
        assert (rs["out_left"] + 1, rs["out_right"]) == (p["left1"], p["right1"]), (rs, p)
        if gain:
            print("%s range %d: gain %.6f, printed sps - initsp %.1f" % (case.name, rs["range"], rs["gain"], p["sps"] - p["initsp"]))
            assert abs(rs["gain"] - (p["sps"] - p["initsp"])) <= GAIN_BOUND, (rs, p)


def same_steps(a, b):
    """two runs' steps: branch, skipped, accepted, and the three doubles with =="""
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in ("branch", "skipped", "accepted", "scr", "val_new", "val_old"):
            assert x[k] == y[k], (k, x, y)
