"""The weighting tree over given groups and the refinement between them, end to end on the GPU: KTree.from_msa_groups
(g2g_ktree_from_msa_groups: group and member divergences on the device, trees and weights on the host) against what the REFERENCE
computed for tests/golden/ktree_groups, guide.refine_plan(groups=) against the restated plan, and refine.refine_groups against the
CPU-checker run of tests/test_refine_groups_host.py -- the same trajectory, the same MSA, every group's rows as they came."""
import numpy as np
import pytest

import ktreegrouplib as kg
import refinelib
import refineplanlib as rp
from ktreelib import bits
from prrn_aln_amd import engine, guide, refine
from prrn_aln_amd.refine import KTree
from test_ktree_groups_host import DBL_KEYS, FIXTURES, IDS, INT_KEYS, same_tree
from test_refine_groups_host import SINGLETON_CASES, family_run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


def quiet(ctx, fn):
    """fn() with the scheduler's counters watched: no wait gave up, no DP was re-run"""
    c0 = ctx.counters()
    out = fn()
    c1 = ctx.counters()
    assert c1["wait_timeouts"] == c0["wait_timeouts"] and c1["recovered_dps"] == c0["recovered_dps"], ctx.last_timeout()
    assert out[3]["wait_timeouts"] == 0 and out[3]["recovered_dps"] == 0
    return out


@pytest.mark.parametrize("case", FIXTURES, ids=IDS)
def test_from_msa_groups_reproduces_the_reference(ctx, case):
    for flat, pfx in ((False, "tree_"), (True, "flat_")):
        tree, weight = KTree.from_msa_groups(ctx, case["codes"], case["groups"], flat_leaves=flat)
        same_tree(tree, {k: case[pfx + k] for k in INT_KEYS + DBL_KEYS})
        assert np.array_equal(bits(weight), bits(case[pfx + "weight"]))
        assert tree.root == len(tree.left) - 1 and tree.ndesc[tree.root] == case["codes"].shape[1]
    if all(len(g) == 1 for g in case["groups"]):                        # singletons: Ktree(msd) + calcpw of the members in that order
        order = [int(g[0]) for g in case["groups"]]
        plain = KTree.from_msa(ctx, case["codes"][:, order])
        same_tree(tree, {k: getattr(plain, k) for k in INT_KEYS + DBL_KEYS})


def test_the_plan_from_given_groups(ctx):
    F = family_run()
    prm, _sm = F["alp"].to_c()
    tree, weight = KTree.from_msa_groups(ctx, F["codes"], F["groups"])
    same_tree(tree, F["tree"])
    assert np.array_equal(bits(weight), bits(F["weight"]))
    rp.same_plan(guide.refine_plan(ctx, F["codes"], tree, prm, 35., weight, groups=F["groups"]), rp.plan_object(F["plan"]))


def test_refine_groups_walks_the_host_trajectory(ctx):
    F = family_run()
    prm, _sm = F["alp"].to_c()
    h_final, h_steps, h_ranges, h_stats = F["res"]
    final, steps, ranges, stats, tree, weight = quiet(ctx, lambda: refine.refine_groups(ctx, F["codes"], F["groups"], prm, 35., window=8))
    same_tree(tree, F["tree"])
    assert np.array_equal(bits(weight), bits(F["weight"]))
    assert np.array_equal(final, h_final)
    rp.same_steps(steps, h_steps)
    for a, b in zip(ranges, h_ranges):
        assert {k: v for k, v in a.items() if k != "gain"} == {k: v for k, v in b.items() if k != "gain"} and a["gain"] == b["gain"]
    assert stats["accepted"] == h_stats["accepted"] >= 1 and stats["batches"] < len(steps)
    for g in F["groups"]:
        assert np.array_equal(kg.rows_without_common_gaps(final, g), kg.rows_without_common_gaps(F["codes"], g))


@pytest.mark.parametrize("path", SINGLETON_CASES, ids=[rp.fixture_id(p) for p in SINGLETON_CASES])
def test_singleton_groups_are_refine_planned(ctx, path):
    """tree, weights and plan made on the device from singleton groups, against refine_planned on the tree of KTree.from_msa: one
    trajectory -- and, the fixture's tree being that tree, the reference's final alignment"""
    case = rp.Case(path)
    many = case.codes.shape[1]
    prm, _sm = case.alp.to_c()
    pprm, _psm = case.alp_plan.to_c()
    plain = KTree.from_msa(ctx, case.codes)
    w = np.asarray(plain.vol[:many], np.float64)
    assert (plain.left, plain.right, plain.parent) == (case.tree.left, case.tree.right, case.tree.parent)
    a = quiet(ctx, lambda: refine.refine_planned(ctx, case.codes, plain, prm, case.thr, w, plan=None, plan_prm=pprm, window=16))
    b = quiet(ctx, lambda: refine.refine_groups(ctx, case.codes, [[m] for m in range(many)], prm, case.thr, plan_prm=pprm, window=16))
    same_tree(b[4], {k: getattr(plain, k) for k in INT_KEYS + DBL_KEYS})
    assert np.array_equal(bits(b[5]), bits(w))
    assert np.array_equal(a[0], b[0]) and np.array_equal(b[0], case.final)
    rp.same_steps(a[1], b[1])
    assert a[2] == b[2] and len(a[1]) > 0
