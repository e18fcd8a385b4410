"""g2g_refine_planned_groups on the CPU: the refinement between groups the caller brings, with the CPU CHECKER in the scorer's seat
(refinelib.oracle_scorer) and the plan as tests/fuselib.py restates it.  No trajectory of the reference exists for given groups
(its -G path reads weights it never set): what stands in is the equivalence with g2g_refine_planned where the
groups are single members -- there the fixtures of tests/golden/refine_plan hold the reference's trajectory -- and the property
the stage is for: every group's rows leave as they came."""
import numpy as np
import pytest

import ktreegrouplib as kg
import refinelib
import refineplanlib as rp
from prrn_aln_amd import guide, refine
from prrn_aln_amd import operator as op
from prrn_aln_amd._lib import G2GError, lib

G2G_ERR_ARG, G2G_ERR_MODE = -1, -2
SINGLETON_CASES = [p for p in rp.fixtures() if rp.fixture_id(p) in ("traced_prot6x260", "grouped_prot6x260")]
_FAMILY = {}


def family_run():
    """the 10-member family in groups of 4, 3, 1, 2: tree and weights by the restatement of phyl_pwt, the plan by fuselib started
    from the groups, one run with the CPU checker -- shared with tests/test_gpu_refine_groups.py"""
    if not _FAMILY:
        codes, groups = kg.family_in_groups()
        tree, weight, _, _, _ = kg.phyl_pwt(codes, groups)
        alp = op.AlnParam()
        pl = kg.plan_groups(codes, groups, tree, alp, 35., weight)
        kt = refine.KTree(tree["left"], tree["right"], tree["parent"], tree["vol"], tree["cur"])
        prm, _sm = alp.to_c()
        res = refine.refine_planned(None, codes, kt, prm, 35., weight, rp.plan_object(pl), groups=groups, scorer=refinelib.oracle_scorer(),
                                    window=8, want_moves=True)
        _FAMILY.update(codes=codes, groups=groups, tree=tree, kt=kt, weight=weight, alp=alp, plan=pl, res=res)
    return _FAMILY


def test_the_entries_exist():
    assert len(SINGLETON_CASES) == 2
    assert lib().g2g_refine_planned_groups and lib().g2g_refine_plan_groups and callable(refine.refine_groups)


@pytest.mark.parametrize("path", SINGLETON_CASES, ids=[rp.fixture_id(p) for p in SINGLETON_CASES])
def test_singleton_groups_are_g2g_refine_planned(path):
    case = rp.Case(path)
    f0, s0, r0, st0 = rp.run_host(case, want_moves=True, window=8)
    many = case.codes.shape[1]
    prm, _sm = case.alp.to_c()
    f1, s1, r1, st1 = refine.refine_planned(None, case.codes, case.tree, prm, case.thr, case.weight, case.plan(), groups=[[m] for m in range(many)],
                                            scorer=refinelib.oracle_scorer(), want_moves=True, window=8)
    assert np.array_equal(f0, f1) and np.array_equal(f1, case.final)
    rp.same_steps(s0, s1)
    assert [(s["na"], s["nb"], s["swp"], s["delta"]) for s in s0] == [(s["na"], s["nb"], s["swp"], s["delta"]) for s in s1]
    assert r0 == r1 and len(r1) == len(case.f["ranges"])
    assert all(a[:3] == b[:3] and np.array_equal(a[3], b[3]) for a, b in zip(st0["moves"], st1["moves"]))
    assert {k: v for k, v in st0.items() if k != "moves"} == {k: v for k, v in st1.items() if k != "moves"}


def test_given_groups_leave_as_they_came():
    F = family_run()
    codes, groups = F["codes"], F["groups"]
    final, steps, ranges, stats = F["res"]
    assert codes.shape[1] == 10 and [len(g) for g in groups] == [4, 3, 1, 2]
    assert stats["accepted"] >= 1 and not np.array_equal(final, codes)         # something moved ...
    for g in groups:                                                            # ... between the groups, nothing inside one
        assert np.array_equal(kg.rows_without_common_gaps(final, g), kg.rows_without_common_gaps(codes, g))
    assert (final > 1).any(1).all()                                            # no all-gap column is left
    for m in range(10):                                                        # every member's residues, in order
        assert np.array_equal(final[:, m][final[:, m] > 1], codes[:, m][codes[:, m] > 1])
    # the divisions are divisions of the groups: both sides of every accepted move are unions of them
    assert all(r["groups"] <= 4 and r["cycle"] == max(2 * r["groups"] - 3, 0) for r in ranges)
    for br, la, lb, skl in stats["moves"]:
        assert sorted(la + lb) == list(range(10))
        for g in groups:
            assert set(g.tolist()) <= set(la) or set(g.tolist()) <= set(lb)


def test_a_plan_that_divides_a_group_is_refused():
    F = family_run()
    many = F["codes"].shape[1]
    prm, _sm = F["alp"].to_c()
    whole = refine.KTree.from_dist(np.linspace(0.1, 0.9, many * (many - 1) // 2))   # any tree over the ten members
    plan = rp.trivial_plan(whole, many, F["codes"].shape[0])                         # ... whose plan has every member alone
    with pytest.raises(G2GError, match=r"rc=%d.*divides group 0" % G2G_ERR_ARG):
        refine.refine_planned(None, F["codes"], F["kt"], prm, 35., F["weight"], plan, groups=F["groups"], scorer=refinelib.oracle_scorer())


def test_refusals():
    F = family_run()
    prm, _sm = F["alp"].to_c()
    plan = rp.plan_object(F["plan"])
    sc = refinelib.oracle_scorer()
    run = lambda **kw: refine.refine_planned(None, F["codes"], kw.pop("tree", F["kt"]), kw.pop("prm", prm), 35., F["weight"], kw.pop("plan", plan),
                                             groups=kw.pop("groups", F["groups"]), **kw)
    with pytest.raises(G2GError, match=r"rc=%d.*context" % G2G_ERR_ARG):       # no context: the caller gives the plan and the scorer
        run()
    with pytest.raises(G2GError, match=r"rc=%d.*context" % G2G_ERR_ARG):
        run(plan=None, scorer=sc)
    with pytest.raises(G2GError, match=r"rc=%d.*malformed groups" % G2G_ERR_ARG):
        run(groups=[[0, 3, 1, 2], [6, 4, 5], [7], [9, 9]], scorer=sc)
    with pytest.raises(G2GError, match=r"rc=%d.*2 \* num - 1" % G2G_ERR_ARG):  # the tree must be the tree over the groups
        run(tree=refine.KTree.from_dist(np.linspace(0.1, 0.9, 45)), scorer=sc)
    with pytest.raises(G2GError, match=r"rc=%d.*fewer than two groups" % G2G_ERR_ARG):
        run(groups=[list(range(10))], scorer=sc)
    for kw, what in ((dict(tgapf=0.5), "terminal-gap"), (dict(u0=1.0), "ether"), (dict(banded=0), "banded")):
        bad, _keep = op.AlnParam(**kw).to_c()
        with pytest.raises(G2GError, match=r"rc=%d.*%s" % (G2G_ERR_MODE, what)):
            run(prm=bad, scorer=sc)
    with pytest.raises(G2GError, match=r"g2g_refine_plan_groups rc=%d" % G2G_ERR_ARG):     # the plan needs a context
        guide.refine_plan(None, F["codes"], F["kt"], prm, 35., F["weight"], groups=F["groups"])
