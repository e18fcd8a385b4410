"""The weighting tree over given groups without a GPU: the restatement (tests/ktreegrouplib.py) is pinned -- its closed form of the
group divergence against the reference's triple loop, and all of it against what the REFERENCE computed for the fixtures of
tests/golden/ktree_groups -- and g2g_ktree_from_dist_leaves (host code of libg2g.so) is held to the restatement bit for bit."""
import numpy as np
import pytest

import ktreegrouplib as kg
import ktreelib
from ktreelib import bits
from prrn_aln_amd.refine import KTree

FIXTURES = kg.fixtures()
IDS = [f["name"] for f in FIXTURES]
INT_KEYS = ("left", "right", "parent", "ndesc")
DBL_KEYS = ("height", "length", "res", "vol", "cur")


def same_tree(got: KTree, want: dict):
    for k in INT_KEYS:
        assert np.array_equal(np.asarray(getattr(got, k), np.int32), np.asarray(want[k], np.int32)), k
    for k in DBL_KEYS:
        assert np.array_equal(np.asarray(getattr(got, k), np.float64).view(np.int64), np.asarray(want[k], np.float64).view(np.int64)), k


def test_closed_form_equals_the_literal_loop():
    """320 seeded cases: 2 - 9 members in two groups with permuted member lists, 1 - 40 columns, run-structured gaps, nil codes in
    every third case; both group orders"""
    rng = np.random.default_rng(20)
    differ = 0
    for t in range(320):
        many, ln = int(rng.integers(2, 10)), int(rng.integers(1, 41))
        codes = kg.random_msa(rng, many, ln, nres=3, pnil=0.1 if t % 3 == 0 else 0.)
        ga, gb = kg.random_groups(rng, many, 2)
        fwd, bwd = kg.group_counts_literal(codes, ga, gb), kg.group_counts_literal(codes, gb, ga)
        assert kg.group_counts(codes, ga, gb) == fwd and kg.group_counts(codes, gb, ga) == bwd, (t, ga, gb)
        assert fwd[:3] == bwd[:3]                                      # mch / mmc / unp do not depend on the order ...
        differ += fwd[3] != bwd[3]
        pair_sum = np.sum([ktreelib.pairdvn_counts(codes[:, i], codes[:, j]) for i in ga for j in gb], axis=0)
        assert tuple(pair_sum[:3]) == fwd[:3]                          # ... and are the sums of the pairwise walks
    assert differ > 20                                                 # gap does depend on it


def test_singletons_are_the_pairwise_walk():
    rng = np.random.default_rng(21)
    codes = kg.random_msa(rng, 7, 60, pnil=0.05)
    _, want = ktreelib.divergence_scalar(codes)
    for counter in (kg.group_counts, kg.group_counts_literal):
        assert np.array_equal(kg.group_divergence(codes, [[m] for m in range(7)], counter)[1], want)


@pytest.mark.parametrize("case", FIXTURES, ids=IDS)
def test_restatement_reproduces_the_reference(case):
    """group distances, leaves, tree and weights of IterMsa::phyl_pwt as the reference's own parts computed them"""
    for flat, pfx in ((False, "tree_"), (True, "flat_")):
        tree, weight, sumwt, dist, counts = kg.phyl_pwt(case["codes"], case["groups"], flat)
        assert np.array_equal(bits(dist), bits(case["gdist"])) and np.array_equal(counts, case["gcounts"])
        for k in INT_KEYS:
            assert np.array_equal(np.asarray(tree[k], np.int32), case[pfx + k]), k
        for k in DBL_KEYS:
            assert np.array_equal(bits(tree[k]), bits(case[pfx + k])), k
        assert np.array_equal(bits(weight), bits(case[pfx + "weight"])) and bits([sumwt])[0] == bits(case[pfx + "sumwt"])[0]
    _, lit = kg.group_divergence(case["codes"], case["groups"], kg.group_counts_literal)
    assert np.array_equal(lit, case["gcounts"])


def test_fixtures_cover_what_they_were_made_for():
    by = {f["name"]: f for f in FIXTURES}
    assert len(by) == 9 and all(f["codes"].shape[1] <= 16 and f["codes"].shape[0] <= 400 for f in FIXTURES)
    tall = by["prot8_tall_leaf"]
    num = len(tall["groups"])
    assert tall["tree_leaf_height"][0] > tall["tree_height"][tall["tree_parent"][0]] and tall["tree_length"][0] == 0.
    assert (tall["tree_res"][num:] == ktreelib.EPS).any()
    assert (by["prot8_identical"]["gdist"] == 0).any()
    assert len(by["prot9_two_groups"]["groups"]) == 2
    assert all(len(g) == 1 for g in by["prot7_singletons"]["groups"])
    assert any((np.diff(g) < 0).any() for g in by["prot12_unsorted"]["groups"])
    assert int(by["dna10_4groups"]["molc"][0]) == 2


@pytest.mark.parametrize("case", FIXTURES, ids=IDS)
def test_from_dist_leaves_equals_the_restatement(case):
    for pfx in ("tree_", "flat_"):
        leaves = (case[pfx + "leaf_ndesc"], case[pfx + "leaf_height"], case[pfx + "leaf_res"])
        got = KTree.from_dist(case["gdist"], leaves=leaves)
        want = kg.tree_from_dist_leaves(case["gdist"], *leaves)
        same_tree(got, want)
        same_tree(got, {k: case[pfx + k] for k in INT_KEYS + DBL_KEYS})       # (= the reference's)
        assert got.root == want["root"] == len(got.left) - 1
        assert got.ndesc[got.root] == case["codes"].shape[1]
        bare = KTree.from_dist(case["gdist"], with_weights=False, leaves=leaves)
        assert bare.left == got.left and bare.height == got.height and not any(bare.vol) and not any(bare.cur)


def test_from_dist_leaves_on_seeded_random_leaves():
    """leaves taller than their merges, zero distances, ndesc of 0 (kept as 1): the clamped length, res = fepsilon and the
    a <= 0 / b <= 0 repairs of pairwt are reached"""
    rng = np.random.default_rng(22)
    clamped = eps = 0
    for t in range(60):
        num = int(rng.integers(2, 12))
        dist = rng.random(num * (num - 1) // 2) * (0.2 if t % 2 else 1.)
        if t % 5 == 0:
            dist[rng.integers(len(dist))] = 0.
        ndesc = rng.integers(0, 9, num).astype(np.int32)
        height = rng.random(num) * 0.3
        res = rng.random(num) * 0.2 * (t % 3 != 0)
        got = KTree.from_dist(dist, leaves=(ndesc, height, res))
        want = kg.tree_from_dist_leaves(dist, ndesc, height, res)
        same_tree(got, want)
        clamped += any(l == 0. for l in got.length[:num])
        eps += any(r == ktreelib.EPS for r in got.res[num:])
    assert clamped > 10 and eps > 3


def test_null_leaves_are_from_dist():
    """NULL arrays mean 1 / 0 / 0: the tree of g2g_ktree_from_dist, on the four fixtures of tests/golden/ktree"""
    cases = ktreelib.ktree_fixtures()
    assert len(cases) == 4
    for name, codes, ref in cases:
        dist, _ = ktreelib.divergence(codes)
        a, b = KTree.from_dist(dist), KTree.from_dist(dist, leaves=(None, None, None))
        same_tree(b, {k: getattr(a, k) for k in INT_KEYS + DBL_KEYS})
        assert (b.left, b.right, b.parent) == (ref["left"], ref["right"], ref["parent"])
        assert np.array_equal(bits(b.vol), bits(ref["vol"])) and np.array_equal(bits(b.cur), bits(ref["cur"]))
        many = codes.shape[1]
        c = KTree.from_dist(dist, leaves=(np.ones(many, np.int32), np.zeros(many), np.zeros(many)))
        same_tree(c, {k: getattr(a, k) for k in INT_KEYS + DBL_KEYS})


def test_refusals_without_a_device():
    """arguments are checked before the device is asked for; with good arguments and no context the answer is NODEVICE, never a
    host computation"""
    from prrn_aln_amd import guide
    from prrn_aln_amd._lib import G2GError, last_error
    codes = np.full((9, 6), 2, np.uint8)
    for groups, word in (([[0, 1, 2], [2, 4, 5]], "listed twice"), ([[0, 1, 2, 3, 4, 5]], "at least two"), ([[0, 1], [2, 3, 4]], "partition")):
        with pytest.raises(G2GError, match="rc=-1"):
            guide.msa_divergence_groups(None, codes, groups)
        assert word in last_error()
    with pytest.raises(G2GError, match="groups 0 and 1"):
        guide.msa_divergence_groups(None, np.full((512, 4096), 2, np.uint8), [np.arange(2048), np.arange(2048, 4096)])
    with pytest.raises(G2GError) as e:
        guide.msa_divergence_groups(None, codes, [[0, 1, 2], [3, 4, 5]])
    assert "rc=-1:" not in str(e.value) and "no device" in str(e.value)
    with pytest.raises(G2GError, match="no device"):
        KTree.from_msa_groups(None, codes, [[0, 1, 2], [3, 4, 5]])
    with pytest.raises(G2GError):
        KTree.from_dist([0.1, -0.2, 0.3], leaves=(None, None, None))
    assert "g2g_ktree_from_dist_leaves" in last_error()
