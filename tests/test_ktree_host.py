"""The weighting tree on the host: g2g_ktree_from_dist (UPGMA + teachparent + Kirchhoff weights, csrc/g2g_ktree.hip; needs no
device) against the trees the REFERENCE built -- every (MSA, tree) pair the refine and pairsum fixtures hold (26, the 256 x 5206
family included) and the edge cases of tests/golden/ktree (tools/make_ktree_golden.py) -- with the Python restatement
(tests/ktreelib.py) supplying the distances and the node values the traces do not record (height / length / res / ndesc).
Everything is compared bit for bit: no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

import ktreelib
from ktreelib import bits
from prrn_aln_amd import _abi
from prrn_aln_amd._lib import G2GError, last_error, lib
from prrn_aln_amd.refine import KTree

PAIRS = ktreelib.pairs()
IDS = [p[0] for p in PAIRS]
EDGE = ktreelib.ktree_fixtures()


def same_topology(t, ref):
    return all(list(getattr(t, k) if isinstance(t, KTree) else t[k]) == list(ref[k]) for k in ("left", "right", "parent"))


def assert_tree_equals_reference(t: KTree, ref: dict):
    assert same_topology(t, ref)
    assert np.array_equal(bits(t.vol), bits(ref["vol"])) and np.array_equal(bits(t.cur), bits(ref["cur"]))


def assert_tree_equals_restatement(t: KTree, r: dict):
    assert same_topology(t, r) and t.ndesc == r["ndesc"] and t.root == r["root"] == len(t.left) - 1
    for k in ("height", "length", "res", "vol", "cur"):
        assert np.array_equal(bits(getattr(t, k)), bits(r[k])), k


def test_exactly_the_26_pairs_are_loaded():
    assert len(PAIRS) == 26 and len(set(IDS)) == 26
    assert sum(1 for i in IDS if i.startswith("refine_")) == 5 and sum(1 for i in IDS if i.startswith("pairsum_")) == 21
    assert max(c.shape[1] for _, c, _ in PAIRS) == 256 and max(c.shape[0] for _, c, _ in PAIRS) == 5206


def test_excluded_cases_record_the_tree_of_case_0():
    """the reason the three pairsum cases are left out, checked: same tree as case #0, other rows"""
    import json
    import os
    for name, k in sorted(ktreelib.NOT_A_PAIR):
        f = json.load(open(os.path.join(ktreelib.GOLD, "pairsum", name + ".json")))
        assert f["cases"][k]["tree"] == f["cases"][0]["tree"] and f["cases"][k]["rows"] != f["cases"][0]["rows"]


def test_vectorised_walk_equals_the_column_by_column_walk():
    """ktreelib.divergence (numpy over columns and partners) against the plain loop, on gap-rich random MSAs with nil codes"""
    rng = np.random.default_rng(5)
    for many, ln in ((2, 1), (3, 7), (7, 90), (9, 300)):
        codes = rng.integers(2, 8, (ln, many)).astype(np.uint8)
        codes[rng.random((ln, many)) < 0.35] = 1
        codes[rng.random((ln, many)) < 0.05] = 0
        if ln > 60:
            codes[10:60, 0] = 1
            codes[30:80, 1] = 1
        d, c = ktreelib.divergence(codes)
        ds, cs = ktreelib.divergence_scalar(codes)
        assert np.array_equal(c, cs) and np.array_equal(bits(d), bits(ds))


@pytest.mark.parametrize("idx", range(len(PAIRS)), ids=IDS)
def test_restatement_reproduces_the_reference_tree(idx):
    ref = PAIRS[idx][2]
    t = ktreelib.restated(idx)[2]
    assert same_topology(t, ref)
    assert np.array_equal(bits(t["vol"]), bits(ref["vol"])) and np.array_equal(bits(t["cur"]), bits(ref["cur"]))


@pytest.mark.parametrize("idx", range(len(PAIRS)), ids=IDS)
def test_from_dist_reproduces_the_reference_tree(idx):
    dist, _, r = ktreelib.restated(idx)
    before = dist.copy()
    t = KTree.from_dist(dist)
    assert_tree_equals_reference(t, PAIRS[idx][2])
    assert_tree_equals_restatement(t, r)
    assert np.array_equal(bits(dist), bits(before))                    # (d) the caller's distances are untouched
    assert t.n_leaves == PAIRS[idx][1].shape[1]


@pytest.mark.parametrize("idx", [0, 4, len(PAIRS) - 1], ids=lambda i: IDS[i])
def test_without_weights_same_topology_and_zero_weights(idx):
    dist, _, r = ktreelib.restated(idx)
    t = KTree.from_dist(dist, with_weights=False)
    assert same_topology(t, r) and t.ndesc == r["ndesc"]
    for k in ("height", "length", "res"):
        assert np.array_equal(bits(getattr(t, k)), bits(r[k])), k
    assert not any(t.vol) and not any(t.cur)
    assert np.array_equal(bits(t.vol), bits(np.zeros(len(t.vol))))


def test_input_distances_are_not_modified_even_read_only():
    d = np.array([0.5, 0.25, 0.75, 0.125, 0.5, 0.25], np.float64)       # 4 members; UPGMA averages rows in its own copy
    keep = d.copy()
    KTree.from_dist(d)
    assert np.array_equal(bits(d), bits(keep))


def test_two_members():
    """prrn builds no tree for two members (tools/make_ktree_golden.py), so this is pinned on the restatement and on what
    upg_method / pairwt give by hand: one merge at height d / 2, every cur 1, every vol 1"""
    for d in (0.375, 0.0):
        t = KTree.from_dist([d])
        assert_tree_equals_restatement(t, ktreelib.tree_from_dist([d]))
        assert (t.left, t.right, t.parent, t.ndesc, t.root) == ([-1, -1, 0], [-1, -1, 1], [2, 2, -1], [1, 1, 2], 2)
        assert t.height == [0., 0., d / 2] and t.length == [d / 2, d / 2, 0.]
        assert t.res[2] == ((d / 2) * (d / 2) / (d / 2 + d / 2) if d else 1e-7)
        assert t.vol == [1., 1., 1.] and t.cur == [1., 1., 1.]


@pytest.mark.parametrize("k", range(len(EDGE)), ids=[e[0] for e in EDGE])
def test_edge_fixtures_from_the_reference(k):
    name, codes, ref = EDGE[k]
    dist, _ = ktreelib.divergence(codes)
    r = ktreelib.tree_from_dist(dist)
    assert same_topology(r, ref) and np.array_equal(bits(r["vol"]), bits(ref["vol"])) and np.array_equal(bits(r["cur"]), bits(ref["cur"]))
    t = KTree.from_dist(dist)
    assert_tree_equals_reference(t, ref)
    assert_tree_equals_restatement(t, r)


def test_edge_fixture_set():
    names = {e[0] for e in EDGE}
    assert names == {"trio3", "pair2_refused_trio3_with_twin", "dup8_two_clusters", "dup8_all_twins"}
    assert {e[1].shape[1] for e in EDGE} == {3, 8}


def test_duplicated_members_take_the_degenerate_branch():
    """twins: distance 0 -> merged at height 0 with res = fepsilon, and pairwt's `a + b <= fepsilon` branch halves the current"""
    by = {e[0]: e for e in EDGE}
    _, codes, ref = by["dup8_all_twins"]
    dist, _ = ktreelib.divergence(codes)
    many = codes.shape[1]
    t = KTree.from_dist(dist)
    for a in range(0, many, 2):
        assert dist[ktreelib.elem(a, a + 1)] == 0.
        p = t.parent[a]
        assert t.parent[a + 1] == p and (t.left[p], t.right[p]) == (a, a + 1)
        assert t.height[p] == 0. and t.res[p] == 1e-7 and t.length[a] == 0. and t.length[a + 1] == 0.
        assert t.cur[a] == 0.5 and t.cur[a + 1] == 0.5 and ref["cur"][a] == 0.5
    _, codes, ref = by["dup8_two_clusters"]                              # three copies: the second merge is degenerate too
    t = KTree.from_dist(ktreelib.divergence(codes)[0])
    assert [t.cur[i] for i in (0, 1, 2, 4, 5)] == [0.5] * 5 and t.height[t.parent[t.parent[0]]] == 0.
    assert_tree_equals_reference(t, ref)


def _rc_from_dist(many, dist):
    d = np.ascontiguousarray(dist, np.float64)
    T = _abi.KTreeOut()
    rc = lib().g2g_ktree_from_dist(many, d.ctypes.data_as(_abi.c_f64p), 1, C.byref(T))
    if rc == 0:
        lib().g2g_ktree_free(C.byref(T))
    return rc


def test_bad_arguments():
    ERR_ARG = -1
    assert _rc_from_dist(3, [0.5, float("nan"), 0.25]) == ERR_ARG
    assert "members 0 and 2" in last_error()                            # entry 1 = elem(0, 2)
    assert _rc_from_dist(3, [0.5, 0.5, -0.25]) == ERR_ARG
    assert "members 1 and 2" in last_error() and "negative" in last_error()
    assert _rc_from_dist(1, [0.]) == ERR_ARG and _rc_from_dist(0, [0.]) == ERR_ARG and _rc_from_dist(4097, [0.]) == ERR_ARG
    assert lib().g2g_ktree_from_dist(3, None, 1, C.byref(_abi.KTreeOut())) == ERR_ARG
    with pytest.raises(G2GError):
        KTree.from_dist([0.5, float("nan"), 0.25])
    with pytest.raises(ValueError):
        KTree.from_dist([0.5, 0.5])                                     # two distances are no whole family
    assert lib().g2g_msa_divergence(None, 3, 5, None, None, None) == ERR_ARG
    lib().g2g_ktree_free(None)                                          # (a no-op)


def test_five_argument_constructor_still_valid():
    t = KTree([-1, -1, 0], [-1, -1, 1], [2, 2, -1], [1., 1., 1.], [1., 1., 1.])
    assert t.n_leaves == 2 and t.height is None and t.root is None
    T, keep = t.to_c()
    assert T.n_nodes == 3
