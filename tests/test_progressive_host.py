"""g2g_progressive on a machine without a GPU: the C++ driver -- tree validation, waves, the swapped member order, the error paths
and their clean-up -- with the CPU checker (oracle/) in the aligner's seat (proglib.oracle_aligner) and the PwdMs built on the
host, held to the reference's per-merge fixtures (tests/golden/progressive, tools/make_progressive_golden.py)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import proglib as pl
from prrn_aln_amd import guide
from prrn_aln_amd._lib import G2GError

NAMES = pl.names()
MODE, ARG = "rc=-2", "rc=-1"


@pytest.fixture(scope="module")
def runs():
    """every fixture once through the driver with the default max_batch: name -> (fixture, codes, order, merges, stats, batch sizes)"""
    out = {}
    for name in NAMES:
        g = pl.load(name)
        sizes = []
        res = guide.progressive(None, pl.seqs_of(g), pl.tree_of(g), pl.prm_of(g), aligner=pl.oracle_aligner(batches=sizes))
        out[name] = (g,) + res + (sizes,)
    return out


def test_the_fixture_set_is_whole():
    assert len(NAMES) == 9
    seen = set()
    for name in NAMES:
        g = pl.load(name)
        seen |= set(zip(g["node_mode"].tolist(), g["node_swp"].tolist()))
    # (a banded NTV merge never swaps: PwdM::selAlnMode swaps by length in NTV_ALN only)
    assert seen == {(6, 0), (10, 0), (7, 0), (8, 1), (9, 0), (9, 1)}


@pytest.mark.parametrize("name", NAMES)
def test_every_merge_is_the_reference_s(runs, name):
    g, codes, order, merges, stats, sizes = runs[name]
    pl.check_against_fixture(g, codes, order, merges)
    n = len(g["lens"])
    assert stats["merges"] == n - 1 == len(merges) and stats["waves"] == len(sizes) and stats["largest_wave"] == max(sizes)
    assert [m["wave"] for m in merges] == sorted(m["wave"] for m in merges) and merges[-1]["wave"] == stats["waves"] - 1
    assert all(m["t_ms"] >= 0 for m in merges)


@pytest.mark.parametrize("name", NAMES)
def test_max_batch_one_changes_nothing(runs, name):
    g, codes, order, merges, stats, _ = runs[name]
    sizes = []
    c1, o1, m1, s1 = guide.progressive(None, pl.seqs_of(g), pl.tree_of(g), pl.prm_of(g), max_batch=1, aligner=pl.oracle_aligner(batches=sizes))
    assert np.array_equal(c1, codes) and np.array_equal(o1, order)
    assert sizes == [1] * (len(g["lens"]) - 1) and s1["waves"] == s1["merges"] and s1["largest_wave"] == 1
    key = lambda m: (m["node"], m["left"], m["right"], m["na"], m["nb"], m["swp"], m["mode"], m["len"], m["scr"])
    assert sorted(map(key, m1)) == sorted(map(key, merges))


def test_one_aligner_call_per_wave(runs):
    assert runs["prot24_caterpillar"][5] == [1] * 23                 # a caterpillar: one DP per wave
    assert runs["prot8_gapfree"][5] == [4, 2, 1]                     # the balanced 8
    assert runs["prot3_leaf_left"][5] == [1, 1] and runs["prot2_unequal"][5] == [1]
    # the nodes of a wave are taken in ascending id
    g, _, _, merges, _, sizes = runs["prot16_indels"]
    at = 0
    for s in sizes:
        ids = [m["node"] for m in merges[at:at + s]]
        assert ids == sorted(ids)
        at += s


def test_a_single_sequence_comes_back_as_it_is():
    g = pl.load("prot2_unequal")
    s = pl.seqs_of(g)[0]
    tree = SimpleNamespace(left=[-1], right=[-1], parent=[-1])
    calls = [0]
    codes, order, merges, stats = guide.progressive(None, [s], tree, pl.prm_of(g), aligner=pl.oracle_aligner(calls=calls))
    assert np.array_equal(codes, s.reshape(-1, 1)) and order.tolist() == [0] and merges == [] and calls[0] == 0
    assert stats["merges"] == stats["waves"] == 0


def _tree8():
    g = pl.load("prot8_gapfree")
    return g, [np.array(g[k]) for k in ("tree_left", "tree_right", "tree_parent")]


def _break(what):
    g, (l, r, p) = _tree8()                                          # leaves 0 .. 7, nodes 8 .. 11 pair them, 12 = (8, 9), 13 = (10, 11), root 14
    node = None
    if what == "two roots":
        p[13] = -1; node = 14
    elif what == "no root":
        p[14] = 13; node = 14
    elif what == "leaf with sons":
        l[3], r[3] = 0, 1; node = 3
    elif what == "one son":
        r[12] = -1; node = 12
    elif what == "reached twice":
        r[13] = 8; p[11] = -1; node = 8
    elif what == "parent disagrees":
        p[9] = 13; node = 9
    elif what == "out of range":
        l[14] = 15; node = 14
    elif what == "own son":
        l[12] = 12; node = 12
    return g, SimpleNamespace(left=l, right=r, parent=p), node


@pytest.mark.parametrize("what", ["two roots", "no root", "leaf with sons", "one son", "reached twice", "parent disagrees", "out of range", "own son"])
def test_a_malformed_tree_is_refused_by_name(what):
    g, tree, node = _break(what)
    calls = [0]
    with pytest.raises(G2GError) as e:
        guide.progressive(None, pl.seqs_of(g), tree, pl.prm_of(g), aligner=pl.oracle_aligner(calls=calls))
    assert ARG in str(e.value) and "malformed tree" in str(e.value) and calls[0] == 0
    assert "node %d:" % node in str(e.value), str(e.value)


def test_a_tree_of_the_wrong_size_is_refused():
    g, (l, r, p) = _tree8()
    with pytest.raises(G2GError, match=ARG):
        guide.progressive(None, pl.seqs_of(g)[:7], SimpleNamespace(left=l, right=r, parent=p), pl.prm_of(g), aligner=pl.oracle_aligner())


@pytest.mark.parametrize("field,value", [("tgapf", 0.5), ("u0", 1.0), ("banded", 0)])
def test_mode_refusals_come_before_any_alignment(field, value):
    g = pl.load("prot3_leaf_left")
    prm = pl.prm_of(g)
    setattr(prm, field, value)
    calls = [0]
    with pytest.raises(G2GError, match=MODE):
        guide.progressive(None, pl.seqs_of(g), pl.tree_of(g), prm, aligner=pl.oracle_aligner(calls=calls))
    assert calls[0] == 0


def test_a_sequence_must_be_given_whole():
    from prrn_aln_amd import _abi
    from prrn_aln_amd._lib import last_error, lib
    g = pl.load("prot2_unequal")
    seqs = pl.seqs_of(g)
    ds = (_abi.DSeq * 2)(*[_abi.dseq(s) for s in seqs])
    ds[1].left = 3
    T, _keep = guide._tree_struct(pl.tree_of(g))
    O = _abi.ProgOpts()
    O.aligner = pl.oracle_aligner()
    out = _abi.c_u8p(); olen = C.c_int(); order = (C.c_int32 * 2)()
    prm = pl.prm_of(g)
    rc = lib().g2g_progressive(None, C.byref(prm), 2, ds, C.byref(T), C.byref(O), C.byref(out), C.byref(olen), order, None, None, None)
    assert rc == -1 and "sequence 1" in last_error() and not out


def test_no_context_and_no_aligner_is_refused():
    g = pl.load("prot2_unequal")
    with pytest.raises(G2GError, match=ARG):
        guide.progressive(None, pl.seqs_of(g), pl.tree_of(g), pl.prm_of(g))


def test_a_failing_aligner_ends_the_call_with_its_code():
    g = pl.load("prot8_gapfree")
    calls = [0]
    with pytest.raises(G2GError, match="rc=7") as e:
        guide.progressive(None, pl.seqs_of(g), pl.tree_of(g), pl.prm_of(g), aligner=pl.oracle_aligner(fail_at=1, calls=calls))
    assert calls[0] == 2 and "wave 1" in str(e.value)
    # ... and the driver is as good as new: the same call without the failure
    codes, order, merges, _ = guide.progressive(None, pl.seqs_of(g), pl.tree_of(g), pl.prm_of(g), aligner=pl.oracle_aligner())
    pl.check_against_fixture(g, codes, order, merges)


def test_a_dp_that_fails_names_its_node():
    """an aligner that reports a status for the second DP of the first wave: the call ends with that status, the node is named"""
    from prrn_aln_amd import _abi
    g = pl.load("prot8_gapfree")
    inner = pl.oracle_aligner()

    def cb(user, n, pw, scr, skl, nskl, status):
        rc = inner(user, n, pw, scr, skl, nskl, status)
        if n > 1:
            status[1] = pl.G2G_ERR_ENDS
        return rc
    with pytest.raises(G2GError, match="rc=-6") as e:
        guide.progressive(None, pl.seqs_of(g), pl.tree_of(g), pl.prm_of(g), aligner=_abi.ALIGN_FN(cb))
    assert "node 9" in str(e.value)


def test_the_restated_merge_orders_the_swapped_side_first():
    a = np.array([[3], [4], [5]], np.uint8); b = np.array([[6, 7], [8, 9]], np.uint8)
    skl = [(0, 0), (1, 0), (3, 2)]
    c, o = pl.merge((a, np.array([0])), (b, np.array([1, 2])), 0, skl)
    assert c.tolist() == [[3, 1, 1], [4, 6, 7], [5, 8, 9]] and o.tolist() == [0, 1, 2]
    c, o = pl.merge((b, np.array([1, 2])), (a, np.array([0])), 1, skl)
    assert c.tolist() == [[3, 1, 1], [4, 6, 7], [5, 8, 9]] and o.tolist() == [0, 1, 2]
