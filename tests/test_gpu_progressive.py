"""g2g_progressive on the GPU: the waves' PwdMs built on the device (g2g_pwdm_create_batch) and their DPs run as one
g2g_align2_batch each, held merge by merge to the reference's fixtures (tests/golden/progressive) and, on a larger family with
modes mixed inside one batch, to the run with the CPU checker in the aligner's seat; align_sequences against the hand-made chain of
its calls."""
import numpy as np
import pytest

import proglib as pl
from prrn_aln_amd import engine, guide
from prrn_aln_amd import operator as op
from prrn_aln_amd._lib import G2GError
from prrn_aln_amd.refine import KTree
from prrn_aln_amd.synth import make_family

pytestmark = pytest.mark.gpu
NAMES = pl.names()


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


def report(name, stats):
    # reported, not asserted: the suite's own last test judges time-outs
    print("%s: %d merges in %d waves (largest %d), wait_timeouts %d, recovered_dps %d"
          % (name, stats["merges"], stats["waves"], stats["largest_wave"], stats["wait_timeouts"], stats["recovered_dps"]))


@pytest.mark.parametrize("name", NAMES)
def test_every_merge_is_the_reference_s(ctx, name):
    g = pl.load(name)
    c0 = ctx.counters()
    codes, order, merges, stats = guide.progressive(ctx, pl.seqs_of(g), pl.tree_of(g), pl.prm_of(g))
    pl.check_against_fixture(g, codes, order, merges)
    assert stats["merges"] == len(g["lens"]) - 1 and ctx.counters()["runs"] > c0["runs"]          # the DPs ran on the device
    report(name, stats)


def test_the_fixtures_are_all_here():
    assert len(NAMES) == 9


def test_max_batch_one_changes_nothing(ctx):
    g = pl.load("prot16_indels")
    a = guide.progressive(ctx, pl.seqs_of(g), pl.tree_of(g), pl.prm_of(g))
    b = guide.progressive(ctx, pl.seqs_of(g), pl.tree_of(g), pl.prm_of(g), max_batch=1)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert a[3]["waves"] < b[3]["waves"] == b[3]["merges"] == 15 and a[3]["largest_wave"] > 1 == b[3]["largest_wave"]
    key = lambda m: (m["node"], m["na"], m["nb"], m["swp"], m["mode"], m["len"], m["scr"])
    assert sorted(map(key, a[2])) == sorted(map(key, b[2]))


@pytest.fixture(scope="module")
def family32():
    alp = op.AlnParam()
    fam = make_family(32, 200, 5, indel=0.02, sub=0.15)
    return alp, [op.encode([s], op.PROTEIN).reshape(-1) for s in fam.seqs]


def test_a_larger_family_against_the_cpu_checker(ctx, family32):
    alp, seqs = family32
    prm, _sm = alp.to_c()
    tree = KTree.from_dist(guide.kmer_distance(ctx, seqs, op.PROTEIN, k=3), with_weights=False)
    dev = guide.progressive(ctx, seqs, tree, prm)
    cpu = guide.progressive(None, seqs, tree, prm, aligner=pl.oracle_aligner())
    assert np.array_equal(dev[0], cpu[0]) and np.array_equal(dev[1], cpu[1])
    strip = lambda ms: [{k: v for k, v in m.items() if k != "t_ms"} for m in ms]
    assert strip(dev[2]) == strip(cpu[2])                                # node, sons, sides, swp, mode, wave, length, bit-equal score
    waves = {}
    for m in dev[2]:
        waves.setdefault(m["wave"], set()).add(m["mode"])
    assert dev[3]["largest_wave"] >= 8 and any(len(s) > 1 for s in waves.values())    # modes mixed inside one batch
    for k in range(32):
        assert np.array_equal(pl.degap(dev[0][:, k]), seqs[dev[1][k]])
    report("synthetic 32 x 200", dev[3])


@pytest.mark.parametrize("distance", ["kmer", "dp"])
def test_align_sequences_is_the_chain_of_its_calls(ctx, family32, distance):
    alp, seqs = family32
    seqs = seqs[:12]
    prm, sm = alp.to_c()
    dist = guide.kmer_distance(ctx, seqs, op.PROTEIN) if distance == "kmer" else guide.distance_matrix(ctx, prm, seqs, sm)
    tree = KTree.from_dist(dist, with_weights=False)
    codes, order, _merges, _stats = guide.progressive(ctx, seqs, tree, prm)
    raw, t1, o1 = guide.align_sequences(ctx, seqs, op.PROTEIN, alp, distance=distance, input_order=False)
    assert np.array_equal(raw, codes) and np.array_equal(o1, order) and (t1.left, t1.right, t1.parent) == (tree.left, tree.right, tree.parent)
    assert sorted(order.tolist()) == list(range(12)) and order.tolist() != list(range(12))
    msa, t2, o2 = guide.align_sequences(ctx, seqs, op.PROTEIN, alp, distance=distance)
    assert o2.tolist() == list(range(12)) and t2.left == tree.left
    for k in range(12):
        assert np.array_equal(msa[:, order[k]], codes[:, k])             # input_order: member order[k] of the input stands in column order[k]
        assert np.array_equal(pl.degap(msa[:, k]), seqs[k])
    assert not (msa <= pl.GAP).all(axis=1).any()                         # no all-gap column


def test_a_failing_aligner_leaks_nothing(ctx):
    g = pl.load("prot16_indels")                                         # six waves; from the third on the sons are groups with gaps
    good = lambda: guide.progressive(ctx, pl.seqs_of(g), pl.tree_of(g), pl.prm_of(g), aligner=pl.oracle_aligner())
    good()
    good()
    c1 = ctx.mem_counters()
    with pytest.raises(G2GError, match="rc=7"):
        guide.progressive(ctx, pl.seqs_of(g), pl.tree_of(g), pl.prm_of(g), aligner=pl.oracle_aligner(fail_at=3))
    c2 = ctx.mem_counters()
    # what the waves' groups took on the device is back in the context's pool
    assert c2["hip_malloc"] - c2["hip_free"] == c1["hip_malloc"] - c1["hip_free"] and c2["pool_free_bytes"] == c1["pool_free_bytes"]
    codes, order, merges, _ = good()
    pl.check_against_fixture(g, codes, order, merges)
