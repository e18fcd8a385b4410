"""The group divergence on the GPU: g2g_msa_divergence_groups (csrc/g2g_ktree_groups.hip: the member-pair kernel for mch / mmc /
unp, one lane per (member, other group) walking the columns in chunks of KG_CHUNK = 8 for the gap count, one wave per group pair
for the sums) against the restatement of the reference's group pairdvn (tests/ktreegrouplib.py): counts equal as integers,
distances equal as bit patterns."""
import ctypes as C

import numpy as np
import pytest

import ktreegrouplib as kg
import ktreelib
from ktreelib import bits
from prrn_aln_amd import _abi, engine, guide
from prrn_aln_amd._lib import last_error, lib

pytestmark = pytest.mark.gpu
T = 8                                                                   # KG_CHUNK: the columns a lane fetches before it walks them


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


def same_dist(got, want):
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got[~nan]), bits(want[~nan]))


def check(ctx, codes, groups, counter=kg.group_counts):
    want_d, want_c = kg.group_divergence(codes, groups, counter)
    got_d, got_c = guide.msa_divergence_groups(ctx, codes, groups)
    assert np.array_equal(got_c, want_c), (got_c[:4], want_c[:4])
    assert same_dist(got_d, want_d)
    return got_c


def split(sizes, order=None):
    """consecutive members in groups of the given sizes; order: a permutation of the members to deal them from"""
    many = sum(sizes)
    src = np.arange(many, dtype=np.int32) if order is None else np.asarray(order, np.int32)
    cuts = np.cumsum(sizes)[:-1]
    return [g.copy() for g in np.split(src, cuts)]


@pytest.mark.parametrize("many", [5, 17])
def test_singletons_equal_the_member_divergence(ctx, many):
    for ln in (1, T - 1, T, T + 1, 2 * T + 1):
        codes = kg.random_msa(np.random.default_rng(100 * many + ln), many, ln, pnil=0.05)
        want_d, want_c = guide.msa_divergence(ctx, codes)
        got_d, got_c = guide.msa_divergence_groups(ctx, codes, [[m] for m in range(many)])
        assert np.array_equal(got_c, want_c) and same_dist(got_d, want_d)
        assert np.array_equal(want_c, ktreelib.divergence(codes)[1])


@pytest.mark.parametrize("sizes", [(1, 2), (2, 1), (3, 5), (63, 65), (64, 64), (1, 130), (255, 3), (256, 2)], ids=str)
def test_two_groups_at_the_wave_and_workgroup_edges(ctx, sizes):
    """both group orders (which group is A decides the walk), lists ascending and reversed (the first member is special)"""
    many = sum(sizes)
    codes = kg.random_msa(np.random.default_rng(many), many, 2 * T + 3, pnil=0.03)
    ga, gb = split(sizes)
    for groups in ([ga, gb], [gb, ga], [ga[::-1].copy(), gb[::-1].copy()], [gb[::-1].copy(), ga]):
        check(ctx, codes, groups)
    if many <= 8:
        check(ctx, codes, [ga, gb], kg.group_counts_literal)


def test_first_member_gapped_or_not(ctx):
    """the same two groups with the gapped member first and last in its list: the counts differ, and both are the reference's"""
    rng = np.random.default_rng(3)
    codes = (2 + rng.integers(0, 3, (3 * T, 6))).astype(np.uint8)
    codes[2:T + 3, 0] = 1                                               # member 0 of A: a run over the first chunk border
    codes[T - 2:2 * T + 2, 3] = 1                                       # member 3 of B: a run over both borders
    seen = set()
    for ga in ([0, 1, 2], [2, 1, 0]):
        for gb in ([3, 4, 5], [5, 4, 3]):
            c = check(ctx, codes, [ga, gb], kg.group_counts_literal)
            seen.add(tuple(c[0]))
    assert len(seen) > 1


def test_gap_run_of_b_across_a_chunk_border_while_a_is_all_gaps(ctx):
    """h of the B member stays 0 over the border: A has no residue in the run's first columns"""
    rng = np.random.default_rng(4)
    codes = (2 + rng.integers(0, 3, (3 * T, 5))).astype(np.uint8)
    codes[T - 3:T + 5, 3] = 1                                           # B's second member: columns 5 .. 12
    codes[T - 3:T + 3, 0:2] = 1                                         # A all gaps in columns 5 .. 10
    codes[T + 1, 4] = 0                                                 # a nil code in B's last member
    c = check(ctx, codes, [[0, 1], [2, 3, 4]], kg.group_counts_literal)
    forgetful = np.zeros(4, np.int64)
    for c0 in range(0, 3 * T, T):
        forgetful += kg.group_counts_literal(codes[c0:c0 + T], [0, 1], [2, 3, 4])
    assert tuple(c[0]) != tuple(forgetful)                              # (a walk that forgot its counters at a border counts otherwise)
    check(ctx, codes, [[2, 3, 4], [0, 1]], kg.group_counts_literal)


def test_gap_run_of_a_across_chunk_borders(ctx):
    rng = np.random.default_rng(5)
    codes = (2 + rng.integers(0, 3, (3 * T + 1, 5))).astype(np.uint8)
    codes[3:2 * T + 4, 1] = 1                                           # A's second member over two borders
    codes[T - 1:T + 1, 0] = 1                                           # A's first member over the first
    codes[2 * T - 1:2 * T + 2, 2] = 1                                   # B's first member over the second
    for groups in ([[0, 1], [2, 3, 4]], [[1, 0], [4, 3, 2]], [[2, 3, 4], [0, 1]]):
        check(ctx, codes, groups, kg.group_counts_literal)


def test_all_gap_columns_at_chunk_edges_and_nil_codes(ctx):
    rng = np.random.default_rng(6)
    codes = (2 + rng.integers(0, 3, (3 * T, 6))).astype(np.uint8)
    codes[rng.random(codes.shape) < 0.25] = 1
    for col in (0, T - 1, T, 2 * T - 1, 2 * T, 3 * T - 1):
        codes[col] = 1 if col % 2 else 0                                # all gaps in both groups: gap codes, or nil codes
    codes[rng.random(codes.shape) < 0.05] = 0
    for groups in ([[0, 1, 2], [3, 4, 5]], [[5, 3], [0, 4], [2, 1]]):
        check(ctx, codes, groups, kg.group_counts_literal)
    codes[:] = 0                                                        # nothing but nil codes: every pair 0 / 0
    d, c = guide.msa_divergence_groups(ctx, codes, [[0, 1, 2], [3, 4, 5]])
    assert np.isnan(d).all() and not c.any()


def test_many_uneven_unsorted_groups(ctx):
    rng = np.random.default_rng(7)
    codes = kg.random_msa(rng, 300, 300, nres=5, pnil=0.02)
    groups = kg.random_groups(rng, 300, 40)
    assert len({len(g) for g in groups}) > 5 and any((np.diff(g) < 0).any() for g in groups)
    check(ctx, codes, groups)


@pytest.mark.parametrize("case", kg.fixtures(), ids=lambda f: f["name"])
def test_fixtures(ctx, case):
    """the counts and distances the REFERENCE's group pairdvn gave (tools/make_ktree_groups_golden.py)"""
    d, c = guide.msa_divergence_groups(ctx, case["codes"], case["groups"])
    assert np.array_equal(c, case["gcounts"]) and np.array_equal(bits(d), bits(case["gdist"]))


def test_refusals(ctx):
    ERR_ARG, L = -1, lib()
    codes = np.full((512, 4096), 2, np.uint8)
    halves = split((2048, 2048))
    with pytest.raises(Exception, match="groups 0 and 1"):              # 512 x 2048 x 2048 = 2^31
        guide.msa_divergence_groups(ctx, codes, halves)
    small = codes[:9, :6].copy()
    for groups in ([[0, 1, 2], [3, 4]], [[0, 1, 2], [2, 4, 5]], [[0, 1, 2], [3, 4, 6]], [[0, 1, 2, 3, 4, 5]], [[0, 1, 2, 3, 4, 5], []]):
        with pytest.raises(Exception):
            guide.msa_divergence_groups(ctx, small, groups)
        assert "g2g_msa_divergence_groups" in last_error()
    ss, keep = guide._subset_struct([[0, 1, 2], [3, 4, 5]])
    d = np.zeros(4, np.float64)
    p, dp = small.ctypes.data_as(_abi.c_u8p), d.ctypes.data_as(_abi.c_f64p)
    assert L.g2g_msa_divergence_groups(ctx._h, 6, 9, p, C.byref(ss), None, None) == ERR_ARG
    assert L.g2g_msa_divergence_groups(ctx._h, 6, 9, None, C.byref(ss), dp, None) == ERR_ARG
    assert L.g2g_msa_divergence_groups(ctx._h, 6, 9, p, None, dp, None) == ERR_ARG
    assert L.g2g_msa_divergence_groups(ctx._h, 6, 0, p, C.byref(ss), dp, None) == ERR_ARG
    assert L.g2g_msa_divergence_groups(ctx._h, 6, 9, p, C.byref(ss), dp, None) == 0      # (counts may be NULL)
