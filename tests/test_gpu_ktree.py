"""The weighting tree from an MSA on the GPU: g2g_msa_divergence (g2g_msa_div_kernel: one workgroup per 16 x 16 tile of pairs,
columns in chunks of 256 staged in LDS, counters carried in registers) against the Python restatement of pairdvn
(tests/ktreelib.py) -- counts equal, distances bit-equal -- and g2g_ktree_from_msa against the trees the REFERENCE built for the
26 (MSA, tree) pairs of the fixtures: same topology, vol / cur bit-equal.  Then the last link: a refinement that gets its tree
from KTree.from_msa walks the reference's trajectory."""
import ctypes as C

import numpy as np
import pytest

import ktreelib
import refinelib
from ktreelib import bits
from prrn_aln_amd import _abi, engine, guide
from prrn_aln_amd._lib import lib
from prrn_aln_amd.refine import KTree, refine_native

pytestmark = pytest.mark.gpu
PAIRS = ktreelib.pairs()
IDS = [p[0] for p in PAIRS]
# every chunk border of the kernel (KT_CHUNK = 256: 255 / 256 / 257, two chunks + 1, a ragged fourth chunk) and the 16-column
# groups inside a chunk (63 / 64 / 65)
LENS = (1, 2, 63, 64, 65, 255, 256, 257, 513, 1000)


@pytest.fixture(scope="module")
def ctx():
    c = engine.Context()
    yield c
    c.close()


def gapped_msa(many, ln, seed):
    """random residues over a small alphabet (so that matches occur), a third of the cells gaps, some nil codes (0 counts as a
    gap), and -- from 513 columns on -- gap runs of 300 columns that cross the chunk borders at 256 and 512 in member 0 alone
    (100 .. 250), in members 0 and 1 at once (250 .. 400), in member 1 alone (400 .. 550), and in the last member (200 .. 500)"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(2, 7, (ln, many)).astype(np.uint8)
    codes[rng.random((ln, many)) < 0.3] = 1
    codes[rng.random((ln, many)) < 0.04] = 0
    if ln > 2:
        codes[rng.integers(0, ln)] = 0                                  # a whole column of nil codes
    if ln >= 513:
        codes[100:400, 0] = 1
        codes[250:550, 1] = 1
        codes[200:500, many - 1] = 1
    return codes


def check_divergence(ctx, codes):
    want_d, want_c = ktreelib.divergence(codes)
    got_d, got_c = guide.msa_divergence(ctx, codes)
    assert np.array_equal(got_c, want_c)
    nan = np.isnan(want_d)                                              # (a pair without a residue / residue or unpaired column: 0 / 0)
    assert np.array_equal(np.isnan(got_d), nan) and np.array_equal(bits(got_d[~nan]), bits(want_d[~nan]))
    return got_d, got_c


@pytest.mark.parametrize("many", [2, 3, 16, 17, 33])
def test_divergence_equals_the_restatement(ctx, many):
    """2 / 3: one diagonal tile, nearly all lanes masked; 16: exactly one tile; 17 / 33: partial tiles off the diagonal"""
    for ln in LENS:
        _, cnt = check_divergence(ctx, gapped_msa(many, ln, 1000 * many + ln))
        assert (cnt[:, :3].sum(1) <= ln).all() and (ln < 63 or (cnt[:, :3].sum(1) > 0).all())


def test_long_gap_runs_cross_chunk_borders(ctx):
    """what the 300-column runs are there for: in the pairs of members 0 and 1 gaps are opened and NOT opened depending on run
    lengths counted across chunk borders -- the restatement's counts differ from a walk that forgets gsi / gsj at a border"""
    codes = gapped_msa(5, 1000, 77)
    _, cnt = check_divergence(ctx, codes)
    forgetful = np.zeros(4, np.int64)
    for c0 in range(0, 1000, 256):
        forgetful += ktreelib.pairdvn_counts(codes[c0:c0 + 256, 0], codes[c0:c0 + 256, 1])
    assert tuple(cnt[ktreelib.elem(0, 1)]) == ktreelib.pairdvn_counts(codes[:, 0], codes[:, 1]) != tuple(forgetful)


def test_all_gap_members(ctx):
    codes = gapped_msa(4, 300, 9)
    codes[:, 0] = 1                                                     # all gaps
    codes[:, 1] = np.where(np.arange(300) % 3 == 0, 0, 1)               # all gaps, nil codes among them
    want_d, want_c = ktreelib.divergence(codes)
    got_d, got_c = guide.msa_divergence(ctx, codes)
    assert np.array_equal(got_c, want_c)
    nan = np.isnan(want_d)
    assert nan[ktreelib.elem(0, 1)] and nan.sum() == 1 and np.array_equal(np.isnan(got_d), nan)      # gap / gap pair: 0 / 0 on both sides
    assert np.array_equal(bits(got_d[~nan]), bits(want_d[~nan]))
    assert got_d[ktreelib.elem(0, 2)] == 1. and tuple(got_c[ktreelib.elem(0, 1)]) == (0, 0, 0, 0)
    with pytest.raises(Exception):                                      # ... and no tree can be built on a NaN
        KTree.from_msa(ctx, codes)


@pytest.mark.parametrize("idx", range(len(PAIRS)), ids=IDS)
def test_from_msa_reproduces_the_reference_tree(ctx, idx):
    _, codes, ref = PAIRS[idx]
    t = KTree.from_msa(ctx, codes)
    assert (t.left, t.right, t.parent) == (ref["left"], ref["right"], ref["parent"])
    assert np.array_equal(bits(t.vol), bits(ref["vol"])) and np.array_equal(bits(t.cur), bits(ref["cur"]))
    assert t.root == len(t.left) - 1 and t.ndesc[t.root] == codes.shape[1]


def test_refinement_on_the_tree_from_msa(ctx):
    """unaligned-to-refined without a tree from outside: KTree.from_msa on the start MSA, then g2g_refine with it"""
    path = [p for p in refinelib.fixtures() if "prot12x80_s3" in p][0]
    f, _, alp, start = refinelib.load(path)
    tree = KTree.from_msa(ctx, start)
    final, steps, stats = refine_native(ctx, start, tree, alp, seed=1, maxitr=10, window=16, want_moves=True)
    refinelib.check_against_trace(f, final, steps, stats)
    assert len(steps) == 51 and stats["accepted"] == len(f["accepted"])


def test_bad_arguments(ctx):
    ERR_ARG = -1
    L = lib()
    buf = np.ones(64, np.uint8)                                         # (refused before anything is read or written)
    d = np.zeros(64, np.float64)
    p, dp = buf.ctypes.data_as(_abi.c_u8p), d.ctypes.data_as(_abi.c_f64p)
    T = _abi.KTreeOut()
    for many, ln in ((1, 5), (4097, 2), (3, 0), (0, 5), (3, -1)):
        assert L.g2g_msa_divergence(ctx._h, many, ln, p, dp, None) == ERR_ARG
        assert L.g2g_ktree_from_msa(ctx._h, many, ln, p, C.byref(T)) == ERR_ARG
    assert L.g2g_msa_divergence(ctx._h, 3, 5, None, dp, None) == ERR_ARG
    assert L.g2g_msa_divergence(ctx._h, 3, 5, p, None, None) == ERR_ARG
    assert L.g2g_ktree_from_msa(ctx._h, 3, 5, p, None) == ERR_ARG
