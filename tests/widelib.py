"""Hand-made "staircase" groups and the wide, gap-rich cases built from them (tests/golden/wide/*.npz, written by
tools/make_golden.py job_wide from the real reference; tests/test_gpu_wide.py runs them on the GPU).

A staircase side has `plain` members without a gap and K members with one gap run each, of 1 .. K columns, all ending just
before column c0.  With at least one plain member that gives hetero = K + 1, a t list of j entries in row c0 - K - 1 + j (the
longest, K, in row c0 - 1) and an s list (row c0) and an r list (row c0 - 1) of K + 1 entries; capa = hetero + 1 = K + 2.

The K of the cases sit on both sides of the constants the engine keys its capacity rules on, as those stand:
  K = 61 / 62    the lanes walker of calcSpScore gives a list of 63 entries back to the scalar walker (`L.cnt >= 63`, `p >= 63`
                 in g2g_kernels.hip): longest list 62 stays on the lanes, 63 is handed over
  K = 64 / 65    g2g_build_gfq_kernel holds one gap class per lane (`nt > 64` is overflow): 64 classes alive in row c0 - 1 are
                 built on the device, 65 on the host
  K = 189 / 190  the running lists of calcSpScore stay in LDS while capa + 1 <= SP_FAST_LIST (192): K + 3 = 192 / 193
  K = 70 x 66    both sides wide: v2_lds_bytes exceeds V2_LDS_MAX at 256 threads, a `_pf` DP that v6 and v2 cannot take falls to
                 g2g_forward_kernel (generation 0) by default
  hf65 / hf20    `_hf` (b one sequence) with lists beyond the 16 register slots of v3r: v2 or v3-LDS by LDS budget; K = 20 is
                 small enough for v3-LDS under a third of V2_LDS_MAX with Noll 2
  m257 / m300    more than 256 members (the builder reads codes in place, `pre == false`) with 40 classes: the gapped members
                 sit at indices on both sides of 63 | 64 and 255 | 256 and at the last index
Every case exists with Noll 2 and Noll 3 (ls = 3); `_w` twins carry member weights."""
import glob
import os

import numpy as np

AA = "ACDEFGHIKLMNPQRSTVWY"
WIDE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide")


def base(seed, n):
    rng = np.random.default_rng(seed)
    return "".join(AA[i] for i in rng.integers(20, size=n))


def member(rng, base, gap_end=0, gap_len=0):
    r = [AA[rng.integers(20)] if rng.random() < 0.2 else c for c in base]
    for i in range(gap_end - gap_len, gap_end):
        r[i] = "-"
    return "".join(r)


def stair(K, c0, base, plain=2, seed=100):
    """`plain` members without a gap, then K members with gap runs of 1 .. K columns that end just before column c0"""
    rng = np.random.default_rng(seed + K)
    return [member(rng, base) for _ in range(plain)] + [member(rng, base, c0, g) for g in range(1, K + 1)]


def stair_at(many, at, c0, base, seed=300):
    """`many` members; the j-th index of `at` (ascending) carries a gap run of j + 1 columns that ends just before column c0"""
    rng = np.random.default_rng(seed + many)
    run = {i: j + 1 for j, i in enumerate(sorted(at))}
    return [member(rng, base, c0, run.get(i, 0)) for i in range(many)]


def list_lengths(side):
    """entries (terminator not counted) of the s, t, r lists of rows -1 .. len - 1 of a g2g_side: [view][row + 1]"""
    return [np.diff(np.ctypeslib.as_array(side.gfq.off[v], shape=(side.len + 2,))) - 1 for v in range(3)]


def fixture_list_lengths(d, pfx):
    """the same from a fixture's arrays"""
    return [np.diff(d[pfx + v + "_off"]) - 1 for v in ("sfq", "tfq", "rfq")]


def check_stair(s, t, r, hetero, K, c0, n):
    """the list lengths a staircase side of n columns with plain members must have"""
    want_t = np.zeros(n, int)
    want_t[c0 - K:c0] = np.arange(1, K + 1)
    assert np.array_equal(t[1:], want_t), t
    assert s[1 + c0] == K + 1 and s.max() == K + 1 and (np.delete(s, 1 + c0) <= 1).all(), s
    assert r[c0] == K + 1 and r.max() == K + 1, r
    assert hetero == K + 1


_M257 = list(range(54, 74)) + list(range(237, 257))                  # 63 | 64, 255 | 256 = the last index
_M300 = list(range(54, 74)) + list(range(246, 265)) + [299]          # 63 | 64, 255 | 256, the last index
# name: (a: K, columns, members or None, gapped indices or None), (b: K, columns; K = 0: one sequence), alnmode
CASES = {
    "K61": ((61, 150, None, None), (3, 140), 9),
    "K62": ((62, 150, None, None), (3, 140), 9),
    "K64": ((64, 150, None, None), (3, 140), 9),
    "K65": ((65, 150, None, None), (3, 140), 9),
    "K189": ((189, 260, None, None), (3, 250), 9),
    "K190": ((190, 260, None, None), (3, 250), 9),
    "K70xK66": ((70, 160, None, None), (66, 150), 9),
    "hf65": ((65, 150, None, None), (0, 140), 7),
    "hf20": ((20, 150, None, None), (0, 140), 7),
    "m257": ((40, 150, 257, _M257), (3, 140), 9),
    "m300": ((40, 150, 300, _M300), (3, 140), 9),
}
WEIGHTED = ("K62", "K65", "K190", "K70xK66")
C0_A, C0_B = 10, 20                                                  # c0 = columns - 10 on a, columns - 20 on b


def names():
    """every fixture of the job: case_noll{2,3}[_w]"""
    out = []
    for c in CASES:
        for noll in (2, 3):
            out.append("%s_noll%d" % (c, noll))
            if c in WEIGHTED:
                out.append("%s_noll%d_w" % (c, noll))
    return out


def case_of(name):
    return name.split("_noll")[0]


def rows(case):
    """the aligned members of the two groups of a case; b is cut from a's base sequence five columns in, so the best path runs
    down the rows of the long lists"""
    (Ka, la, many, at), (Kb, lb), _ = CASES[case]
    ba = base(5, la)
    bb = ba[5:5 + lb]
    ra = stair(Ka, la - C0_A, ba) if many is None else stair_at(many, at, la - C0_A, ba)
    rb = [member(np.random.default_rng(7), bb)] if Kb == 0 else stair(Kb, lb - C0_B, bb, plain=2 if Kb > 3 else 1, seed=7)
    return ra, rb


def weights(case):
    ra, rb = rows(case)
    rng = np.random.default_rng(11)
    return rng.uniform(0.2, 1.0, len(ra)), rng.uniform(0.2, 1.0, len(rb))


def check_fixture(name, d):
    """the edge a case was made for is still in the problem the reference built from it"""
    case = case_of(name)
    (Ka, la, many, at), (Kb, lb), mode = CASES[case]
    assert d["alnmode"][0] == mode and not d["swp"][0], (name, d["alnmode"][0], d["swp"][0])
    assert d["Noll"][0] == (3 if "_noll3" in name else 2)
    assert ("a_weight" in d) == name.endswith("_w")
    assert (d["a_len"][0], d["b_len"][0]) == (la, lb) and (d["a_left"][0], d["a_right"][0]) == (0, la)
    assert d["a_many"][0] == (Ka + 2 if many is None else many)
    if at is not None:
        col = d["a_seq"][la - C0_A]                                  # (position -1 first: the last column of the gap runs)
        assert np.array_equal(np.flatnonzero(col == 1), sorted(at)) and len(at) == Ka
    s, t, r = fixture_list_lengths(d, "a_")
    check_stair(s, t, r, d["a_hetero"][0], Ka, la - C0_A, la)
    if Kb:
        s, t, r = fixture_list_lengths(d, "b_")
        check_stair(s, t, r, d["b_hetero"][0], Kb, lb - C0_B, lb)
    else:
        assert d["b_many"][0] == 1


def load():
    """[(name, fixture)] of tests/golden/wide, every case of names() present"""
    paths = sorted(glob.glob(os.path.join(WIDE_DIR, "*.npz")))
    got = [os.path.basename(p)[:-4] for p in paths]
    assert got == sorted(names()), (got, names())
    return [(n, dict(np.load(p))) for n, p in zip(got, paths)]
