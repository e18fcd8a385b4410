"""Test-side helpers of the progressive alignment (g2g_progressive): the loader of the reference's per-merge fixtures
(tests/golden/progressive/*.npz, written by tools/make_progressive_golden.py), a plain Python restatement of one merge -- apply a
skeleton, order the members --, and an aligner callback that puts the CPU CHECKER (oracle/) in the seat of g2g_align2_batch so that
the C++ driver -- tree validation, waves, the swapped member order, clean-up -- runs on a machine without a GPU.  Tests only: the
product never sets an aligner."""
from __future__ import annotations

import ctypes as C
import os
from types import SimpleNamespace

import numpy as np

import oraclelib
from prrn_aln_amd import _abi
from prrn_aln_amd import operator as op
from prrn_aln_amd._lib import lib

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "progressive")
GAP = 1
MODE_NAME = {6: "NGP_ALB", 7: "HLF_ALB", 8: "RHF_ALB", 9: "GPF_ALB", 10: "NTV_ALB"}
G2G_ERR_ENDS = -6


def names():
    return sorted(n[:-4] for n in os.listdir(GOLD) if n.endswith(".npz")) if os.path.isdir(GOLD) else []


def load(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


def seqs_of(g):
    at = np.concatenate([[0], np.cumsum(g["lens"])])
    return [np.ascontiguousarray(g["codes"][at[i]:at[i + 1]]) for i in range(len(g["lens"]))]


def tree_of(g):
    return SimpleNamespace(left=g["tree_left"], right=g["tree_right"], parent=g["tree_parent"])


def alp_of(g):
    molc = int(g["molc"][0])
    return op.AlnParam(u=float(g["u"][0]), v=float(g["v"][0]), u1=float(g["u1"][0]), k1=int(g["k1"][0]), ls=int(g["ls"][0]),
                       sh=int(g["sh"][0]), scale=float(g["scale"][0]), tgapf=float(g["tgapf"][0]), molc=molc, simmtx=g["simmtx"],
                       max_code=25 if molc == 1 else 17)


def prm_of(g):
    """the fixture's parameters as a g2g_params that owns what it points to"""
    prm, sm = alp_of(g).to_c()
    prm._keep = sm
    return prm


def node_records(g):
    """the reference's merges of a fixture: {node: dict(len, scr, swp, mode, na, nb, order, codes (len, members), skl (n, 2))}"""
    out = {}
    for i, k in enumerate(g["node"].tolist()):
        o0, o1 = g["node_order_off"][i:i + 2]
        c0, c1 = g["node_codes_off"][i:i + 2]
        s0, s1 = g["node_skl_off"][i:i + 2]
        members = int(o1 - o0)
        out[k] = dict(len=int(g["node_len"][i]), scr=float(g["node_scr"][i]), swp=int(g["node_swp"][i]), mode=int(g["node_mode"][i]),
                      na=int(g["node_na"][i]), nb=int(g["node_nb"][i]), order=g["node_order"][o0:o1],
                      codes=g["node_codes"][c0:c1].reshape(-1, members), skl=g["node_skl"][s0:s1].reshape(-1, 2))
    return out


# ---- one merge, restated -----------------------------------------------------------------------------------------------------------
def apply_skeleton(a, b, skl):
    """syntheseq (reference src/maln2.cc:2027-2046) on blocks of codes [column][member]: the columns of a and b interleaved as the
    corners of the skeleton say, a's members first"""
    a = np.asarray(a, np.uint8).reshape(len(a), -1)
    b = np.asarray(b, np.uint8).reshape(len(b), -1)
    skl = np.asarray(skl).reshape(-1, 2)
    assert tuple(skl[0]) == (0, 0) and tuple(skl[-1]) == (len(a), len(b))
    rows = []
    for (m0, n0), (m1, n1) in zip(skl[:-1].tolist(), skl[1:].tolist()):
        dm, dn = m1 - m0, n1 - n0
        assert dm >= 0 and dn >= 0 and (dm == dn or dm == 0 or dn == 0)
        for t in range(max(dm, dn)):
            ra = a[m0 + t] if dm else np.full(a.shape[1], GAP, np.uint8)
            rb = b[n0 + t] if dn else np.full(b.shape[1], GAP, np.uint8)
            rows.append(np.concatenate([ra, rb]))
    return np.array(rows, np.uint8).reshape(len(rows), a.shape[1] + b.shape[1])


def merge(left, right, swp, skl):
    """(codes, order) of a father from its sons' (codes, order): the PwdM's a side -- the right son when it swapped -- comes first"""
    (ca, oa), (cb, ob) = (right, left) if swp else (left, right)
    return apply_skeleton(ca, cb, skl), np.concatenate([oa, ob]).astype(np.int32)


def degap(col):
    return np.asarray(col)[np.asarray(col) > GAP]


# ---- the CPU checker in the aligner's seat ---------------------------------------------------------------------------------------
def _stripe(prob, sh):
    """stripe() (reference src/aln2.cc:156-174) of a problem's two sides"""
    a, b = prob.a, prob.b
    if sh < 0:
        sh = -sh * min(a.right - a.left, b.right - b.left) // 100
    u, l = b.right - a.right, b.left - a.left
    if u < l:
        u, l = l, u
    u += sh; l -= sh
    return max(l, b.left - a.right), min(u, b.right - a.left)


def oracle_aligner(fail_at: int = -1, calls=None, batches=None):
    """An _abi.ALIGN_FN: align2() of every PwdM of a wave by the CPU checker -- forwardB + traceback + stdskl, the end check, and on
    a mismatch the band reopened to sh = -100 and the DP repeated (reference src/maln2.cc:1946-1952).  calls: a one-element list
    that counts the calls; batches: a list that receives every call's size.  fail_at >= 0: the call with that index (0-based)
    returns 7 instead."""
    OL = oraclelib.load()
    L = lib()
    calls = calls if calls is not None else [0]

    def cb(user, n, pw, scr, skl, nskl, status):
        k = calls[0]
        calls[0] += 1
        if batches is not None:
            batches.append(n)
        if fail_at >= 0 and k == fail_at:
            return 7
        try:
            for i in range(n):
                prob = L.g2g_pwdm_problem(pw[i])
                status[i] = 0
                for attempt in range(2):
                    res = _abi.Result()
                    if OL.g2g_oracle_forward(prob, C.byref(res)) != 0:
                        return 3
                    nout = C.c_int(0)
                    s = OL.g2g_oracle_stdskl(res.trace, res.ntrace, C.byref(nout))      # malloc'ed: handed to the library, which frees it
                    OL.g2g_oracle_free(res.trace)
                    a, b = prob.contents.a, prob.contents.b
                    m = nout.value
                    if m >= 1 and (s[0].m, s[0].n, s[m - 1].m, s[m - 1].n) == (a.left, b.left, a.right, b.right):
                        scr[i] = res.score
                        skl[i] = s
                        nskl[i] = m
                        break
                    OL.g2g_oracle_free(s)
                    if attempt == 0:
                        prob.contents.lw, prob.contents.up = _stripe(prob.contents, -100)
                    else:
                        status[i] = G2G_ERR_ENDS
            return 0
        except Exception:
            return 9
    return _abi.ALIGN_FN(cb)


# ---- what every run is held to ---------------------------------------------------------------------------------------------------
def check_against_fixture(g, codes, order, merges):
    """g2g_progressive's outputs against the reference's merges: per inner node a bit-equal DP score, equal swp, mode, member
    counts of the PwdM's sides and merged length; the member order and the merged codes of EVERY node, rebuilt from the leaves with
    the recorded skeletons and the swp the library reported; the final MSA and order"""
    ref = node_records(g)
    seqs = seqs_of(g)
    n = len(seqs)
    assert sorted(m["node"] for m in merges) == sorted(ref)
    done = {i: (seqs[i].reshape(-1, 1), np.array([i], np.int32)) for i in range(n)}
    for m in merges:
        r = ref[m["node"]]
        assert (m["left"], m["right"]) == (int(g["tree_left"][m["node"]]), int(g["tree_right"][m["node"]]))
        assert np.float64(m["scr"]).view(np.uint64) == np.float64(r["scr"]).view(np.uint64), (m["node"], m["scr"], r["scr"])
        assert (m["swp"], m["mode"], m["na"], m["nb"], m["len"]) == (r["swp"], r["mode"], r["na"], r["nb"], r["len"]), (m, r["swp"], r["mode"])
        c, o = merge(done[m["left"]], done[m["right"]], m["swp"], r["skl"])
        assert np.array_equal(o, r["order"]), m["node"]
        assert np.array_equal(c, r["codes"]), m["node"]
        done[m["node"]] = (c, o)
    root = int(np.flatnonzero(g["tree_parent"] < 0)[0])
    assert np.array_equal(order, done[root][1])
    assert np.array_equal(codes, done[root][0])
    for k in range(n):
        assert np.array_equal(degap(codes[:, k]), seqs[order[k]])
    # ... and read off the library's own result: later merges only add gaps to a block, so the members of a node stand together
    # in the final MSA, in the node's order, and their columns without the all-gap ones are the node's merged block
    for k, r in ref.items():
        inside = np.isin(order, r["order"])
        at = np.flatnonzero(inside)
        assert at[-1] - at[0] + 1 == len(at) and np.array_equal(order[at], r["order"]), k
        sub = codes[:, at]
        assert np.array_equal(sub[(sub > GAP).any(axis=1)], r["codes"]), k
