"""Python glue over g2g_refine / g2g_pairsum (include/g2g.h): prrn's randomised iterative
refinement (Prrn::rir, reference src/prrn5.cc:633-666) runs in C++ behind the C ABI (csrc/g2g_refine.cpp); this module only
marshals the MSA, the weighting tree and the options, and offers an exchange callback on torch.distributed for runs sharded
over ranks.  Nothing here computes."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _abi
from . import operator as op
from ._lib import G2GError, last_error, lib


@dataclass
class KTree:
    """The weighting tree as the reference's Ktree::lead[] holds it: node id = tid (leaves 0..n-1 = members), -1 where a link is
    absent, vol / cur = the Kirchhoff weights of Ktree::calcpw.  from_msa / from_dist build it in the library (g2g_ktree_from_msa /
    g2g_ktree_from_dist: the reference's tree, bit for bit) and fill height / length / res / ndesc / root as well; a tree from
    elsewhere is given by its first five arrays."""
    left: List[int]
    right: List[int]
    parent: List[int]
    vol: List[float]
    cur: List[float]
    height: Optional[List[float]] = None
    length: Optional[List[float]] = None
    res: Optional[List[float]] = None
    ndesc: Optional[List[int]] = None
    root: Optional[int] = None

    @property
    def n_leaves(self) -> int:
        return (len(self.left) + 1) // 2

    @classmethod
    def _take(cls, T: "_abi.KTreeOut") -> "KTree":
        """copy a g2g_ktree out of the library's arrays and release them"""
        n = T.n_nodes
        get = lambda p: np.ctypeslib.as_array(p, shape=(n,)).tolist()
        t = cls(get(T.left), get(T.right), get(T.parent), get(T.vol), get(T.cur), get(T.height), get(T.length), get(T.res),
                get(T.ndesc), int(T.root))
        lib().g2g_ktree_free(C.byref(T))
        return t

    @classmethod
    def from_dist(cls, dist, with_weights: bool = True, leaves=None) -> "KTree":
        """g2g_ktree_from_dist: UPGMA tree (DistTree::upg_method) of a condensed distance vector -- pair (i < j) at j (j - 1) / 2 + i --
        and, with_weights, the Kirchhoff weights (Ktree::calcpw); host only.  Without them vol / cur are zero.
        leaves = (ndesc, height, res), each an array of one value per leaf or None: g2g_ktree_from_dist_leaves, leaves that are
        sub-alignments (what IterMsa::phyl_pwt puts into lead[k])."""
        d = np.ascontiguousarray(dist, np.float64).reshape(-1)
        many = int(round((1 + (1 + 8 * len(d)) ** 0.5) / 2))
        if many * (many - 1) // 2 != len(d):
            raise ValueError("%d distances are not the pairs of a whole number of members" % len(d))
        T = _abi.KTreeOut()
        if leaves is None:
            rc = lib().g2g_ktree_from_dist(many, d.ctypes.data_as(_abi.c_f64p), 1 if with_weights else 0, C.byref(T))
            if rc != 0:
                raise G2GError("g2g_ktree_from_dist rc=%d: %s" % (rc, last_error()))
            return cls._take(T)
        ndesc, height, res = leaves
        nd = None if ndesc is None else np.ascontiguousarray(ndesc, np.int32)
        hg = None if height is None else np.ascontiguousarray(height, np.float64)
        rs = None if res is None else np.ascontiguousarray(res, np.float64)
        if any(a is not None and a.shape != (many,) for a in (nd, hg, rs)):
            raise ValueError("one ndesc / height / res per leaf")
        ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
        rc = lib().g2g_ktree_from_dist_leaves(many, d.ctypes.data_as(_abi.c_f64p), ptr(nd, C.POINTER(C.c_int32)), ptr(hg, _abi.c_f64p),
                                              ptr(rs, _abi.c_f64p), 1 if with_weights else 0, C.byref(T))
        if rc != 0:
            raise G2GError("g2g_ktree_from_dist_leaves rc=%d: %s" % (rc, last_error()))
        return cls._take(T)

    @classmethod
    def from_msa_groups(cls, ctx, codes: np.ndarray, groups, flat_leaves: bool = False):
        """g2g_ktree_from_msa_groups: IterMsa::phyl_pwt over groups the caller brings -- (the weighting tree over the groups, the
        members' weights).  The tree's leaves are the groups; it is the tree guide.fuse_groups / conserved_regions_groups take
        with `groups`."""
        from .guide import _subset_struct
        codes = np.ascontiguousarray(codes, np.uint8)
        ln, many = codes.shape
        ss, keep = _subset_struct(groups)
        T = _abi.KTreeOut()
        weight = np.zeros(many, np.float64)
        sumwt = C.c_double(0.)
        rc = lib().g2g_ktree_from_msa_groups(None if ctx is None else ctx._h, many, ln, codes.ctypes.data_as(_abi.c_u8p), C.byref(ss),
                                             1 if flat_leaves else 0, C.byref(T), weight.ctypes.data_as(_abi.c_f64p), C.byref(sumwt))
        del keep
        if rc != 0:
            raise G2GError("g2g_ktree_from_msa_groups rc=%d: %s" % (rc, last_error()))
        return cls._take(T), weight

    @classmethod
    def from_msa(cls, ctx, codes: np.ndarray) -> "KTree":
        """g2g_ktree_from_msa: the weighting tree of an MSA ((len, many) uint8 codes), divergences on the GPU"""
        codes = np.ascontiguousarray(codes, np.uint8)
        ln, many = codes.shape
        T = _abi.KTreeOut()
        rc = lib().g2g_ktree_from_msa(ctx._h, many, ln, codes.ctypes.data_as(_abi.c_u8p), C.byref(T))
        if rc != 0:
            raise G2GError("g2g_ktree_from_msa rc=%d: %s" % (rc, last_error()))
        return cls._take(T)

    def to_c(self):
        """(g2g_tree, arrays to keep alive)"""
        arr = lambda x, t: np.ascontiguousarray(x, t)
        keep = (arr(self.left, np.int32), arr(self.right, np.int32), arr(self.parent, np.int32), arr(self.vol, np.float64), arr(self.cur, np.float64))
        T = _abi.Tree()
        T.n_nodes = len(keep[0])
        i32p = C.POINTER(C.c_int32)
        T.left, T.right, T.parent = (k.ctypes.data_as(i32p) for k in keep[:3])
        T.vol, T.cur = keep[3].ctypes.data_as(_abi.c_f64p), keep[4].ctypes.data_as(_abi.c_f64p)
        return T, keep


def torch_exchange(device=None):
    """An exchange callback for g2g_refine on torch.distributed (RCCL when `device` is a GPU, gloo on the CPU): all-gathers the
    ranks' buffers.  Returns (callback object to keep alive, rank, world).  A rank whose part of a window failed still calls it
    (its error code travels in its buffer, g2g.h), so the collective is entered by every rank in every window."""
    import torch
    import torch.distributed as dist
    rank, world = dist.get_rank(), dist.get_world_size()

    def cb(user, mine, n_ints, out):
        try:
            t = torch.from_numpy(np.ctypeslib.as_array(mine, shape=(n_ints,)).copy())
            if device is not None:
                t = t.to(device)
            parts = [torch.empty_like(t) for _ in range(world)]
            dist.all_gather(parts, t)
            dst = np.ctypeslib.as_array(out, shape=(world * n_ints,))
            for r, part in enumerate(parts):
                dst[r * n_ints:(r + 1) * n_ints] = part.cpu().numpy()
            return 0
        except Exception:
            return 1
    return _abi.EXCHANGE_FN(cb), rank, world


def _refine_opts(seed: int = 1, maxitr: int = 10, window: int = 32, exchange=None, scorer=None, window_min: int = 0,
                 want_moves: bool = False, slot_cap: int = 0):
    """(g2g_refine_opts, the accepted moves' list or None, objects to keep alive)"""
    O = _abi.RefineOpts()
    O.seed, O.maxitr, O.window, O.window_min, O.slot_cap = seed, maxitr, window, window_min, slot_cap
    if exchange is not None:
        O.exchange, O.rank, O.world = exchange
    if scorer is not None:
        O.scorer = scorer
    moves, acb = None, None
    if want_moves:
        moves = []

        def on_accept(user, branch, na, la, nb, lb, nskl, skl):
            moves.append((branch, [la[i] for i in range(na)], [lb[i] for i in range(nb)],
                          np.array([(skl[i].m, skl[i].n) for i in range(nskl)], np.int32).reshape(-1, 2)))
        acb = _abi.ACCEPT_FN(on_accept)
        O.on_accept = acb
    return O, moves, acb


def _take_results(many, out, olen, steps, ns, st, moves):
    """(final MSA, step dicts, stats dict) out of the library's arrays, which are released"""
    L = lib()
    final = np.ctypeslib.as_array(out, shape=(olen.value * many,)).reshape(olen.value, many).copy()
    L.g2g_free(out)
    log = [dict(branch=s.branch, na=s.na, nb=s.nb, swp=bool(s.swp), accepted=bool(s.accepted), skipped=bool(s.skipped), scr=s.scr,
                val_new=s.val_new, val_old=s.val_old, delta=s.delta, t_ms=s.t_ms) for s in (steps[i] for i in range(ns.value))]
    L.g2g_free(steps)
    stats = {k: getattr(st, k) for k, _ in _abi.RefineStats._fields_ if k != "reserved"}
    if moves is not None:
        stats["moves"] = moves
    return final, log, stats


def refine_native(ctx, codes: np.ndarray, tree: KTree, alp: op.AlnParam, seed: int = 1, maxitr: int = 10, window: int = 32,
                  exchange=None, scorer=None, window_min: int = 0, want_moves: bool = False, slot_cap: int = 0):
    """g2g_refine: (refined MSA (len, many) uint8, [step dicts], stats dict).  `exchange`: the triple torch_exchange returns, for
    a run sharded over ranks.  `scorer`: an _abi.SCORE_FN standing in for the GPU (tests; ctx may then be None).  With
    want_moves every accepted move is recorded as stats["moves"] = [(branch, la, lb, skl (n, 2))]."""
    codes = np.ascontiguousarray(codes, np.uint8)
    ln, many = codes.shape
    prm, _sm = alp.to_c()
    T, _keep = tree.to_c()
    O, moves, _acb = _refine_opts(seed, maxitr, window, exchange, scorer, window_min, want_moves, slot_cap)
    out = _abi.c_u8p(); olen = C.c_int(); steps = C.POINTER(_abi.RefineStep)(); ns = C.c_int(); st = _abi.RefineStats()
    rc = lib().g2g_refine(ctx._h if ctx is not None else None, C.byref(prm), many, ln, codes.ctypes.data_as(_abi.c_u8p), C.byref(T), C.byref(O),
                          C.byref(out), C.byref(olen), C.byref(steps), C.byref(ns), C.byref(st))
    if rc != 0:
        raise G2GError("g2g_refine rc=%d: %s" % (rc, last_error()))
    return _take_results(many, out, olen, steps, ns, st, moves)


def refine_planned(ctx, codes: np.ndarray, tree, prm: "_abi.Params", thr: float = 35., weight=None, plan=None, plan_prm=None, groups=None, **opts):
    """g2g_refine_planned: prrn's default refinement -- fused groups move as blocks, only the unconserved column ranges are refined,
    from the last to the first.  prm: the parameters of the DPs (the alignment's).  plan: what guide.refine_plan returned (or a
    guide.RefinePlan made by hand).  plan None: with plan_prm the plan is made here first by guide.refine_plan(ctx, ..., plan_prm,
    thr, weight) -- the reference decides it with parameters of its own (its localprm and similarity matrix number 1), not the
    alignment's; without plan_prm the library makes it with prm itself.  Either way a context is needed.  weight as for
    guide.refine_plan; opts as for refine_native.  groups: g2g_refine_planned_groups -- tree is the tree over these groups, which
    are refined against each other and stay as they are inside.  Returns (refined MSA (len, many) uint8, [step dicts] of the ranges
    in processing order, [range dicts] in the plan's order, stats dict)."""
    from . import guide
    if plan is None and plan_prm is not None:
        plan = guide.refine_plan(ctx, codes, tree, plan_prm, thr, weight, groups=groups)
    codes, w = guide._msa_args(codes, weight)
    ln, many = codes.shape
    T, _keep = guide._tree_struct(tree)
    P, _keep_p = guide.plan_struct(plan) if plan is not None else (None, None)
    O, moves, _acb = _refine_opts(**opts)
    out = _abi.c_u8p(); olen = C.c_int(); steps = C.POINTER(_abi.RefineStep)(); ns = C.c_int(); st = _abi.RefineStats()
    rs = C.POINTER(_abi.RefineRangeStat)(); nrs = C.c_int()
    head = (ctx._h if ctx is not None else None, C.byref(prm), float(thr), many, ln, codes.ctypes.data_as(_abi.c_u8p),
            None if w is None else w.ctypes.data_as(_abi.c_f64p), C.byref(T))
    tail = (None if P is None else C.byref(P), C.byref(O), C.byref(out), C.byref(olen), C.byref(steps), C.byref(ns), C.byref(rs), C.byref(nrs),
            C.byref(st))
    if groups is None:
        rc = lib().g2g_refine_planned(*head, *tail)
        if rc != 0:
            raise G2GError("g2g_refine_planned rc=%d: %s" % (rc, last_error()))
    else:
        ss, _keep_s = guide._subset_struct(groups)
        rc = lib().g2g_refine_planned_groups(*head, C.byref(ss), *tail)
        if rc != 0:
            raise G2GError("g2g_refine_planned_groups rc=%d: %s" % (rc, last_error()))
    ranges = [{k: getattr(rs[i], k) for k, _ in _abi.RefineRangeStat._fields_ if k != "reserved"} for i in range(nrs.value)]
    lib().g2g_free(rs)
    final, log, stats = _take_results(many, out, olen, steps, ns, st, moves)
    return final, log, ranges, stats


def refine_groups(ctx, codes: np.ndarray, groups, prm: "_abi.Params", thr: float = 35., flat_leaves: bool = False, plan_prm=None, **opts):
    """prrn's refinement between groups that stay as they are (its multi-profile stage), in one call: the weighting tree over the
    groups and the members' weights (KTree.from_msa_groups <-> IterMsa::phyl_pwt), the plan started from the groups
    (g2g_refine_plan_groups) and the refinement over it (g2g_refine_planned_groups).  plan_prm / opts as for refine_planned.
    Returns what refine_planned returns, then the tree and the weights."""
    tree, weight = KTree.from_msa_groups(ctx, codes, groups, flat_leaves)
    final, log, ranges, stats = refine_planned(ctx, codes, tree, prm, thr, weight, None, plan_prm, groups=groups, **opts)
    return final, log, ranges, stats, tree, weight


def pairsum(ctx, codes: np.ndarray, tree: KTree, alp: op.AlnParam, use_pw: bool = True) -> float:
    """g2g_pairsum: Ssrel::pairsum_ss of an MSA -- the sum-of-pairs score prrn reports"""
    codes = np.ascontiguousarray(codes, np.uint8)
    ln, many = codes.shape
    prm, _sm = alp.to_c()
    T, _keep = tree.to_c()
    out = C.c_double()
    rc = lib().g2g_pairsum(ctx._h, C.byref(prm), many, ln, codes.ctypes.data_as(_abi.c_u8p), C.byref(T), 1 if use_pw else 0, C.byref(out))
    if rc != 0:
        raise G2GError("g2g_pairsum rc=%d: %s" % (rc, last_error()))
    return out.value
