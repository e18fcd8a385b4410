"""Restatement of the reference's conserved-region search (src/consreg.cc) in plain Python / numpy, working from the HOST-built
arrays of a g2g_pwdm (the host builders are pinned to the reference elsewhere in this suite):

    colscores   s of every column: cons2_ng / cons2_nv / cons2_hf / cons2_pf (consreg.cc:170-406) by the PwdM's banded mode --
                PwdM::sim?? (src/maln2.cc:534-623, 1230-1296), the d3 = 0 branch of PwdM::crg?? (:881-1024, 1454-1614),
                PwdM::newgap2(asi, bs, glb) (:850-879), newgap(cf, df) (src/gfreq.cc:493-505); pregap / incrgap for the members'
                gap runs (src/seq.cc:1870-1883, src/mgaps.cc:431-440)
    scan        the thresholded running sum every cons2_* ends with (consreg.cc:184-207)
    cmnrng      src/css.cc:261-282, complerng: the complement inside [0, len)
    divisions   the 2 N - 3 branches of the weighting tree as Randiv's tree_tab / bin2lst2g hand them out (src/randiv.cc:88-156)
    consreg     Ssrel::consreg (consreg.cc:484-518)

Every sum is formed element by element in the reference's order (Python floats are IEEE doubles, nothing is fused), so the column
scores are the device's bit for bit."""
import ctypes as C
import glob
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "consreg")
NGP_ALB, HLF_ALB, RHF_ALB, GPF_ALB, NTV_ALB = 6, 7, 8, 9, 10
MODE_NAME = {NGP_ALB: "ng", HLF_ALB: "hf", RHF_ALB: "hf", GPF_ALB: "pf", NTV_ALB: "nv"}


def fixtures():
    return [(os.path.basename(f)[:-4], dict(np.load(f))) for f in sorted(glob.glob(os.path.join(GOLD, "*.npz")))]


# ---- the host arrays of one side of a g2g_problem ------------------------------------------------------------------------------
class SideView:
    def __init__(self, s):
        self.many, self.len, self.nelm, self.felm = s.many, s.len, s.nelm, s.felm
        cols = s.len + 2
        arr = lambda p, n, shape=None: None if not p else np.ctypeslib.as_array(p, shape=(n,)).copy().reshape(shape or (n,))
        self.seq = arr(s.seq, cols * s.many, (cols, s.many))[1:]                          # position 0 first
        self.weight = arr(s.weight, s.many)
        self.pseq = arr(s.pseq, cols * s.nelm, (cols, s.nelm))[1:] if s.pseq and s.nelm > 0 else None
        self.gapdens = arr(s.gapdens, cols * s.many, (cols, s.many))[1:] if s.gapdens else None
        self.lists = None
        if s.has_gfq:
            self.lists = []
            for v in range(3):
                off = arr(s.gfq.off[v], s.len + 2)
                pool = int(off[s.len + 1])
                self.lists.append((off, arr(s.gfq.glen[v], pool), arr(s.gfq.freq[v], pool)))

    def gfq(self, view, pos):
        """the list of a position as [(glen, freq)] without its terminator"""
        off, glen, freq = self.lists[view]
        out = []
        k = int(off[pos + 1])
        while glen[k] >= 0:
            out.append((int(glen[k]), float(freq[k])))
            k += 1
        return out


class ProblemView:
    def __init__(self, p):
        self.alnmode, self.sim2_kind, self.crg2_kind = p.alnmode, p.sim2_kind, p.crg2_kind
        self.basic_gop, self.weighted_gop = p.basic_gop, p.weighted_gop
        self.simmtx = np.ctypeslib.as_array(p.simmtx, shape=(p.simrows * p.simdim,)).copy().reshape(p.simrows, p.simdim) if p.simmtx else None
        self.a, self.b = SideView(p.a), SideView(p.b)


# ---- PwdM::sim?? ---------------------------------------------------------------------------------------------------------------
def sim2(P, c):
    a, b, mtx, kind = P.a, P.b, P.simmtx, P.sim2_kind
    ar, br = a.seq[c], b.seq[c]
    s = 0.0
    if kind == 0:
        return 0.0
    if kind == 11:
        return float(mtx[ar[0], br[0]])
    if kind == 120:
        for j in range(b.many):
            s += float(mtx[ar[0], br[j]])
        return s
    if kind == 121:
        for j in range(b.many):
            s += float(mtx[ar[0], br[j]]) * float(b.weight[j])
        return s
    if kind == 13:
        return float(b.pseq[c][b.felm + ar[0]])
    if kind == 210:
        for i in range(a.many):
            s += float(mtx[br[0], ar[i]])
        return s
    if kind == 211:
        for i in range(a.many):
            s += float(mtx[br[0], ar[i]]) * float(a.weight[i])
        return s
    if kind == 220:
        for i in range(a.many):
            for j in range(b.many):
                s += float(mtx[ar[i], br[j]])
        return s
    if kind == 221:
        for i in range(a.many):
            st = 0.0
            for j in range(b.many):
                st += float(mtx[ar[i], br[j]]) * float(b.weight[j])
            s += st * float(a.weight[i])
        return s
    if kind in (230, 231):
        vb = b.pseq[c][b.felm:]
        for i in range(a.many):
            s += float(vb[ar[i]]) * float(a.weight[i]) if kind == 231 else float(vb[ar[i]])
        return s
    if kind == 31:
        return float(a.pseq[c][a.felm + br[0]])
    if kind in (320, 321):
        va = a.pseq[c][a.felm:]
        for j in range(b.many):
            s += float(va[br[j]]) * float(b.weight[j]) if kind == 321 else float(va[br[j]])
        return s
    if kind in (33, 330):
        va, vb = a.pseq[c][a.felm:], b.pseq[c]
        dc = (0, 1, 2, 3, 5, 9)                                             # decompact, mseq.h:41
        for j in range(b.felm):
            s += float(va[dc[j] if kind == 330 else j]) * float(vb[j])
        return s
    raise ValueError("sim2 kind %d" % kind)


# ---- PwdM::crg??, d3 = 0 -------------------------------------------------------------------------------------------------------
def crg2_diag(P, c, gla, glb):
    a, b, kind = P.a, P.b, P.crg2_kind
    as_, bs = a.seq[c], b.seq[c]
    agd, bgd = a.gapdens[c], b.gapdens[c]
    wa, wb = a.weight, b.weight
    ng = lambda x: x > 1
    g = 0.0
    if kind == 11:
        if ng(as_[0]) and bgd[0] > 0 and gla[0] >= glb[0]:
            return float(bgd[0]) * P.basic_gop
        if ng(bs[0]) and agd[0] > 0 and glb[0] >= gla[0]:
            return float(agd[0]) * P.basic_gop
        return 0.0
    if kind in (120, 121):
        w = kind & 1
        if ng(as_[0]):
            for j in range(b.many):
                if bgd[j] > 0 and gla[0] >= glb[j]:
                    g += float(wb[j]) * float(bgd[j]) if w else float(bgd[j])
        elif agd[0] > 0:
            for j in range(b.many):
                if ng(bs[j]) and glb[j] >= gla[0]:
                    g += float(wb[j]) * float(agd[0]) if w else float(agd[0])
        return g * P.basic_gop
    if kind in (210, 211):
        w = kind & 1
        if ng(bs[0]):
            for i in range(a.many):
                if agd[i] > 0 and glb[0] >= gla[i]:
                    g += float(wa[i]) * float(agd[i]) if w else float(agd[i])
        elif bgd[0] > 0:
            for i in range(a.many):
                if ng(as_[i]) and gla[i] >= glb[0]:
                    g += float(wa[i]) * float(bgd[0]) if w else float(bgd[0])
        return g * P.basic_gop
    if kind == 220:
        for i in range(a.many):
            if ng(as_[i]):
                for j in range(b.many):
                    if bgd[j] > 0 and gla[i] >= glb[j]:
                        g += float(bgd[j])
            elif agd[i] > 0:
                for j in range(b.many):
                    if ng(bs[j]) and glb[j] >= gla[i]:
                        g += float(agd[i])
        return g * P.basic_gop
    if kind == 221:
        for i in range(a.many):
            s = 0.0
            if ng(as_[i]):
                for j in range(b.many):
                    if bgd[j] > 0 and gla[i] >= glb[j]:
                        s += float(wb[j]) * float(bgd[j])
            elif agd[i] > 0:
                for j in range(b.many):
                    if ng(bs[j]) and glb[j] >= gla[i]:
                        s += float(wb[j]) * float(agd[i])
            g += s * float(wa[i])
        return g * P.basic_gop
    raise ValueError("crg2 kind %d" % kind)


def newgap_static(cf, df):
    """newgap(cf, df), gfreq.cc:493-505"""
    g = 0.0
    ci = 0
    for dg, dfq in df:
        while ci < len(cf) and cf[ci][0] < dg:
            ci += 1
        if ci == len(cf):
            break
        g += cf[ci][1] * dfq
    return g


def newgap2(P, c, glb):
    """PwdM::newgap2(asi, bs, glb), maln2.cc:850-879 (no terminal discount: the density of a gap is 1)"""
    a, b = P.a, P.b
    bs = b.seq[c]
    adf, acf = a.gfq(1, c), a.gfq(0, c)
    g = 0.0
    for j in range(b.many):
        w = float(b.weight[j]) if b.weight is not None else 1.0
        if bs[j] > 1:
            for gl, fq in adf:
                if glb[j] < gl:
                    break
                g += fq * w
        else:
            bu = 1.0
            for gl, fq in acf:
                if gl >= glb[j]:
                    g += fq * w * bu
                else:
                    break
    return P.weighted_gop * g


def incrgap(gl, res):
    for i in range(len(gl)):
        gl[i] = gl[i] + 1 if res[i] <= 1 else 0


def colscores(problem):
    """s of every column of a juxtaposed pair (both groups whole, same length): float64[len]"""
    P = problem if isinstance(problem, ProblemView) else ProblemView(problem)
    n = P.a.len
    assert P.b.len == n
    out = np.zeros(n, np.float64)
    mode = MODE_NAME[P.alnmode]
    gla, glb = [0] * P.a.many, [0] * P.b.many                               # pregap with left = 0
    for c in range(n):
        s = sim2(P, c)
        if mode == "nv":
            s = s + crg2_diag(P, c, gla, glb)
            incrgap(gla, P.a.seq[c])
            incrgap(glb, P.b.seq[c])
        elif mode == "hf":
            s = s + newgap2(P, c, glb)
            incrgap(glb, P.b.seq[c])
        elif mode == "pf":
            s = s + newgap_static(P.a.gfq(0, c), P.b.gfq(1, c)) * P.basic_gop + newgap_static(P.b.gfq(0, c), P.a.gfq(1, c)) * P.basic_gop
        out[c] = s
    return out


def scan(s, vthr):
    """the ranges of one division, consreg.cc:184-207: [(left, right)]"""
    out = []
    scr = mxv = 0.0
    left = right = 0
    for i, x in enumerate(s):
        x = float(x)
        if scr == 0 and x > 0:
            left = i
        scr += x
        if scr < 0:
            scr = 0.0
        elif scr >= vthr and scr > mxv:
            mxv = scr
            right = i + 1
        if mxv > 0 and (scr <= 0 or scr < mxv - vthr):
            out.append((left, right))
            mxv = scr = 0.0
    if scr >= vthr:
        out.append((left, right))
    return out


def cmnrng(a, b):
    """cmnrng(a, b, 0), css.cc:261-282: the intersection of two ascending lists of disjoint ranges; empty pieces are dropped"""
    out = []
    i = j = 0
    while i < len(a) and j < len(b):
        a_low = a[i][1] <= b[j][1]
        ll, uu = (a[i], b[j]) if a_low else (b[j], a[i])
        if ll[1] >= uu[0]:
            left, right = max(a[i][0], b[j][0]), ll[1]
            if right - left > 0:
                out.append((left, right))
        if a_low:
            i += 1
        else:
            j += 1
    return out


def complerng(length, r):
    """complerng(c, a), css.cc:313-336, with c the single range [0, length)"""
    out = []
    left = 0
    for l, rr in r:
        if left < l:
            out.append((left, l))
        left = rr
    if left < length:
        out.append((left, length))
    return out


def divisions(left, right, parent, many):
    """[(son 0 = the members outside, son 1 = the members below the node)] for node 0 .. 2 many - 4, both ascending (tree_tab +
    bin2lst2g); the tree is numbered as the reference numbers it: leaves first, the root last"""
    nn = 2 * many - 1
    below = {}

    def leaves(k):
        if k not in below:
            below[k] = [k] if left[k] < 0 else sorted(leaves(int(left[k])) + leaves(int(right[k])))
        return below[k]
    out = []
    for k in range(2 * many - 3):
        ins = leaves(k)
        inset = set(ins)
        outs = [m for m in range(many) if m not in inset]
        out.append((outs, ins))
    assert parent[nn - 1] < 0
    return out


def vthr_of(pwd, thr):
    from prrn_aln_amd import operator as op
    return op.spparams(pwd).vab * float(thr)


def host_pair(codes, lists, alp, weight=None):
    """the host-built PwdM of two sons extracted as Seq::extseq does (every column kept; weights handed down, a single member 1)"""
    from prrn_aln_amd import operator as op
    sons = []
    for lst in lists:
        w = None if weight is None else ([1.0] if len(lst) == 1 else [float(weight[m]) for m in lst])
        sons.append(op.mSeq(np.ascontiguousarray(codes[:, lst]), alp, w))
    return op.PwdM(sons, alp)


def consreg(codes, tree, alp, thr=35., weight=None, dissim=False, want_divisions=False):
    """Ssrel::consreg on the host: tree = (left, right, parent)"""
    ln, many = codes.shape
    united = [(0, ln)]
    per = []
    for lists in divisions(tree[0], tree[1], tree[2], many):
        pw = host_pair(codes, lists, alp, weight)
        rng = scan(colscores(pw.problem), vthr_of(pw, thr))
        per.append((pw.alnmode, rng))
        united = cmnrng(united, rng)
    if dissim:
        united = complerng(ln, united)
    return (united, per) if want_divisions else united


def alp_of(g):
    """the AlnParam of a fixture: the reference's localprm with the recorded u, v and similarity matrix"""
    from prrn_aln_amd import operator as op
    molc = int(g["molc"][0])
    return op.AlnParam(u=float(g["u"][0]), v=float(g["v"][0]), u0=0.0, u1=0.0, tgapf=1.0, scale=1.0, gamma=0.5, k1=7, ls=2, sh=100,
                       banded=1, molc=molc, simmtx=np.ascontiguousarray(g["simmtx"], np.float64), max_code=int(g["max_code"][0]))


def fixture_divisions(g):
    """[(son 0, son 1, ranges, in_tree)] as recorded; in_tree 0: a division of the tree recorded again with its sons exchanged"""
    out = []
    for k in range(int(g["ndiv"][0])):
        l0 = g["div_l0"][g["div_l0_off"][k]:g["div_l0_off"][k + 1]]
        l1 = g["div_l1"][g["div_l1_off"][k]:g["div_l1_off"][k + 1]]
        r = g["div_rng"][g["div_rng_off"][k]:g["div_rng_off"][k + 1]]
        out.append(([int(x) for x in l0], [int(x) for x in l1], [(int(a), int(b)) for a, b in r], int(g["div_in_tree"][k])))
    return out
