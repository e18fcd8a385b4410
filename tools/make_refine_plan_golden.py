#!/usr/bin/env python3
"""Generate tests/golden/refine_plan/*.json from the REAL reference (oracle/_ref): prrn's DEFAULT refinement (local_thr = 35,
IterMsa::preprrn, src/prrn5.cc:785-839) on small seeded families -- fused groups, one Prrn per unconserved column range.  Data only.

Which binary gives which field
  oracle/_ref/prrn5 -R1 [-yl3] fam.msa   (the unmodified reference, every case)
      final_rows   the alignment it prints on stdout
      ranges       the attack ranges it prints on stderr (`4  4;  0 44; 68 150;`: a header entry, then the ranges)
      prrn         one entry per `Prrn` line on stderr (`( 1 - 44 )  501.3 <--  498.8, 11 grp,  31 rep`): the range it belongs to (by its
                   left column), the one-based columns after refinement, sps, initsp, groups, rep (= Prrn::countaln)
  oracle/_ref/prrn5_trace -R1 -O4 [-yl3] fam.msa   (the same prrn5.cc linked with oracle/ref_trace.cc; TRACED cases only)
      trace        per Prrn, in processing order (last range first): cycle, the relation's tree (T records), the branches (D), every align2
                   (A: member counts, swp, scr, val, the member weights of both sides) and every accepted move (S: member lists, skeleton).
                   The `C` record with no pairsum_ss (`P`) record before it is the Randiv that Ssrel::consreg builds (rn = 0: it walks the
                   divisions in order and draws nothing from rand()); it is skipped.
                   The tracer is used only where nothing fuses: its pairsum_ss wrapper walks 2 many - 1 nodes of a tree that has 2 num - 1.
  tests/ktreelib.py   (the restatement of Ktree(msd) + calcpw, pinned against the reference elsewhere)
      tree, weight   the member tree of the start MSA and msd->weight as phyl_pwt leaves it (vol of the leaves); for a traced case the
                   tree is asserted equal to the T records
  tests/golden/fuse/*.npz   (recorded from the reference by tools/make_fuse_golden.py)
      plan_simmtx  similarity matrix number 1 of the molecule, which the reference's localprm (consreg.cc:39-40: u 3, v 10, thr 35) uses

Before a case is saved: tests/fuselib.py's plan of the start MSA gives the printed ranges and per printed line the printed group count;
the final rows differ from the start rows; g2g_refine_planned (CPU checker scoring) does not refuse the case for an empty leaf group.
Over all cases each condition of COND must occur; the conditions are printed per case.

Usage: python tools/make_refine_plan_golden.py          every case (one process each), then the check over the set
       python tools/make_refine_plan_golden.py <case>   one case
       python tools/make_refine_plan_golden.py --check  the conditions over the committed set"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
REF = os.path.join(ROOT, "oracle", "_ref")
GOLD = os.path.join(ROOT, "tests", "golden", "refine_plan")
_AA = "ARNDCQEGHILKMFPSTWYV"
_NT = "ACGT"
COND = ("accepted_in_fused_group_range", "accepted_after_first_range", "range_skipped", "two_or_three_groups_run", "length_change_then_range",
        "whole_fused", "dna_yl3")


def slide_gaps(rows, seed, frac=0.5):
    """the start alignment made wrong in places: in a random subset of rows every gap run changes places with the 1 .. 4 residues on its right"""
    rng = np.random.default_rng(seed)
    out = []
    for r in rows:
        r = list(r)
        if rng.random() < frac:
            i = 0
            while i < len(r):
                if r[i] != "-":
                    i += 1
                    continue
                j = i
                while j < len(r) and r[j] == "-":
                    j += 1
                k = int(rng.integers(1, 5))
                if j + k <= len(r) and "-" not in r[j:j + k]:
                    seg = r[j:j + k]
                    r[i:i + k] = seg
                    r[i + k:j + k] = ["-"] * (j - i)
                i = j + k
        out.append("".join(r))
    return out


def run_reference(rows, extra, traced):
    """(final rows, ranges, prrn lines, trace lines or None)"""
    import refdump
    from make_refine_golden import parse_msa
    names = ["s%02d" % i for i in range(len(rows))]
    env = dict(os.environ, ALN_TAB=os.path.join(REF, "table"))
    with tempfile.TemporaryDirectory() as tmp:
        refdump.write_multi(os.path.join(tmp, "fam.msa"), names, list(rows), "fam")
        p = subprocess.run([os.path.join(REF, "prrn5"), "-R1"] + extra + ["fam.msa"], cwd=tmp, env=env, check=True, capture_output=True, text=True)
        L = None
        if traced:
            tr = os.path.join(tmp, "trace.txt")
            subprocess.run([os.path.join(REF, "prrn5_trace"), "-R1", "-O4"] + extra + ["fam.msa"], cwd=tmp, env=dict(env, G2G_TRACE=tr), check=True, capture_output=True)
            L = [l.rstrip("\n") for l in open(tr)]
    final, order = parse_msa(p.stdout)
    assert order == names, order[:3]
    width = max(len(r) for r in final)
    final = [r.ljust(width, "-").replace(" ", "-") for r in final]
    ranges, prrn = None, []
    for line in p.stderr.splitlines():
        if ranges is None and re.match(r"^\s*(\d+\s+\d+;\s*)+$", line):
            ent = [tuple(int(x) for x in e.split()) for e in line.split(";") if e.strip()]
            assert ent[0][0] == ent[0][1] == len(ent) + 1, ent          # (the header counts itself and the closing sentinel)
            ranges = [list(e) for e in ent[1:]]
        m = re.search(r"\(\s*(\d+) - (\d+)\s*\)\s+(-?[\d.]+) <--\s+(-?[\d.]+),\s*(\d+) grp,\s*(\d+) rep,", line)
        if m:
            prrn.append(dict(left1=int(m.group(1)), right1=int(m.group(2)), sps=float(m.group(3)), initsp=float(m.group(4)), groups=int(m.group(5)), rep=int(m.group(6))))
    assert ranges is not None, p.stderr[:400]
    return final, ranges, prrn, L


def parse_trace(L):
    """the Prrns of a trace in order: [dict(cycle, num, tree, branches, align2, accepted)]"""
    out, cur, after_p = [], None, False
    for l in L:
        k = l[:2]
        if k == "P ":
            after_p = True                      # Prrn::Prrn scores the start (initsp) just before rir builds its Randiv
        if k == "C ":
            if cur is not None:
                out.append(cur)
            _, cyc, nn = l.split()
            # the Randiv of Ssrel::consreg (rn = 0: it walks 0 .. cycle - 1, draws nothing from rand()) has no pairsum_ss before it
            cur = dict(cycle=int(cyc), num=int(nn), T=[], branches=[], align2=[], accepted=[]) if after_p else None
            after_p = False
        elif cur is None:
            continue
        elif k == "T " and not cur["branches"]:
            cur["T"].append(l.split())
        elif k == "D ":
            cur["branches"].append(int(l.split()[1]))
        elif k == "A " and cur["branches"]:
            p = l.split("|")
            h = p[0].split()
            cur["align2"].append(dict(na=int(h[1]), nb=int(h[2]), swp=int(h[3]), scr=float(h[4]), val=float(h[5]),
                                      wa=[float(x) for x in p[3].split()], wb=[float(x) for x in p[4].split()]))
        elif k == "S " and cur["branches"]:
            p = l.split("|")
            sk = [int(x) for x in p[3].split()]
            cur["accepted"].append(dict(lst0=[int(x) for x in p[1].split()], lst1=[int(x) for x in p[2].split()], skl=[sk[i:i + 2] for i in range(0, len(sk), 2)]))
    if cur is not None:
        out.append(cur)
    for t in out:
        T = t.pop("T")
        assert [int(x[1]) for x in T] == list(range(2 * t["num"] - 1)), "the T records are not the relation's 2 num - 1 nodes"
        t["tree"] = dict(left=[int(x[2]) for x in T], right=[int(x[3]) for x in T], parent=[int(x[4]) for x in T], vol=[float(x[5]) for x in T], cur=[float(x[6]) for x in T])
    return out


def plan_simmtx(molc):
    g = np.load(os.path.join(ROOT, "tests", "golden", "fuse", "prot12_clusters.npz" if molc == 1 else "dna9_clusters.npz"))
    assert int(g["molc"][0]) == molc
    return g["simmtx"], int(g["max_code"][0])


def run(name, molc, rows, extra=(), traced=False, save=True):
    import ktreelib as kl
    import refineplanlib as rp
    from prrn_aln_amd import operator as op
    extra = list(extra)
    assert 6 <= len(rows) <= 16 and 150 <= len(rows[0]) <= 400, "families of 6 to 16 members and 150 to 400 columns"
    final, ranges, prrn, L = run_reference(rows, extra, traced)
    codes = op.encode(rows, molc)
    ln, many = codes.shape
    t = kl.tree_from_dist(kl.divergence(codes)[0])
    sm, max_code = plan_simmtx(molc)
    fix = dict(name=name, kind="traced" if traced else "grouped", molc=molc, max_code=max_code, ls=3 if "-yl3" in extra else 1, options=["-R1"] + extra,
               rows=list(rows), tree={k: [float(x) if k in ("vol", "cur") else int(x) for x in t[k]] for k in ("left", "right", "parent", "vol", "cur")},
               weight=[float(x) for x in t["vol"][:many]], thr=35., plan_u=3., plan_v=10., plan_simmtx=np.asarray(sm).tolist(),
               ranges=ranges, prrn=prrn, final_rows=final)
    # the printed lines belong to ranges by their left column (a range's left never moves: the ranges before it lie to its right)
    by_left = {r[0]: i for i, r in enumerate(ranges)}
    for p in prrn:
        assert p["left1"] - 1 in by_left, (p, ranges)
        p["range"] = by_left[p["left1"] - 1]
    assert [p["range"] for p in prrn] == sorted((p["range"] for p in prrn), reverse=True), "the Prrn lines do not run from the last range to the first"
    if traced:
        tr = parse_trace(L)
        assert len(tr) == len(prrn), "the trace holds %d Prrns, %d lines were printed" % (len(tr), len(prrn))
        for x, p in zip(tr, prrn):
            x["range"] = p["range"]
            assert x["num"] == p["groups"] == many, "a traced case must not fuse anything"
            for k in ("left", "right", "parent"):
                assert x["tree"][k] == fix["tree"][k], "the restated member tree differs from the T records (%s)" % k
            for k in ("vol", "cur"):
                assert np.array_equal(np.asarray(x["tree"][k]).view(np.int64), np.asarray(fix["tree"][k]).view(np.int64)), "the restated member tree differs from the T records (%s)" % k
            del x["tree"]
        fix["trace"] = tr
    os.makedirs(GOLD, exist_ok=True)
    path = os.path.join(GOLD, "%s_%s.json" % (fix["kind"], name))
    tmp = path + ".tmp"
    json.dump(fix, open(tmp, "w"))
    try:
        case = rp.Case(tmp)
        # 1. the restated plan gives the printed ranges and group counts
        pl = case.restated()
        assert [list(r) for r in pl["ranges"]] == ranges, "the restated plan's ranges %s, printed %s" % (pl["ranges"], ranges)
        pr = case.printed()
        for i, (f, rel, org) in enumerate(pl["per_range"]):
            if i in pr:
                assert len(rel[0]) == pr[i]["groups"], "range %d: %d groups restated, %d printed" % (i, len(rel[0]), pr[i]["groups"])
            else:
                assert len(rel[0]) < 2, "range %d printed no Prrn line but has %d groups" % (i, len(rel[0]))
        if traced:
            assert not pl["whole"][0] and not any(f for f, _, _ in pl["per_range"]), "a traced case must not fuse anything"
        # 2. something moved
        assert final != [r.ljust(len(final[0]), "-") for r in rows] or len(final[0]) != ln, "the final rows are the start rows"
        assert final != list(rows), "the final rows are the start rows"
        # 4. the product does not refuse the case (an empty leaf group would be G2G_ERR_MODE)
        got, steps, rstat, stats = rp.run_host(case)
        cond = conditions(case, rstat)
        same = np.array_equal(got, case.final)
    finally:
        os.remove(tmp)
    print("%-26s %2d x %3d -> %3d: ranges %s, groups %s, rep %s, accepted %s, whole groups %d | final %s | %s"
          % (fix["kind"] + "_" + name, many, ln, len(final[0]), ranges, [r["groups"] for r in rstat], [pr[i]["rep"] if i in pr else None for i in range(len(ranges))],
             [r["accepted"] for r in rstat], len(pl["whole"][1][0]), "as the product's" if same else "DIFFERS from the product's", " ".join(c for c in COND if cond[c])))
    if save:
        json.dump(fix, open(path, "w"))
    return cond


def conditions(case, rstat):
    """which of COND a case shows; accepted moves are read off the product's run (CPU checker scoring), which the tests hold to the printed
    lines and the final rows"""
    pl = case.restated()
    order = [r for r in sorted(rstat, key=lambda r: -r["range"])]          # processing order
    ran = [r for r in order if r["nsteps"]]
    c = dict.fromkeys(COND, False)
    for r in order:
        groups = pl["per_range"][r["range"]][1][0]
        if r["accepted"] and any(len(g) >= 2 for g in groups):
            c["accepted_in_fused_group_range"] = True
        if r["accepted"] and ran and r is not ran[0]:
            c["accepted_after_first_range"] = True
        if r["groups"] < 2:
            c["range_skipped"] = True
        if r["groups"] in (2, 3) and r["nsteps"]:
            c["two_or_three_groups_run"] = True
        if r["out_right"] - r["out_left"] != r["right"] - r["left"] and any(q["nsteps"] and q["range"] < r["range"] for q in order):
            c["length_change_then_range"] = True
    c["whole_fused"] = bool(pl["whole"][0])
    c["dna_yl3"] = case.molc == 2 and case.f["ls"] == 3
    return c


def check_set():
    import refineplanlib as rp
    seen = dict.fromkeys(COND, False)
    kinds = {"traced": 0, "grouped": 0}
    for p in rp.fixtures():
        case = rp.Case(p)
        kinds[case.f["kind"]] += 1
        c = conditions(case, rp.run_host(case)[2])
        print("%-28s %s" % (rp.fixture_id(p), " ".join(k for k in COND if c[k])))
        for k in COND:
            seen[k] = seen[k] or c[k]
    assert kinds["traced"] >= 2 and kinds["grouped"] >= 4, kinds
    missing = [k for k in COND if not seen[k]]
    assert not missing, "no case shows: %s" % ", ".join(missing)
    print("every condition occurs; %d traced and %d grouped cases" % (kinds["traced"], kinds["grouped"]))


def family(sizes, length, seed, blocks, slide, **kw):
    from make_fuse_golden import clustered
    return slide_gaps(clustered(sizes, length, seed, blocks, **kw), slide)


def _others(n):
    return tuple(range(1, n))


_B3 = [(0, 38, (1, 2)), (71, 150, (2,)), (71, 110, (1,))]
JOBS = {
    # ---- traced: nothing fuses anywhere, the MSA splits into ranges (inside a block every member has an ancestor of its own)
    "t_prot6": lambda: run("prot6x260", 1, family([1] * 6, 260, 31, [(30, 90, (1, 2, 3)), (150, 220, (3, 4, 5))], 5, within=0.08, gaps=0.02), traced=True),
    "t_prot8": lambda: run("prot8x300", 1, family([1] * 8, 300, 44, [(20, 70, _others(8)), (120, 180, _others(8)), (230, 280, _others(8))], 5, within=0.05, gaps=0.02), traced=True),
    # ---- grouped: plain prrn5 only
    # singletons that fuse inside ranges; the first range fuses to one group and is skipped; lengths change
    "g_prot6": lambda: run("prot6x260", 1, family([1] * 6, 260, 21, [(30, 90, (1, 2, 3)), (150, 220, (3, 4, 5))], 5, within=0.05, gaps=0.02)),
    # a range of two groups: the one division, once
    "g_prot8": lambda: run("prot8x300", 1, family([1] * 8, 300, 23, [(20, 70, (1, 2, 3, 4)), (120, 180, (4, 5, 6, 7)), (230, 280, (0, 2, 4, 6))], 5, within=0.05, gaps=0.02)),
    # two clusters of eight: a range of three groups with an accepted move between ranges of sixteen
    "g_prot16": lambda: run("prot16x400", 1, slide_gaps(family([8, 8], 400, 20, [(0, 90, (1,)), (200, 260, (1,))], 6, within=0.02, gaps=0.025), 16, 1.0)),
    # DNA with -yl3; two members fuse over the whole MSA
    "g_dna8": lambda: run("dna8x240_ls3", 2, family([1] * 8, 240, 41, [(30, 90, _others(8)), (150, 210, _others(8))], 5, alphabet=_NT, within=0.04, gaps=0.02), extra=["-yl3"]),
    # DNA with -yl3: a range of two groups, a skipped range, a length that changes
    "g_dna8b": lambda: run("dna8x240_ls3_b", 2, family([1] * 8, 240, 46, [(30, 90, _others(8)), (150, 210, _others(8))], 5, alphabet=_NT, within=0.04, gaps=0.02), extra=["-yl3"]),
}

if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--check":
        check_set()
    elif len(sys.argv) > 1:
        JOBS[sys.argv[1]]()
    else:
        for j in JOBS:
            subprocess.check_call([sys.executable, os.path.abspath(__file__), j])
        check_set()
