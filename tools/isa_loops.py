#!/usr/bin/env python3
"""Static instruction table of a unit's kernels, loop by loop (runs without a GPU: hipcc cross-compiles gfx950 with the flags
of prrn_aln_amd/build.py and stops at the assembly).

    python3 tools/isa_loops.py v6                      # unit name of build.py, or a .hip path
    python3 tools/isa_loops.py v3 -k g2g_v3r_hf2 --min 40
    python3 tools/isa_loops.py --asm saved.s           # table of an assembly file made before (--keep FILE writes one)

Loops are LLVM's natural loops as the AMDGPU printer marks them ("Loop Header: Depth=N", "in Loop: Header=BBx_y").  Per loop:
its own blocks (those whose innermost loop it is; nested loops are listed on their own rows) and, in `incl`, the instructions
of the loop and everything nested in it.  Columns count instructions as written in the code, not as executed:
  insts      every instruction
  valu       v_* (v_readlane / v_writelane / v_accvgpr_* included)
  salu       s_* except s_nop, s_waitcnt and branches
  rdl_spill  v_readlane_b32 from a spill lane (a VGPR the kernel writes SGPR spills into with v_writelane_b32 at a constant lane)
  wrl_spill  v_writelane_b32 into a spill lane
  s_nop      wait states the compiler inserted
  accvgpr    v_accvgpr_read / v_accvgpr_write / v_accvgpr_mov
  saveexec   s_*_saveexec (exec-mask branches)
  ds         ds_* (LDS)
  vmem       global_* / buffer_* / flat_* / scratch_*
With --lines the unit is compiled with -gline-tables-only (codegen is unchanged by it) and each loop shows the source lines
that most of its own instructions come from."""
from __future__ import annotations

import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLS = ["insts", "valu", "salu", "rdl_spill", "wrl_spill", "s_nop", "accvgpr", "saveexec", "ds", "vmem"]


def compile_asm(src: str, lines: bool, keep: str | None) -> str:
    from prrn_aln_amd import build as b
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "unit.s")
        cmd = [hipcc] + b.FLAGS + b._extra() + ["--cuda-device-only", "-S", "-o", out, src]
        if lines:
            cmd.insert(1, "-gline-tables-only")
        subprocess.check_call(cmd, stderr=subprocess.DEVNULL)
        text = open(out).read()
    if keep:
        open(keep, "w").write(text)
    return text


RE_LABEL = re.compile(r"^(\.LBB(\d+)_(\d+)|; %bb\.\d+):")
RE_HDR = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")
RE_IN = re.compile(r"in Loop: Header=BB(\d+_\d+) Depth=(\d+)")
RE_PARENT = re.compile(r"Parent Loop BB(\d+_\d+) Depth=(\d+)")
RE_LOC = re.compile(r"^\s*\.loc\s+(\d+)\s+(\d+)")
RE_FILE = re.compile(r'^\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?')


def classify(mn: str, ops: str, spill_vgprs: set) -> list:
    c = ["insts"]
    if mn.startswith("v_"):
        c.append("valu")
        if mn.startswith("v_accvgpr"):
            c.append("accvgpr")
        if mn == "v_readlane_b32":
            p = [x.strip() for x in ops.split(",")]
            if len(p) == 3 and p[1] in spill_vgprs and p[2].isdigit():
                c.append("rdl_spill")
        if mn == "v_writelane_b32":
            p = [x.strip() for x in ops.split(",")]
            if len(p) == 3 and p[0] in spill_vgprs and p[2].isdigit():
                c.append("wrl_spill")
    elif mn.startswith("s_"):
        if mn == "s_nop":
            c.append("s_nop")
        elif "saveexec" in mn:
            c += ["salu", "saveexec"]
        elif not (mn.startswith("s_waitcnt") or mn.startswith("s_cbranch") or mn == "s_branch" or mn.startswith("s_setpc")):
            c.append("salu")
    elif mn.startswith("ds_"):
        c.append("ds")
    elif mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        c.append("vmem")
    return c


def kernel_meta(text: str) -> dict:
    meta = {}
    for chunk in re.split(r"\n  - \.", text.split("amdhsa.kernels:", 1)[-1]):
        m = re.search(r"\.name:\s+(\S+)", chunk)
        if not m:
            continue
        g = lambda k: (int(re.search(r"\.%s:\s+(\d+)" % k, chunk).group(1)) if re.search(r"\.%s:\s+(\d+)" % k, chunk) else None)
        meta[m.group(1)] = {"sgpr_spill_count": g("sgpr_spill_count"), "vgpr_spill_count": g("vgpr_spill_count"),
                            "private_segment_fixed_size": g("private_segment_fixed_size"), "sgpr_count": g("sgpr_count"),
                            "vgpr_count": g("vgpr_count"), "agpr_count": g("agpr_count")}
    return meta


def parse(text: str):
    """-> {kernel: (loops, counts per loop (None: outside every loop), source lines per loop, file table)}; loops: {hdr: [depth, parent]}"""
    files = {}
    kernels = collections.OrderedDict()
    lines = text.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(?:;.*)?$", lines[i])
        if not m or lines[i].startswith("."):
            fm = RE_FILE.match(lines[i])
            if fm:
                files[fm.group(1)] = fm.group(3) or fm.group(2)
            i += 1
            continue
        name = m.group(1)
        j = i + 1
        while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
            j += 1
        kernels[name] = lines[i + 1:j]
        i = j + 1
    out = collections.OrderedDict()
    for name, body in kernels.items():
        spill = set()
        for l in body:
            t = l.strip().split(None, 1)
            if len(t) == 2 and t[0] == "v_writelane_b32":
                p = [x.strip() for x in t[1].split(",")]
                if len(p) == 3 and p[2].isdigit():
                    spill.add(p[0])
        loops = collections.OrderedDict()             # header -> [depth, parent]
        own = collections.defaultdict(collections.Counter)
        src = collections.defaultdict(collections.Counter)
        cur = None                                    # innermost loop of the current block (None: outside every loop)
        pending_parent = None
        loc = None
        for l in body:
            lm = RE_LABEL.match(l)
            if lm:
                cur, pending_parent = None, None
                bbname = ("BB%s_%s" % (lm.group(2), lm.group(3))) if lm.group(2) else None
            s = l.strip()
            if s.startswith(";") or lm:
                com = l.split(";", 1)[1] if ";" in l else ""
                pm = RE_PARENT.search(com)
                if pm:
                    pending_parent = "BB" + pm.group(1)
                hm = RE_HDR.search(com)
                if hm and bbname:
                    loops[bbname] = [int(hm.group(1)), pending_parent]
                    cur = bbname
                im = RE_IN.search(com)
                if im:
                    cur = "BB" + im.group(1)
                continue
            fl = RE_LOC.match(l)
            if fl:
                loc = (fl.group(1), int(fl.group(2)))
                continue
            if not s or s.startswith(".") or s.endswith(":"):
                continue
            t = s.split(None, 1)
            mn, ops = t[0], (t[1] if len(t) > 1 else "")
            for c in classify(mn, ops.split(";")[0], spill):
                own[cur][c] += 1
            if loc:
                src[cur][loc] += 1
        out[name] = (loops, own, src, files)
    return out


def incl(loops, own):
    tot = {h: collections.Counter(own[h]) for h in loops}
    for h in sorted(loops, key=lambda h: -loops[h][0]):
        p = loops[h][1]
        if p in tot:
            tot[p].update(tot[h])
    return tot


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("unit", nargs="?", default="v6", help="unit of prrn_aln_amd/build.py (engine, v2, v3, v6, v78) or a .hip file")
    ap.add_argument("-k", "--kernel", action="append", help="only these kernels (default: every kernel whose name starts with g2g_)")
    ap.add_argument("--asm", help="read this assembly file instead of compiling")
    ap.add_argument("--keep", help="write the assembly here")
    ap.add_argument("--min", type=int, default=20, help="hide loops with fewer inclusive instructions (default 20)")
    ap.add_argument("--lines", action="store_true", help="compile with line tables and name each loop's main source lines")
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        from prrn_aln_amd import build as b
        src = a.unit if a.unit.endswith(".hip") else os.path.join(b.CSRC, b.UNITS[a.unit][0])
        text = compile_asm(src, a.lines, a.keep)
    meta = kernel_meta(text)
    res = parse(text)
    for name, (loops, own, src, files) in res.items():
        if a.kernel and name not in a.kernel:
            continue
        if not a.kernel and not name.startswith("g2g_"):
            continue
        md = meta.get(name, {})
        print("== %s   sgpr_spill_count %s  vgpr_spill_count %s  private_segment %s B  sgpr %s  vgpr %s  agpr %s" % (
            name, md.get("sgpr_spill_count"), md.get("vgpr_spill_count"), md.get("private_segment_fixed_size"),
            md.get("sgpr_count"), md.get("vgpr_count"), md.get("agpr_count")))
        whole = collections.Counter()
        for c in own.values():
            whole.update(c)
        tot = incl(loops, own)
        hdr = "%-22s %5s " % ("loop (header, depth)", "") + " ".join("%9s" % c for c in COLS) + "  %7s" % "incl"
        print(hdr)
        print("%-28s " % "kernel" + " ".join("%9d" % whole[c] for c in COLS) + "  %7d" % whole["insts"])
        print("%-28s " % "outside loops" + " ".join("%9d" % own[None][c] for c in COLS))

        def walk(h, ind):
            if tot[h]["insts"] < a.min:
                return
            lbl = "%s%s d%d" % ("  " * ind, h, loops[h][0])
            line = "%-28s " % lbl + " ".join("%9d" % own[h][c] for c in COLS) + "  %7d" % tot[h]["insts"]
            if a.lines and src[h]:
                top = src[h].most_common(3)
                line += "   " + ", ".join("%s:%d" % (os.path.basename(files.get(f, f)), ln) for (f, ln), _ in top)
            print(line)
            for k in loops:
                if loops[k][1] == h:
                    walk(k, ind + 1)
        for h in loops:
            if loops[h][1] is None:
                walk(h, 0)
        print()


if __name__ == "__main__":
    main()
