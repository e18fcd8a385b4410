"""Annotated DPs on the bonus-aware strips against g2g_forward_kernel (NO_STRIP_BONUS=1): configs[0]'s DP alone and a batch of
16 annotated _pf DPs (the largest _pf golden with the synthetic annotation of tests/intronlib.py), and annotated _nv DPs on
g2g_v8_ntv{2,3}_ib: 16 x the largest _nv golden (115 x 221 nt, Noll 3) and 16 x a three-strip division of four synthetic
members (154 x 156 aa, Noll 2; tests/intron_nvlib.py); median of five runs each way (forward-kernel ms, HIP events) with the
five times and the paths, one JSON line.  Needs the GPU.

    python3 tools/intron_timing.py [out.json]"""
import json, os, sys, statistics
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import intronlib as il
import intron_nvlib as nv
from prrn_aln_amd import _abi, engine

def med(ctx, hs):
    b = ctx.prepare(hs)
    b.run()                                  # warm-up
    t = []
    for _ in range(5):
        b.run(); t.append(b.times_ms()[0])
    p = b.paths(); b.free()
    return statistics.median(t), t, sorted(set(p))

out = {}
ce = [_abi.problem_from_arrays(dict(np.load(os.path.join(il.GOLD, "intron_ce13a1_ce13a2.npz"))))]
big = il.annotate(il.load("prot16x100_ls3_k6"))           # the largest _pf golden (182 x 204 cells, Noll 3)
grp = [_abi.problem_from_arrays(big) for _ in range(16)]
nvd = nv.annotate(il.load(nv.NV[0][0]), nv.NV[0][4])      # the largest _nv golden (115 x 221 cells in a band of 245, Noll 3)
nvg = [_abi.problem_from_arrays(nvd) for _ in range(16)]
nv3 = [nv.three_strips(False)] * 16                        # three strips of 64 rows, Noll 2
for tag, opts in (("strips", {}), ("v1", {"NO_STRIP_BONUS": "1"})):
    c = engine.Context(options=opts)
    out["configs0_dp_" + tag] = med(c, ce)
    out["pf_batch16_" + tag] = med(c, grp)
    out["nv_batch16_" + tag] = med(c, nvg)
    out["nv3strip_batch16_" + tag] = med(c, nv3)
    c.close()
print(json.dumps(out))
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
