"""The host-side planning of a batch (prrn_aln_amd/csrc/g2g_plan.h) without a GPU -- of a run: the variant table, the CU shares,
the launch list, the text of a time-out report; of prepare: the kernel of a DP (choose), the shape of a batch (shape), its tile
queues, flag image and LDS plans (queues).  tests/host/plan_main.cc runs a fixed list of cases, built with g++ under ASan + UBSan,
and its output is compared with tests/golden/host_plan/*.txt.

The expectation files were written by the same program compiled against the blocks of g2g_batch_run / batch_prepare_impl as they
stood before they moved into g2g_plan.h (the slot arithmetic, the apportionment block, the four launch loops with the launches
recorded instead of made, the report formatter; for the three prepare sections choose_kernel, v2_lds_bytes, v3_layout, v3_need,
the tile-width block and build_queues with g2g_opt a lookup in the case's options and the HIP copies recorded), so they pin that
behaviour, not the header's."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_plan")


@pytest.fixture(scope="module")
def plan_main(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_plan") / "plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "prrn_aln_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "plan_main.cc")])
    return exe


@pytest.mark.parametrize("what", ["slots", "shares", "launches", "report", "choose", "shape", "queues"])
def test_plan_matches_recorded_behaviour(plan_main, what):
    p = subprocess.run([plan_main, what], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == "", p.stderr            # (a sanitizer report goes to stderr)
    want = open(os.path.join(GOLDEN, what + ".txt")).read()
    got_lines, want_lines = p.stdout.split("\n"), want.split("\n")
    for k, (g, w) in enumerate(zip(got_lines, want_lines)):
        assert g == w, "line %d of %s" % (k + 1, what)
    assert len(got_lines) == len(want_lines)


def test_table_names_every_kernel_the_engine_launches():
    """The typed kernel pointers live in g2g_engine.hip, in one array indexed by slot: slot by slot it must name the kernel the
    table names (and nothing for the six holes)."""
    import re
    eng = open(os.path.join(ROOT, "prrn_aln_amd", "csrc", "g2g_engine.hip")).read()
    body = eng[eng.index("G2G_KERNEL[G2G_NVAR] = {"):]
    body = body[:body.index("};")]
    kernels = re.findall(r"K[2367]\((\w+)\)", body)
    hdr = open(os.path.join(ROOT, "prrn_aln_amd", "csrc", "g2g_plan.h")).read()
    tab = hdr[hdr.index("G2G_VARIANT[G2G_NVAR] = {"):]
    tab = tab[:tab.index("};")]
    names = re.findall(r'\{"(\w*)",', tab)
    assert len(kernels) == 32 and len(names) == 32
    assert [k if k != "0" else "" for k in kernels] == names
