"""The LDS plan of the v6 (`_pf`, one lane per cell) launches without a GPU (prrn_aln_amd/csrc/g2g_plan.h: v6_ring_need, v6_layout):
tests/host/v6_layout_main.cc, built with g++ under ASan + UBSan like tests/host/plan_main.cc, checks

  need     on synthetic offset tables (dense, sparse, one huge list, lists only at the right edge, the longest list in the last
           column, b shorter than the window, no lists at all) and several column ranges of each: the need of a view equals the
           most entries any V6_WINDOW consecutive columns hold, counted entry by entry; it covers what the kernel's feed schedule
           keeps alive at any refill of any strip (lane 63's column through min(n0 + V6_AHEAD, right - 1); the window keeps four
           columns more than the schedule, so this is <=, not ==); a ring is the need rounded up to 32 entries (32 at least), the
           tail a multiple of 4 above the longest list;
  layout   the regions of a plan are 16-byte aligned, disjoint, and `total` is their end;
  bench16  the recorded facts of the bench sweep's 16 balanced divisions (rows_bytes 26 032, ca4 8-16, s needs 165-191, t needs
           470-725, longest list 11-14) give plans of at most 40 960 B, four strips per CU -- one by one and as one launch."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def layout_main(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("host_v6_layout") / "v6_layout_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "prrn_aln_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "host", "v6_layout_main.cc")])
    return exe


@pytest.mark.parametrize("what", ["need", "layout", "bench16"])
def test_v6_plan(layout_main, what):
    p = subprocess.run([layout_main, what], capture_output=True, text=True)
    assert p.stderr == "", p.stderr                                  # (a sanitizer report goes to stderr)
    assert p.returncode == 0 and "FAIL" not in p.stdout, "\n".join(l for l in p.stdout.split("\n") if l.startswith("FAIL"))
    assert len(p.stdout.split("\n")) > 5


def test_bench16_totals_are_the_recorded_ones(layout_main):
    """37 152 - 40 288 B per division, 40 320 B for the launch that holds them all (ca4 16 from one division, the 736-entry t ring
    from another)."""
    out = subprocess.run([layout_main, "bench16"], capture_output=True, text=True, check=True).stdout.split("\n")
    tot = [int(l.split()[-1]) for l in out if l.startswith("division")]
    assert len(tot) == 16 and min(tot) == 37152 and max(tot) == 40288
    assert [l for l in out if l.startswith("launch")] == ["launch: rings 192 736 tail 16 total 40320"]
