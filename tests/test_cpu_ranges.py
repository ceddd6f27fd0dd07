"""The overlap predicates the C API puts to a caller's planes (csrc/dsm_ranges.h: ranges_overlap, planes_distinct) on the host:
tests/ranges_host.cpp is a stand-alone program that holds them to adjacent ranges, one shared byte, containment, ranges of no
bytes and ranges that end at the top of the address space.  It includes the header without HIP."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_overlap_predicates(tmp_path):
    from densesurfelmapping_amd import build
    assert "dsm_ranges.h" in build.HEADERS
    exe = str(tmp_path / "ranges_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "ranges_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip() == "ranges_host: ok"
