"""The vocabulary of the voxel-grid calls (csrc/dsm_grid_shape.h: GridDims, grid_dims_ok, ScratchPlan, capped, launch_blocks) on the
host: tests/grid_shape_host.cpp is a stand-alone program that holds them to row lengths on both sides of a word and of a wave, to
shapes at both voxel limits and past 32 bits, to the scratch offsets of dsm_grid_compose and of the field layout written out by
hand, and to the launch caps on both sides.  It includes the header without HIP, and runs a second time under the address and
undefined-behaviour sanitizers as an executable of its own."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [("-O1",), ("-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")], ids=["plain", "sanitizers"])
def test_grid_shape_vocabulary(tmp_path, flags):
    from densesurfelmapping_amd import build
    assert "dsm_grid_shape.h" in build.HEADERS
    exe = str(tmp_path / "grid_shape_host")
    subprocess.run(["g++", "-std=c++17", "-g", "-Wall", "-Werror", *flags, os.path.join(ROOT, "tests", "grid_shape_host.cpp"), "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip() == "grid_shape_host: ok"
