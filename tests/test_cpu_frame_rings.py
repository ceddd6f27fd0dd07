"""The host-side bookkeeping of the C API's frame path (csrc/dsm_frame_rings.h: the slot ring of a handle's uploads and enqueue
calls, param_chunk, group_size, map_upper_after, tail_may_be_large) on the host: tests/frame_rings_host.cpp is a stand-alone
program that holds the ring to a model that keeps the whole history -- a consumer is never sent to an older event than the
newest upload it has to wait for, never to none, and no event is lost or held twice -- and the arithmetic to its cases.  It
includes the header without HIP.  It runs as built plainly and, where g++ links their runtimes, as built with the address and
undefined-behaviour sanitizers."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "frame_rings_host.cpp")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _build_and_run(exe, extra):
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror"] + extra + [SRC, "-o", exe], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.strip() == "frame_rings_host: ok"


def test_frame_rings(tmp_path):
    from densesurfelmapping_amd import build
    assert "dsm_frame_rings.h" in build.HEADERS
    _build_and_run(str(tmp_path / "frame_rings_host"), [])
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run(["g++"] + SANITIZE + [str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode == 0:
        _build_and_run(str(tmp_path / "frame_rings_host_san"), SANITIZE)
