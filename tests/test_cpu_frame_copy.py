"""The plane-copy plan of every frame upload (csrc/dsm_frame_copy.h) on the host: tests/frame_copy_host.cpp carries each plan
out with memcpy between buffers of exactly the extents the geometry implies and checks ranges, payload and untouched gaps; this
module enumerates the geometries and holds the plan's shape -- transfers, 1-D / 2-D, packed, resulting strides -- against the
three rules written out below."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_lib = None


def host_lib():
    global _lib
    if _lib is None:
        out = os.path.join(ROOT, "tests", "_build", "libframe_copy_host.so")
        src = os.path.join(ROOT, "tests", "frame_copy_host.cpp")
        deps = [src, os.path.join(ROOT, "densesurfelmapping_amd", "csrc", "dsm_frame_copy.h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-shared", "-fPIC", src, "-o", out + ".tmp"], check=True)
            os.replace(out + ".tmp", out)
        lib = C.CDLL(out)
        lib.frame_copy_host_run.argtypes = [C.c_int] + [C.c_size_t] * 6 + [C.c_int, C.POINTER(C.c_int64)]
        lib.frame_copy_host_run.restype = C.c_int
        _lib = lib
    return _lib


def rule(n, rows, row_bytes, step, frame_step, dst_step, dst_frame_step, pack_tight):
    """-> (rule, transfers, two_d, packed, out_step, out_frame_step): the table, first match wins"""
    if step == dst_step and (n == 1 or frame_step == dst_frame_step):
        return 1, 1, False, False, dst_step, dst_frame_step  # laid out like the destination: one piece
    if pack_tight and step == row_bytes and (n == 1 or frame_step == row_bytes * rows):
        return 2, 1, False, True, row_bytes, row_bytes * rows  # tight, and the reader takes tight: one piece, packed
    if step == dst_step:
        return 3, n, False, False, dst_step, dst_frame_step  # frame by frame, each in one piece
    return 3, n, True, False, dst_step, dst_frame_step  # frame by frame, row by row


def geometries(w):
    for elem, rows, n, pack_tight in itertools.product((1, 2, 3, 4), (1, 2, 19), (1, 2, 5), (False, True)):
        row_bytes, dst_step = w * elem, (w + 63) // 64 * 64 * elem
        dst_frame_step = dst_step * rows
        for step in (dst_step, row_bytes, row_bytes + 1, dst_step + elem):
            for frame_step in (step * rows, dst_frame_step, step * rows + 3):
                yield n, rows, row_bytes, step, frame_step, dst_step, dst_frame_step, pack_tight


@pytest.mark.parametrize("w", [1, 25, 64, 250])
def test_every_plan_inside_exact_buffers(w):
    lib = host_lib()
    out = (C.c_int64 * 5)()
    seen = set()
    for g in geometries(w):
        line = lib.frame_copy_host_run(*g[:7], int(g[7]), out)
        assert line == 0, f"frame_copy_host.cpp:{line} failed for n, rows, row_bytes, step, frame_step, dst_step, dst_frame_step, pack_tight = {g}"
        want = rule(*g)
        assert (out[0], bool(out[1]), bool(out[2]), out[3], out[4]) == want[1:], (g, list(out), want)
        seen.add((want[0], want[1] > 1, want[2]))
    # the enumeration reaches every shape a plan can have: (rule, more than one transfer, 2-D)
    assert seen >= {(1, False, False), (3, True, False), (3, True, True), (3, False, True)}
    assert ((2, False, False) in seen) == (w != 64), "w == 64 makes rules 1 and 2 coincide: rule 1 must win"
