"""Viewpoint gain on the host (no GPU): the brute-force checker of tests/view_host.cpp -- csrc/dsm_view.h over every pose, voxel and
interior point, the line by the closed form with an explicit floor division -- against an independent numpy restatement; the
kernel's integer error terms (ViewWalk) against the formula; the census of the crafted calls; pad bits; the declarations; and a
sanitizer build of the checker as a program of its own.  Every comparison is bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import grid_cases as gc
import space_cases as sc
import view_cases as vc

ROOT = vc.ROOT
SMALL_CALLS = ("70x33x19/3", "130x3x2/3", "1x1x1/3")  # what the numpy restatement walks in a few seconds


# ------------------------------------------------------------------ 1. the checker against numpy
def test_checker_against_numpy():
    for name in SMALL_CALLS:
        s, poses, occ, fre, tgt = vc.call(name)
        for flags in (0, vc.UNKNOWN_BLOCKS):
            t = vc.with_flags(s, flags)
            got = vc.host_view(t, poses, occ, fre, tgt, detail=True)
            want = vc.np_view(t, poses, occ, fre, tgt)
            assert np.array_equal(got["exits"], want["exits"]), (name, flags, np.argwhere(got["exits"] != want["exits"])[:3])
            for k in vc.LINE_DTYPE.names:
                assert np.array_equal(got["lines"][k], want["lines"][k]), (name, flags, k)
            assert np.array_equal(got["scores"], want["scores"]), (name, flags, got["scores"], want["scores"])
            assert np.array_equal(got["visible"], vc.pack_planes(want["visible"])), (name, flags)
            # the shared, cached result is the same thing without the detail
            exp = vc.expected(name, flags)
            assert np.array_equal(exp["scores"], got["scores"]) and np.array_equal(exp["visible"], got["visible"]) and exp["steps"] == got["steps"]
            sco = got["scores"]
            assert (sco["unknown"] + sco["free"] + sco["occupied"] == sco["visible"]).all() and (sco["visible"] <= sco["in_view"]).all()
            assert (sco["target"] <= sco["visible"]).all() and not sco["reserved"].any()
            # without a target the count is 0 and nothing else moves
            bare = vc.host_view(t, poses, occ, fre, None)
            assert not bare["scores"]["target"].any() and np.array_equal(bare["visible"], got["visible"])
            assert all(np.array_equal(bare["scores"][k], sco[k]) for k in ("in_view", "visible", "unknown", "free", "occupied"))
        assert vc.expected(name)["scores"]["visible"].sum() > 0 or name.startswith("1x1x1")
    # the blocking flag only ever removes voxels
    for name in SMALL_CALLS[:2]:
        a, b = vc.expected(name, 0), vc.expected(name, vc.UNKNOWN_BLOCKS)
        assert not (b["visible"] & ~a["visible"]).any() and ((a["visible"] != b["visible"]).any() or name != SMALL_CALLS[0]), name


def test_pad_bits_are_ignored_and_written_zero():
    rng = np.random.default_rng(5)
    for name in ("70x33x19/3", "130x3x2/3"):
        s, poses, occ, fre, tgt = vc.call(name)
        pad = gc.pad_mask(s.nx)
        assert all((b[..., -1] & pad).any() for b in (occ, fre, tgt))  # (the shared sets carry garbage there)
        clean = [b.copy() for b in (occ, fre, tgt)]
        for b in clean:
            b[..., -1] &= ~pad
        exp = vc.expected(name)
        got = vc.host_view(s, poses, *clean)
        assert np.array_equal(got["scores"], exp["scores"]) and np.array_equal(got["visible"], exp["visible"])
        assert not (exp["visible"][..., -1] & pad).any()


# ------------------------------------------------------------------ 2. the line
def test_error_term_walk_equals_the_closed_form():
    """ViewWalk (what the kernel steps) against the formula restated in numpy, and the checker's own closed form against the same"""
    rng = np.random.default_rng(9)
    ends = [((0, 0, 0), (0, 0, 0)), ((0, 0, 0), (1, 0, 0)), ((0, 0, 0), (2, 1, 0)), ((0, 0, 0), (2, -1, 1)), ((5, 5, 5), (-2, 3, 4)), ((3, -7, 2), (3, 9, 2)),
            ((-vc.MAX_REACH, 1, 0), (129, 1, 1)), ((129 + vc.MAX_REACH, 2, 1), (0, 0, 0)), ((-4096, -4096, -4096), ((1 << 28) - 1, 0, 0)),
            (((1 << 28) + 4095, 4096, -4096), (0, 0, 0))]
    for _ in range(300):
        a = rng.integers(-60, 60, 3)
        ends.append((tuple(a), tuple(a + rng.integers(-40, 41, 3))))
    differ = 0
    for a, v in ends:
        a64, v64 = np.array(a, np.int64), np.array(v, np.int64)
        n = int(np.abs(v64 - a64).max())
        if n > 100000:  # the longest lines there can be: the first and the last thousand points, every step of the walk taken on the way
            for skip in (0, n - 1 - 1000):
                ks = np.arange(skip + 1, skip + 1001)
                want = vc.np_line_points(a64, (v64 - a64)[None, :].repeat(len(ks), 0), np.full(len(ks), n, np.int64), ks[:, None])
                assert np.array_equal(vc.host_walk(a, v, skip=skip, cap=1000), want) and np.array_equal(vc.host_walk(a, v, closed=True, skip=skip, cap=1000), want), (a, v)
            continue
        ks = np.arange(1, max(n, 1))
        want = vc.np_line_points(a64, (v64 - a64)[None, :].repeat(len(ks), 0), np.full(len(ks), n, np.int64), ks[:, None])
        walk, closed = vc.host_walk(a, v), vc.host_walk(a, v, closed=True)
        assert len(walk) == max(n - 1, 0) == len(closed)
        assert np.array_equal(walk, closed), (a, v)
        if n > 1:
            assert np.array_equal(closed, want), (a, v)
            # the same line from the other end, both ends excluded, 26-adjacent steps
            back = vc.host_walk(v, a)
            assert np.array_equal(back[::-1], walk), (a, v)
            steps = np.diff(np.concatenate([a64[None], walk, v64[None]]), axis=0)
            assert np.abs(steps).max() <= 1 and (np.abs(steps).max(-1) == 1).all()
            trunc = vc.np_line_points(a64, (v64 - a64)[None, :].repeat(len(ks), 0), np.full(len(ks), n, np.int64), ks[:, None], truncate=True)
            differ += int((trunc != want).any())
    assert differ > 100, differ  # (lines with negative components: truncation is another line)


# ------------------------------------------------------------------ 3. the census
def test_census():
    s, poses, occ, fre, tgt, marks = vc.census_call()
    res = vc.host_view(s, poses, occ, fre, tgt, detail=True)
    res_unknown = vc.host_view(vc.with_flags(s, vc.UNKNOWN_BLOCKS), poses, occ, fre, tgt, detail=True)
    want = vc.np_view(s, poses, occ, fre, tgt)
    assert np.array_equal(res["exits"], want["exits"]) and np.array_equal(res["scores"], want["scores"])
    census = vc.census(s, poses, occ, fre, tgt, marks, res, res_unknown, vc.np_view(s, poses, occ, fre, tgt, truncate=True))
    print("\n".join("%-70s %d" % kv for kv in census.items()))
    missing = [k for k, n in census.items() if n <= 0]
    assert not missing, missing
    assert len(census) == 8 + 3 + 1 + 3 + 6 + 1 + 1 + 4 + 1 + 4
    # the camera's voxel is occupied and in view, and it is seen: a voxel never blocks itself, the camera's never blocks
    cam = marks["camera"]
    assert (res["exits"][:6, cam[2], cam[1], cam[0]] == 0).all()
    # what stands behind the occupied neighbour along +y is blocked by it, at k = 1
    nb = marks["neighbour"]
    behind = res["lines"][2][cam[2], cam[1] + 2:cam[1] + 8, cam[0]]
    assert (res["exits"][2][cam[2], cam[1] + 2:cam[1] + 8, cam[0]] == 7).all() and (behind["k_first"] == 1).all() and nb == (cam[0], cam[1] + 1, cam[2])


def test_census_of_the_callers_inverse():
    """a caller's inverse one ulp from the closed form moves voxels across the far bound: the inverse is taken bit for bit"""
    s, pose, base, inv = vc.inverse_call()
    assert inv is not None, "no single-ulp change of the inverse moved a voxel across a bound"
    assert (inv != base).sum() == 1 and np.abs(inv.view(np.int32).astype(np.int64) - base.view(np.int32)).max() == 1
    occ, fre, tgt = vc.sets_of(s, 81)
    closed = vc.host_view(s, [pose], occ, fre, tgt, detail=True)
    own = vc.host_view(s, [pose], occ, fre, tgt, invs=[inv], detail=True)
    in_view = lambda r: (r["exits"] == 0) | (r["exits"] == 7)
    moved = in_view(closed) != in_view(own)
    print("voxels moved across a bound by the caller's inverse:", int(moved.sum()))
    assert moved.sum() > 0 and closed["scores"]["in_view"][0] != own["scores"]["in_view"][0]
    want = vc.np_view(s, [pose], occ, fre, tgt, invs=[inv])
    assert np.array_equal(own["exits"], want["exits"]) and np.array_equal(own["scores"], want["scores"])


# ------------------------------------------------------------------ 4. the camera's voxel and the reach
def test_camera_voxel_and_reach():
    for name in ("130x3x2/reach", "1x1x1/reach"):
        s, poses, occ, fre, tgt = vc.call(name)
        g = vc.dims(s)
        for k, pose in enumerate(poses):
            a, ok = vc.cam_voxel(s, pose)
            axis, high = divmod(k, 2)
            assert ok and a[axis] == (g[axis] + vc.MAX_REACH - 1 if high else -vc.MAX_REACH), (name, k, a)
        exp = vc.expected(name)
        assert exp["scores"]["in_view"].sum() > 0, name  # (the grid is in range and in the image from that far)
        for axis in range(3):
            for side in ("low-1", "high+1"):
                assert not vc.cam_voxel(s, vc.reach_pose(s, axis, side))[1]
    # the voxel is the floor of the quotient in double, negative coordinates included
    s = vc.make(vc.GRID_70, vc.CAM_40)
    for t in ((-0.01, 0.0, 1.6), (3.49, -1.651, 0.649), (-3.5, 1.65, 2.55), (-3.5001, 1.6501, 2.5501)):
        pose = vc.look((1, 0, 0), t)
        want = np.floor((pose[:3, 3].astype(np.float64) - np.array(s.origin[:], np.float64)) / np.float64(s.voxel))
        assert np.array_equal(vc.cam_voxel(s, pose)[0], want.astype(np.int32)), t


# ------------------------------------------------------------------ 5. the sanitizers
def test_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "view_host_main")
    r = vc.build_main(exe)
    assert r.returncode == 0, r.stderr[-3000:]
    files = []

    def add(s, poses, occ, fre, tgt, invs=None):
        path = str(tmp_path / ("case%d.bin" % len(files)))
        vc.write_case(path, s, poses, invs, occ, fre, tgt)
        files.append(path)

    s, poses, occ, fre, tgt, _ = vc.census_call()
    add(s, poses, occ, fre, tgt)
    add(vc.with_flags(s, vc.UNKNOWN_BLOCKS), poses, occ, fre, None)
    for name in ("130x3x2/3", "1x1x1/3", "130x3x2/reach", "1x1x1/reach"):
        s, poses, occ, fre, tgt = vc.call(name)
        add(s, poses, occ, fre, tgt)
    s, pose, base, inv = vc.inverse_call()
    add(s, [pose], *vc.sets_of(s, 81), invs=[inv])
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "view_host: consistent" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert r.stdout.count("line steps") == len(files)


# ------------------------------------------------------------------ 6. declarations
def test_view_abi_declarations(tmp_path):
    from densesurfelmapping_amd import api, build, surfel_map
    build.build_library()
    lib = C.CDLL(api.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "dsm.h")).read()
    node_hdr = open(os.path.join(ROOT, "include", "dsm_surfel_map.h")).read()
    facade = open(os.path.join(ROOT, "include", "dsm_surfel_map.hpp")).read()
    assert "dsm_grid_view" in api.ABI_SYMBOLS and "dsm_grid_view(" in hdr and hasattr(lib, "dsm_grid_view")
    for name in ("dsm_view_query_init", "dsm_surfel_map_view_gain", "dsm_surfel_map_view_gain_device"):
        assert name in surfel_map.ABI_SYMBOLS and name + "(" in node_hdr and hasattr(lib, name) and name + "(" in facade, name
    assert re.search(r"#define DSM_ABI_VERSION 4\b", hdr)
    assert re.search(r"#define DSM_VIEW_MAX_REACH 4096\b", hdr) and api.VIEW_MAX_REACH == 4096 == vc.MAX_REACH
    assert re.search(r"#define DSM_VIEW_MAX_POSES 4096\b", hdr) and api.VIEW_MAX_POSES == 4096 == vc.MAX_POSES
    assert re.search(r"#define DSM_VIEW_UNKNOWN_BLOCKS 1u", hdr) and api.VIEW_UNKNOWN_BLOCKS == 1 == vc.UNKNOWN_BLOCKS
    assert re.search(r"#define DSM_VIEW_TARGET_NONE 0\b", node_hdr) and re.search(r"#define DSM_VIEW_TARGET_FRONTIER 1\b", node_hdr)
    assert (api.VIEW_TARGET_NONE, api.VIEW_TARGET_FRONTIER) == (0, 1)
    assert api.VIEW_SCORE_DTYPE == vc.SCORE_DTYPE and api.VIEW_SCORE_DTYPE.itemsize == 32
    assert [f[0] for f in api._ViewQuery._fields_] == ["struct_size", "camera", "flags", "target"] and C.sizeof(api._ViewQuery) == 44
    assert "viewpoints or goal poses" not in hdr and "viewpoints or goal poses" not in node_hdr and "pose search" in hdr
    q = api.view_query(vc.CAM_40, target="none", flags=1)
    assert q.struct_size == 44 and q.camera.width == 40 and q.camera.fy == np.float32(26.25) and q.flags == 1 and q.target == 0
    assert api.view_query(vc.CAM_40).target == 1
    # the layout the compiler gives the structs, and the headers as plain C
    src = tmp_path / "view_abi.c"
    src.write_text('''#include <stddef.h>
#include "dsm.h"
#include "dsm_surfel_map.h"
typedef char score_size[sizeof(dsm_view_score) == 32 ? 1 : -1];
typedef char score_in_view[offsetof(dsm_view_score, in_view) == 0 ? 1 : -1];
typedef char score_visible[offsetof(dsm_view_score, visible) == 4 ? 1 : -1];
typedef char score_unknown[offsetof(dsm_view_score, unknown) == 8 ? 1 : -1];
typedef char score_free[offsetof(dsm_view_score, free) == 12 ? 1 : -1];
typedef char score_occupied[offsetof(dsm_view_score, occupied) == 16 ? 1 : -1];
typedef char score_target[offsetof(dsm_view_score, target) == 20 ? 1 : -1];
typedef char score_reserved[offsetof(dsm_view_score, reserved) == 24 ? 1 : -1];
typedef char query_size[sizeof(dsm_view_query) == 44 ? 1 : -1];
typedef char query_camera[offsetof(dsm_view_query, camera) == 4 ? 1 : -1];
typedef char query_flags[offsetof(dsm_view_query, flags) == 36 ? 1 : -1];
typedef char query_target[offsetof(dsm_view_query, target) == 40 ? 1 : -1];
typedef char limits[DSM_VIEW_MAX_REACH == 4096 && DSM_VIEW_MAX_POSES == 4096 && DSM_VIEW_UNKNOWN_BLOCKS == 1u ? 1 : -1];
int use(dsm_handle *h, dsm_surfel_map *m, const void *occupied, const void *free_set, uint32_t *visible) {
    dsm_grid_spec spec;
    dsm_view_query q;
    dsm_view_score score;
    const float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int rc;
    dsm_grid_spec_init(&spec);
    dsm_view_query_init(m, &q);
    rc = dsm_grid_view(h, &spec, &q.camera, DSM_VIEW_UNKNOWN_BLOCKS, 1, pose, 0, occupied, free_set, 0, &score, 0, visible);
    rc |= dsm_surfel_map_view_gain(m, DSM_CLOUD_ALL, &q, 1, pose, &score, visible);
    rc |= dsm_surfel_map_view_gain_device(m, DSM_CLOUD_ALL, &q, 1, pose, &score, visible);
    return rc + score.free;
}
''')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "view_abi.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # every call refused with a NULL handle, before anything else is looked at
    lib.dsm_grid_view.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    spec, cam = api.grid_spec(), api.render_camera(vc.CAM_40)
    word = C.c_uint32(0)
    score = (C.c_int32 * 8)(*([-7] * 8))
    pose = (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    assert lib.dsm_grid_view(None, C.byref(spec), C.byref(cam), 0, 1, pose, None, C.byref(word), C.byref(word), None, score, 0, None) == api.DSM_E_INVALID
    surfel_map._bind(lib)
    q = api.view_query(vc.CAM_40)
    assert lib.dsm_surfel_map_view_gain(None, 2, C.byref(q), 1, pose, score, None) == api.DSM_E_INVALID
    assert lib.dsm_surfel_map_view_gain_device(None, 2, C.byref(q), 1, pose, score, None) == api.DSM_E_INVALID
    lib.dsm_view_query_init(None, None)  # (a NULL query is ignored)
    q2 = api._ViewQuery()
    lib.dsm_view_query_init(None, C.byref(q2))  # (a NULL node: the camera is left for the caller)
    assert q2.struct_size == 44 and q2.target == 1 and q2.flags == 0 and q2.camera.width == 0
    assert word.value == 0 and list(score) == [-7] * 8
    assert "dsm_k_view.h" in build.HEADERS and "dsm_view.h" in build.HEADERS
    kernels = open(os.path.join(ROOT, "densesurfelmapping_amd", "csrc", "dsm_kernels.hip")).read()
    assert kernels.index('#include "dsm_k_carve.h"') < kernels.index('#include "dsm_k_view.h"')
    # msglog's options and its poses: the last pose turned about its own y axis, the first one unturned
    from densesurfelmapping_amd import msglog
    mlog = open(os.path.join(ROOT, "densesurfelmapping_amd", "msglog.py")).read()
    for opt in ("--save-view-gain", "--view-yaws"):
        assert '"%s"' % opt in mlog, opt
    base = sc.pose_at((0.3, -0.2, 1.1), yaw=0.4, pitch=0.1)
    turned = msglog.yaw_poses(base, 4)
    assert turned.shape == (4, 4, 4) and turned.dtype == np.float32 and np.array_equal(turned[0], base)
    assert np.allclose(turned[:, :3, 3], base[:3, 3]) and np.allclose(turned[:, :3, 1], base[:3, 1], atol=1e-6)  # (the y axis and the place stay)
    assert np.allclose(turned[2][:3, 2], -base[:3, 2], atol=1e-6) and np.allclose(turned[1][:3, 2], base[:3, 0], atol=1e-6)  # half a turn; a quarter: z -> x
