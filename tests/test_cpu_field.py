"""The distance field's definition on the host (no GPU): the brute-force checker of tests/field_host.cpp -- the minimum of
csrc/dsm_math.h's field_key over the set voxels within R -- against an independent numpy restatement, its two forms against each
other, the distance table, the inflation as the field's level sets, the declarations, and a sanitizer build of the checker as a
program of its own.  Every comparison is bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import field_cases as fc
import grid_cases as gc

ROOT = fc.ROOT


# ------------------------------------------------------------------ 1. the checker against numpy
def test_checker_against_numpy():
    cases = [c for c in fc.case_list() if c[0][0] * c[0][1] * c[0][2] <= fc.NUMPY_MAX_VOXELS]
    assert {c[0] for c in cases} == {g for g in fc.GRIDS if g[0] * g[1] * g[2] <= fc.NUMPY_MAX_VOXELS} and len(cases) > 500
    assert {c[2] for c in cases if c[0] == (37, 21, 13)} == set(fc.RADII)
    memo = {}
    for g, name, r in cases:
        vox = fc.sets(g)[name]
        exp = fc.expected(g, name, r)
        key = (g, vox.tobytes(), r)  # (the eight corners of a one-voxel grid are one set)
        if key not in memo:
            memo[key] = fc.np_field(vox, r)
        d2, near = memo[key]
        assert np.array_equal(exp["dist2"], d2) and np.array_equal(exp["nearest"], near), (g, name, r)
        # what the definition says of every result
        have = near >= 0
        assert ((exp["dist2"] == fc.FAR) == ~have).all() and (exp["dist2"][have] <= r * r).all()
        assert (exp["dist2"][vox] == 0).all() and np.array_equal(near[vox], np.flatnonzero(vox.ravel()))
        assert vox.ravel()[near[have]].all(), (g, name, r)
        table = fc.host_table(fc.VOXEL, r)
        assert np.array_equal(exp["distance"].view(np.uint32), table[np.where(have, exp["dist2"], r * r)].view(np.uint32))


def test_ties_and_truncation_by_hand():
    g = (37, 21, 13)
    mid = (18, 10, 6)
    lin = lambda x, y, z: (z * g[1] + y) * g[0] + x
    for a, name in enumerate("xyz"):
        lo = list(mid)
        lo[a] -= 1
        e = fc.expected(g, "tie along " + name, 3)
        assert e["dist2"][mid[2], mid[1], mid[0]] == 1 and e["nearest"][mid[2], mid[1], mid[0]] == lin(*lo)
    e = fc.expected(g, "tie diagonal", 3)
    assert e["dist2"][6, 10, 18] == 3 and e["nearest"][6, 10, 18] == lin(17, 9, 5)
    e = fc.expected(g, "tie across y and x", 3)  # -dy with +dx against +dy with -dx: the lower row wins although its x is higher
    assert e["dist2"][6, 10, 18] == 2 and e["nearest"][6, 10, 18] == lin(19, 9, 6)
    # 64 is inside the truncation, 65 is not
    for g, a in (((300, 5, 3), 0), ((5, 300, 3), 1), ((3, 5, 300), 2)):
        name = "129 apart along " + "xyz"[a]
        mid = [n // 2 for n in g]

        def at(p, e):
            q = list(mid)
            q[a] = p
            return int(e["dist2"][q[2], q[1], q[0]]), int(e["nearest"][q[2], q[1], q[0]])

        def lin_of(p):
            q = list(mid)
            q[a] = p
            return (q[2] * g[1] + q[1]) * g[0] + q[0]

        e = fc.expected(g, name, 64)
        assert at(69, e) == (4096, lin_of(5)) and at(70, e) == (4096, lin_of(134)) and at(198, e) == (4096, lin_of(134)) and at(199, e) == (fc.FAR, -1)
        e = fc.expected(g, name, 63)
        assert at(69, e) == (fc.FAR, -1) and at(70, e) == (fc.FAR, -1) and at(68, e) == (63 * 63, lin_of(5)) and at(197, e) == (63 * 63, lin_of(134))


def test_both_forms_and_pad_bits():
    rng = np.random.default_rng(4)
    for g in ((33, 3, 2), (65, 4, 3), (37, 21, 13)):
        for name in ("random 0.05", "random 0.5", "corner 7", "empty"):
            bits = gc.pack(fc.sets(g)[name])
            for r in (1, 3, 16):
                a, b = fc.host_field(bits, g[0], r, form=1), fc.host_field(bits, g[0], r, form=2)
                fc.same_fields(a, b, (g, name, r, "list vs window"))
                fc.same_fields(fc.host_field(fc.dirty_pads(bits, g[0], rng), g[0], r), a, (g, name, r, "pad bits"))


# ------------------------------------------------------------------ 2. the table
def test_distance_table():
    from densesurfelmapping_amd import api
    k = np.arange(4097, dtype=np.float64)
    for voxel in (0.1, 0.25, 1.0):
        want = (np.float64(np.float32(voxel)) * np.sqrt(k)).astype(np.float32)
        got = fc.host_table(voxel, 64)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), voxel
        assert np.array_equal(api.field_distance_table(voxel, 64).view(np.uint32), want.view(np.uint32))
        assert np.array_equal(api.field_distance_table(voxel, 3).view(np.uint32), want[:10].view(np.uint32))
        for kk in (0, 1, 2, 4095, 4096):
            assert got[kk] == np.float32(np.float64(np.float32(voxel)) * np.sqrt(np.float64(kk)))


# ------------------------------------------------------------------ 3. the inflation is the field's level sets
def test_inflation_is_a_level_set():
    for name, vox in gc.inflate_sets():
        nz, ny, nx = vox.shape
        bits = gc.pack(vox)
        d2 = fc.host_field(bits, nx, 16)["dist2"]
        for r in gc.INFLATE_RADII:
            level = d2 <= r * r
            if not name.startswith("single") or r in (0, 1, 3, 16):
                assert np.array_equal(level, gc.np_inflate(vox, r)), (name, r)
            assert np.array_equal(gc.pack(level), gc.host_inflate(bits, nx, r)), (name, r)


# ------------------------------------------------------------------ 4. the sanitizers
def test_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "field_host_main")
    r = fc.build_main(exe)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(6)
    files = []
    for k, (g, name, radius) in enumerate((((1, 1, 1), "full", 64), ((2, 3, 4), "random 0.5", 3), ((33, 3, 2), "random 0.05", 64), ((65, 4, 3), "random 0.5", 16),
                                           ((37, 21, 13), "random 0.05", 16), ((37, 21, 13), "tie diagonal", 63), ((300, 5, 3), "129 apart along x", 64),
                                           ((3, 5, 300), "64 and 65 apart along z", 64), ((5, 300, 3), "empty", 1))):
        path = str(tmp_path / ("case%d.bin" % k))
        fc.write_case(path, fc.dirty_pads(gc.pack(fc.sets(g)[name]), g[0], rng), g[0], radius)
        files.append(path)
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "field_host: list == window" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


# ------------------------------------------------------------------ 5. declarations
def test_field_abi_declarations(tmp_path):
    from densesurfelmapping_amd import api, build, surfel_map
    build.build_library()
    lib = C.CDLL(api.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "dsm.h")).read()
    node_hdr = open(os.path.join(ROOT, "include", "dsm_surfel_map.h")).read()
    for name in ("dsm_grid_distance", "dsm_field_compose"):
        assert name in api.ABI_SYMBOLS and name + "(" in hdr and hasattr(lib, name), name
    for name in ("dsm_surfel_map_field", "dsm_surfel_map_field_device"):
        assert name in surfel_map.ABI_SYMBOLS and name + "(" in node_hdr and hasattr(lib, name), name
    assert re.search(r"#define DSM_ABI_VERSION 4\b", hdr)
    lib.dsm_abi_version.restype = C.c_int
    assert lib.dsm_abi_version() == 4
    assert re.search(r"#define DSM_FIELD_MAX_DIST 64\b", hdr) and api.FIELD_MAX_DIST == 64 == fc.MAX_DIST
    assert re.search(r"#define DSM_FIELD_FAR 65535u", hdr) and api.FIELD_FAR == 65535 == fc.FAR
    assert "typedef struct dsm_field_planes" in hdr
    assert [f[0] for f in api._FieldPlanes._fields_] == ["dist2", "nearest", "distance"] == list(api.FIELD_PLANES) == list(fc.PLANES)
    assert C.sizeof(api._FieldPlanes) == 3 * C.sizeof(C.c_void_p) and C.sizeof(api._GridSpec) == 36
    assert [f[0] for f in api._GridPlanes._fields_] == ["occupied", "inflated", "index", "cells", "cells_cap"]
    for k in fc.PLANES:
        assert api.FIELD_PLANE_TYPES[k] == fc.TYPES[k]
    # the layout the compiler gives the struct, and the headers as plain C
    src = tmp_path / "field_abi.c"
    src.write_text('''#include <stddef.h>
#include "dsm.h"
#include "dsm_surfel_map.h"
typedef char planes_size[sizeof(dsm_field_planes) == 3 * sizeof(void *) ? 1 : -1];
typedef char planes_dist2[offsetof(dsm_field_planes, dist2) == 0 ? 1 : -1];
typedef char planes_nearest[offsetof(dsm_field_planes, nearest) == sizeof(void *) ? 1 : -1];
typedef char planes_distance[offsetof(dsm_field_planes, distance) == 2 * sizeof(void *) ? 1 : -1];
typedef char spec_size[sizeof(dsm_grid_spec) == 36 ? 1 : -1];
typedef char far_fits[DSM_FIELD_FAR == 65535u && DSM_FIELD_MAX_DIST * DSM_FIELD_MAX_DIST < DSM_FIELD_FAR ? 1 : -1];
int use(dsm_handle *h, dsm_surfel_map *m, const uint32_t *bits, uint16_t *d2, int32_t *nearest, float *metres) {
    dsm_grid_spec spec;
    dsm_field_planes planes = {0, 0, 0};
    int32_t n = 0;
    dsm_grid_spec_init(&spec);
    planes.dist2 = d2;
    planes.nearest = nearest;
    planes.distance = metres;
    return dsm_grid_distance(h, 64, 64, 32, DSM_FIELD_MAX_DIST, 0.1f, bits, &planes)
         + dsm_field_compose(h, DSM_CLOUD_SELECT_MATURE, 0, 0, 0, &spec, 16, 0, &planes, 0, &n)
         + dsm_surfel_map_field(m, DSM_CLOUD_ALL, &spec, 16, 0, &planes, &n) + dsm_surfel_map_field_device(m, DSM_CLOUD_ALL, &spec, 16, 0, &planes, &n);
}
''')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # without a handle every call is refused before anything else
    lib.dsm_grid_distance.argtypes = [C.c_void_p] + [C.c_int32] * 4 + [C.c_float, C.c_void_p, C.c_void_p]
    assert lib.dsm_grid_distance(None, 1, 1, 1, 1, 0.1, None, None) == api.DSM_E_INVALID
    lib.dsm_field_compose.argtypes = [C.c_void_p, C.c_int, C.c_int32] + [C.c_void_p] * 3 + [C.c_int32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p]
    assert lib.dsm_field_compose(None, 1, 0, None, None, None, 16, 0, None, 0, None) == api.DSM_E_INVALID
    for name in ("dsm_surfel_map_field", "dsm_surfel_map_field_device"):
        fn = getattr(lib, name)
        fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p]
        assert fn(None, 2, None, 16, 0, None, None) == api.DSM_E_INVALID
    hpp = open(os.path.join(ROOT, "include", "dsm_surfel_map.hpp")).read()
    assert "dsm_surfel_map_field(" in hpp and "dsm_surfel_map_field_device(" in hpp
    assert "dsm_surfel_map_field.cpp" in build.SOURCES and "dsm_k_field.h" in build.HEADERS
