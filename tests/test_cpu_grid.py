"""The voxel grid's definition without a GPU: csrc/dsm_math.h's grid_setup / grid_covers / grid_centre through the host checker
tests/grid_host.cpp (which tests/test_gpu_grid.py compares the kernels with, bit for bit).
  1. boxed == brute: the voxel box loses no covered voxel, for crafted and for random records
  2. the checker against a numpy float64 restatement of the definition, on every (surfel, voxel) pair away from the margins
  3. the brute-force inflation against a numpy dilation; pad bits
  4. dsm_grid_spec_around
  5. grid_host.cpp's own main under the sanitizers
  6. the declarations"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import grid_cases as gc
import mesh_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


@pytest.fixture(scope="module")
def dtype():
    from densesurfelmapping_amd import api
    return api.SURFEL_DTYPE


# ------------------------------------------------------------------ 1. boxed == brute
@pytest.mark.parametrize("grid", list(gc.ALL_GRIDS), ids=list(gc.ALL_GRIDS))
def test_boxed_equals_brute_crafted(dtype, grid):
    s = gc.ALL_GRIDS[grid]
    m, names = gc.crafted_records(dtype, s)
    brute = gc.host_grid(m, s, brute=True)
    gc.same_grids(gc.host_grid(m, s, brute=False), brute, ("crafted", grid))
    pairs = gc.host_pairs(m, s)
    assert np.array_equal(np.where(pairs.any(0), pairs.argmax(0), -1).reshape(brute["index"].shape), brute["index"])  # the lowest number
    assert np.array_equal(gc.unpack(brute["occupied"], s.nx), brute["index"] >= 0)
    assert not (brute["occupied"][..., -1] & gc.pad_mask(s.nx)).any()
    covers = dict(zip(names, pairs.any(1)))
    for name in ("zero normal", "minus-zero normal", "NaN px", "+inf py", "-inf pz", "NaN size", "negative size", "-inf size", "nn overflows", "NaN normal",
                 "inf normal", "tiny normal: nn underflows to 0", "outside the low x face", "outside the high z face", "far outside, large",
                 "huge finite position", "huge finite position, huge size"):
        assert not covers[name], name
    if grid == "1x1x1":
        return
    for name in ("update_times 0", "update_times 4", "update_times 5", "zero size at a voxel centre", "inf size: the whole slab",
                 "huge size: (size + h)^2 overflows", "huge normal, nn finite", "tiny normal: nn a denormal", "normal of length 1e-3", "normal of length 40",
                 "plane on a cube face, normal along x", "plane on a cube face, normal along z", "centre on a voxel corner", "straddles the low y face",
                 "straddles the high x face", "just outside the high y face, reaching in", "through the whole grid", "wide along x", "duplicate a",
                 "duplicate b"):
        assert covers[name], name
    lo, hi, keep = gc.host_boxes(m, s)
    small, big = gc.tiers(lo, hi, keep)
    if grid in gc.MAIN_GRIDS:
        assert small.sum() >= 10 and big.sum() >= 3, (small.sum(), big.sum())
        assert big[names.index("through the whole grid")] and big[names.index("inf size: the whole slab")]
    assert (brute["index"] == names.index("duplicate a")).any() and not (brute["index"] == names.index("duplicate b")).any()


def test_face_and_corner_margins(dtype):
    """on the dyadic grid the crafted margins are exact: the plane on a cube face has e2 == ta in both neighbours, and a disc of
    radius h on a voxel corner with an axis normal covers the four voxels round the corner on either side of its plane (e2 == ta,
    in-plane distance sqrt(2) h <= 2 h) and none of the next ring (sqrt(10) h) -- eight"""
    s = gc.GRID_37
    m, names = gc.crafted_records(dtype, s)
    pairs = gc.host_pairs(m, s).reshape(len(m), s.nz, s.ny, s.nx)
    for a, f in enumerate(("x", "y", "z")):
        i = names.index("plane on a cube face, normal along " + f)
        r = m[i]
        c = gc.centres(s, a)
        p = f32(r[("px", "py", "pz")[a]])
        e = c - p
        on = np.flatnonzero(e * e == (f32(s.voxel) * f32(0.5)) ** 2)
        assert len(on) == 2 and on[1] == on[0] + 1, (f, on)
        cov = np.moveaxis(pairs[i], 2 - a, 0)  # the axis first
        assert cov[on[0]].any() and cov[on[1]].any() and not cov[:on[0]].any() and not cov[on[1] + 1:].any()
    i = names.index("centre on a voxel corner, axis normal")
    assert pairs[i].sum() == 8


def test_boxed_equals_brute_random(dtype):
    rng = np.random.default_rng(2025)
    for grid, s in gc.ALL_GRIDS.items():
        sets = (("random bits", mc.random_records(rng, 1500, dtype)), ("in and around the grid", gc.grid_records(rng, 1500, dtype, s)),
                ("large", gc.grid_records(rng, 300, dtype, s, sizes=(0.5, 30.0), scales=(1e-25, 1e-12, 1.0, 1e15))))
        for what, m in sets:
            brute = gc.host_grid(m, s, brute=True)
            gc.same_grids(gc.host_grid(m, s, brute=False), brute, (what, grid))
        assert (brute["index"] >= 0).any()


# ------------------------------------------------------------------ 2. the float64 restatement
@pytest.mark.parametrize("grid", list(gc.MAIN_GRIDS), ids=list(gc.MAIN_GRIDS))
def test_checker_against_float64(dtype, grid):
    s = gc.MAIN_GRIDS[grid]
    rng = np.random.default_rng(41)
    m = gc.grid_records(rng, 4000, dtype, s)
    covered, near, inside = gc.np_cover64(m, s)
    got = gc.host_pairs(m, s)
    frac = (near & inside).sum() / inside.sum()
    print("%s: %d pairs, %d inside, %d covered, %.3f %% of the inside ones near a margin" % (grid, covered.size, inside.sum(), covered.sum(), 100 * frac))
    assert covered.sum() > 1000 and inside.sum() >= covered.sum()
    assert frac <= 0.005  # the condition of the comparison, met by the restatement alone
    assert not (covered & ~inside).any()  # the exact bound |d_a| <= size + 3h
    bad = (got != covered) & ~near
    assert not bad.any(), (bad.sum(), np.argwhere(bad)[0])


# ------------------------------------------------------------------ 3. the inflation
def test_inflation_against_numpy():
    rng = np.random.default_rng(3)
    for name, vox in gc.inflate_sets():
        nz, ny, nx = vox.shape
        bits = gc.pack(vox)
        assert np.array_equal(gc.unpack(bits, nx), vox)
        dirty = bits.copy()
        dirty[..., -1] |= gc.pad_mask(nx) & rng.integers(0, 1 << 32, dirty[..., -1].shape, dtype=np.uint64).astype(np.uint32)
        radii = gc.INFLATE_RADII if not name.startswith("single") else (0, 1, 3, 16)
        for r in radii:
            got = gc.host_inflate(bits, nx, r)
            want = gc.np_inflate(vox, r)
            assert np.array_equal(gc.unpack(got, nx), want), (name, r)
            assert not (got[..., -1] & gc.pad_mask(nx)).any(), (name, r)
            assert np.array_equal(gc.host_inflate(dirty, nx, r), got), (name, r, "dirty pad bits")
            if r == 0:
                assert np.array_equal(got, bits)
            if name.startswith("single"):  # the ball itself, clipped
                z, y, x = np.argwhere(vox)[0]
                zz, yy, xx = np.ogrid[:nz, :ny, :nx]
                assert np.array_equal(want, (zz - z) ** 2 + (yy - y) ** 2 + (xx - x) ** 2 <= r * r), (name, r)
            cells = gc.host_cells(got, nx)
            assert np.array_equal(cells, np.flatnonzero(want.ravel())) and np.array_equal(gc.host_cells(dirty, nx), np.flatnonzero(vox.ravel()))


def test_inflate_width_table():
    """grid_inflate_width of csrc/dsm_math.h, which fills the kernel's table: floor(sqrt(r^2 - s)) in exact integers for every
    radius and every s = dy^2 + dz^2 inside it -- and the rows of the brute-force ball are that wide"""
    import math
    width = gc.host_lib().grid_host_inflate_width
    for r in range(17):
        for s in range(r * r + 1):
            assert width(r, s) == math.isqrt(r * r - s), (r, s)
        vox = np.zeros((2 * r + 1,) * 3, bool)
        vox[r, r, r] = True
        ball = gc.unpack(gc.host_inflate(gc.pack(vox), 2 * r + 1, r), 2 * r + 1)
        for dz in range(-r, r + 1):
            for dy in range(-r, r + 1):
                row = ball[r + dz, r + dy]
                if dy * dy + dz * dz <= r * r:
                    k = width(r, dy * dy + dz * dz)
                    assert row.sum() == 2 * k + 1 and row[r - k] and row[r + k], (r, dy, dz)
                else:
                    assert not row.any()


# ------------------------------------------------------------------ 4. dsm_grid_spec_around
def test_spec_around():
    from densesurfelmapping_amd import api, build
    build.build_library()
    g = api.grid_spec()
    assert (g.struct_size, g.voxel, g.nx, g.ny, g.nz, g.inflate) == (C.sizeof(api._GridSpec), f32(0.1), 1, 1, 1, 0) and list(g.origin) == [0, 0, 0]

    def want(c, v, n):  # the header's formula, in Python's doubles
        import math
        return f32(math.floor(float(f32(c)) / float(f32(v)) - n / 2.0) * float(f32(v)))

    for v in (0.1, 0.25, 0.2, 1.0):
        for dims in ((64, 64, 32), (37, 21, 13), (1, 1, 1), (2, 3, 4)):
            for c in ((0.0, 0.0, 0.0), (-3.37, 12.2, -0.01), (-1000.05, -0.0001, 250.7), (5 * v, -7 * v, 0.5 * v), (-v, v, 1e-9)):
                g = api.grid_spec_around(c, v, dims, inflate=3)
                assert (g.nx, g.ny, g.nz, g.inflate, g.struct_size) == dims + (3, C.sizeof(api._GridSpec)) and g.voxel == f32(v)
                for a in range(3):
                    assert g.origin[a] == want(c[a], v, dims[a]), (v, dims, c, a)
                    # the centre lies in the middle voxel (or on the face between the two middle ones)
                    i = (float(f32(c[a])) - float(g.origin[a])) / float(f32(v))
                    assert dims[a] / 2.0 - 1e-3 <= i <= dims[a] / 2.0 + 1 + 1e-3, (v, dims, c, a, i)
    # exact lattice points, odd and even dimensions, negative centres: dyadic voxel, so every product is exact
    for n, c, o in ((4, 0.0, -0.5), (5, 0.0, -0.75), (4, 0.25, -0.25), (5, 0.25, -0.5), (4, -0.25, -0.75), (5, -0.25, -1.0), (4, -0.3, -1.0), (5, -0.3, -1.0),
                    (1, -0.01, -0.25), (1, 0.0, -0.25), (2, -1024.0, -1024.25)):
        assert api.grid_spec_around((c, c, c), 0.25, (n, n, n)).origin[0] == f32(o), (n, c, o)
    # two centres one voxel apart: origins exactly one voxel apart -- one lattice
    for v in (0.25, 0.5, 2.0):
        for c in (-3.3, 0.0, 17.77, -1000.0):
            for n in (7, 8):
                a, b = api.grid_spec_around((c,) * 3, v, (n,) * 3), api.grid_spec_around((c + v,) * 3, v, (n,) * 3)
                assert b.origin[0] - a.origin[0] == f32(v), (v, c, n)
    for c in (-3.3, 0.04, 17.77):  # and for a voxel that is no dyadic number: one lattice to within the rounding of a float
        a, b = api.grid_spec_around((c,) * 3, 0.1, (8,) * 3), api.grid_spec_around((c + 0.1,) * 3, 0.1, (8,) * 3)
        k = round(float(a.origin[0]) / 0.1)
        assert abs(float(a.origin[0]) - k * 0.1) < 1e-5 and abs(float(b.origin[0]) - (k + 1) * 0.1) < 1e-5


# ------------------------------------------------------------------ 5. the stand-alone program under the sanitizers
def test_host_program_under_sanitizers(dtype, tmp_path):
    exe = str(tmp_path / "grid_host_main")
    r = gc.build_main(exe)
    assert r.returncode == 0, r.stderr[-3000:]
    files = []
    rng = np.random.default_rng(6)
    for k, (grid, s) in enumerate(gc.ALL_GRIDS.items()):
        m, names = gc.crafted_records(dtype, s)
        for name in ("inf size: the whole slab", "NaN px", "NaN size", "huge finite position", "huge finite position, huge size", "nn overflows"):
            assert name in names
        path = str(tmp_path / ("case%d.bin" % k))
        gc.write_case(path, gc.with_inflate(s, (2, 0, 16, 1, 5)[k]), np.concatenate([m, mc.random_records(rng, 500, dtype), gc.grid_records(rng, 500, dtype, s)]))
        files.append(path)
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "grid_host: boxed == brute" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


# ------------------------------------------------------------------ 6. declarations
def test_grid_abi_declarations(tmp_path):
    from densesurfelmapping_amd import api, build, surfel_map
    build.build_library()
    lib = C.CDLL(api.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "dsm.h")).read()
    node_hdr = open(os.path.join(ROOT, "include", "dsm_surfel_map.h")).read()
    for name in ("dsm_grid_spec_init", "dsm_grid_spec_around", "dsm_grid_compose", "dsm_grid_inflate"):
        assert name in api.ABI_SYMBOLS and name + "(" in hdr and hasattr(lib, name), name
    for name in ("dsm_surfel_map_grid", "dsm_surfel_map_grid_device"):
        assert name in surfel_map.ABI_SYMBOLS and name + "(" in node_hdr and hasattr(lib, name), name
    assert re.search(r"#define DSM_ABI_VERSION 4\b", hdr)
    lib.dsm_abi_version.restype = C.c_int
    assert lib.dsm_abi_version() == 4
    assert re.search(r"#define DSM_GRID_CELLS_OF_INFLATED 1u", hdr) and api.GRID_CELLS_OF_INFLATED == 1 == gc.CELLS_OF_INFLATED
    assert "typedef struct dsm_grid_spec" in hdr and "typedef struct dsm_grid_planes" in hdr
    assert C.sizeof(api._GridSpec) == 36 == C.sizeof(gc.Spec) and [f[0] for f in api._GridSpec._fields_] == [f[0] for f in gc.Spec._fields_]
    assert [f[0] for f in api._GridPlanes._fields_] == ["occupied", "inflated", "index", "cells", "cells_cap"]
    # the layouts the compiler gives the two structs, and the headers as plain C
    src = tmp_path / "grid_abi.c"
    src.write_text('''#include <stddef.h>
#include "dsm.h"
#include "dsm_surfel_map.h"
typedef char spec_size[sizeof(dsm_grid_spec) == 36 ? 1 : -1];
typedef char spec_inflate[offsetof(dsm_grid_spec, inflate) == 32 ? 1 : -1];
typedef char planes_cap[offsetof(dsm_grid_planes, cells_cap) == 4 * sizeof(void *) ? 1 : -1];
int use(dsm_handle *h, dsm_surfel_map *m, const float *centre, uint32_t *bits) {
    dsm_grid_spec spec;
    dsm_grid_planes planes = {0, 0, 0, 0, 0};
    int32_t n = 0, cells = 0;
    dsm_grid_spec_init(&spec);
    dsm_grid_spec_around(&spec, centre, 0.1f, 64, 64, 32);
    planes.occupied = bits;
    return dsm_grid_compose(h, DSM_CLOUD_SELECT_MATURE, 0, 0, 0, &spec, DSM_GRID_CELLS_OF_INFLATED, &planes, 0, &n, &cells)
         + dsm_grid_inflate(h, 64, 64, 32, 3, bits, bits) + dsm_surfel_map_grid(m, DSM_CLOUD_ALL, &spec, 0, &planes, &n, &cells)
         + dsm_surfel_map_grid_device(m, DSM_CLOUD_ALL, &spec, 0, &planes, &n, &cells);
}
''')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # without a handle every call is refused before anything else
    lib.dsm_grid_compose.argtypes = [C.c_void_p, C.c_int, C.c_int32] + [C.c_void_p] * 3 + [C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.dsm_grid_compose(None, 1, 0, None, None, None, 0, None, 0, None, None) == api.DSM_E_INVALID
    lib.dsm_grid_inflate.argtypes = [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p] * 2
    assert lib.dsm_grid_inflate(None, 1, 1, 1, 0, None, None) == api.DSM_E_INVALID
    lib.dsm_surfel_map_grid.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.dsm_surfel_map_grid(None, 2, None, 0, None, None, None) == api.DSM_E_INVALID
    hpp = open(os.path.join(ROOT, "include", "dsm_surfel_map.hpp")).read()
    assert "dsm_surfel_map_grid(" in hpp and "dsm_surfel_map_grid_device(" in hpp
    assert "dsm_surfel_map_grid.cpp" in build.SOURCES and "dsm_k_grid.h" in build.HEADERS
