"""Connected components of a bit set without a GPU: the host checker of tests/components_host.cpp against a plain Python
restatement of the definition of include/dsm.h, its two forms against each other as a program under the sanitizers, the rule for
the voxel of a world point, the ABI surface of the new calls, and a census showing that every case of tests/components_cases.py
reaches what it is built for (tests/test_gpu_components.py runs the same list against the kernels)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import components_cases as cc
import grid_cases as gc

ROOT = cc.ROOT


def _same_as_numpy(vox, conn, what):
    nx = vox.shape[2]
    label, stats = cc.np_components(vox, conn)
    for form in (0, 1):
        res = cc.host_components(gc.pack(vox), nx, conn, form=form)
        assert np.array_equal(res["label"], label), (what, conn, form)
        assert res["n"] == res["n_all"] == len(stats), (what, conn, form)
        t = res["table"]
        assert list(t["root"]) == sorted(stats), (what, conn, form)
        for e in t:
            count, sums, lo, hi = stats[int(e["root"])]
            assert (int(e["count"]), tuple(e["sum"]), tuple(e["lo"]), tuple(e["hi"])) == (count, sums, lo, hi), (what, conn, form, e)
            assert e["tag"] == 0 and e["reserved"] == 0


GRIDS = ((1, 1, 1), (2, 3, 4), (20, 9, 7), (7, 9, 20), (33, 3, 2), (1, 17, 3))


@pytest.mark.parametrize("g", GRIDS, ids=["%dx%dx%d" % g for g in GRIDS])
def test_checker_against_numpy_on_random_sets(g):
    rng = np.random.default_rng(g[0] + 10 * g[1] + 100 * g[2])
    for density in (0.0, 0.05, 0.2, 0.31, 0.5, 1.0):
        vox = rng.random(g[::-1]) < density
        for conn in (cc.FACES, cc.ALL):
            _same_as_numpy(vox, conn, (g, density))


def test_checker_against_numpy_on_hand_placed_sets():
    g = (20, 9, 7)
    for offset in [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]:
        vox = np.zeros(g[::-1], bool)
        vox[3, 4, 10] = vox[3 + offset[2], 4 + offset[1], 10 + offset[0]] = True
        for conn in (cc.FACES, cc.ALL):
            _same_as_numpy(vox, conn, offset)
            joined = sum(abs(o) for o in offset) == 1 or conn == cc.ALL
            assert cc.host_components(gc.pack(vox), g[0], conn)["n_all"] == (1 if joined else 2), (offset, conn)
    # opposite borders do not touch: nothing outside the grid connects anything
    vox = np.zeros(g[::-1], bool)
    vox[:, :, 0] = vox[:, :, -1] = True
    assert cc.host_components(gc.pack(vox), g[0], cc.ALL)["n_all"] == 2
    # a ring, a spiral staircase and a filter
    vox = np.zeros(g[::-1], bool)
    vox[1, 2:7, 2:9] = True
    vox[1, 3:6, 3:8] = False
    for k in range(6):
        vox[k, 8, 12 + k] = True
    for conn in (cc.FACES, cc.ALL):
        _same_as_numpy(vox, conn, "ring and stairs")
    res = cc.host_components(gc.pack(vox), g[0], cc.FACES, min_count=2)
    assert res["n_all"] == 7 and res["n"] == 1 and res["table"]["count"][0] == 20


def test_tags_and_pad_bits_in_the_checker():
    rng = np.random.default_rng(3)
    vox = rng.random((3, 5, 33)) < 0.3
    tags = rng.integers(-2**31, 2**31, vox.shape, dtype=np.int64).astype(np.int32)
    res = cc.host_components(gc.pack(vox), 33, cc.ALL, tags=tags)
    assert np.array_equal(res["table"]["tag"], tags.ravel()[res["table"]["root"]])
    dirty = gc.pack(vox)
    dirty[..., -1] |= gc.pad_mask(33)
    again = cc.host_components(dirty, 33, cc.ALL, tags=tags)
    assert np.array_equal(again["label"], res["label"]) and again["table"].tobytes() == res["table"].tobytes()


def test_two_forms_agree_as_a_sanitized_program(tmp_path):
    """every case at its CPU size, every connectivity and min_count it is run with"""
    exe = os.path.join(ROOT, "tests", "_build", "components_host_main")
    built = cc.build_main(exe)
    assert built.returncode == 0, built.stderr
    files = []
    rng = np.random.default_rng(17)
    for c in cc.cases():
        vox = c.vox(True)
        for conn in c.conns:
            for mc in c.min_counts:
                path = str(tmp_path / ("case%03d.bin" % len(files)))
                tags = rng.integers(-5, 5, vox.shape).astype(np.int32) if len(files) % 3 == 0 else None
                cc.write_case(path, vox, conn, mc, tags)
                files.append(path)
    run = subprocess.run([exe] + files, capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout, run.stderr)
    assert run.stdout.strip() == "components_host: %d cases, the flood fill and the union-find agree" % len(files), run.stdout
    assert "runtime error" not in run.stderr and "Sanitizer" not in run.stderr, run.stderr


def test_abi_surface():
    from densesurfelmapping_amd import api, build, surfel_map
    build.build_library()
    lib = C.CDLL(api.LIB_PATH)
    for name in ("dsm_grid_components", "dsm_frontier_query_init", "dsm_surfel_map_frontier_clusters", "dsm_surfel_map_frontier_clusters_device"):
        assert hasattr(lib, name), name
    assert "dsm_grid_components" in api.ABI_SYMBOLS and "dsm_surfel_map_frontier_clusters" in surfel_map.ABI_SYMBOLS
    assert cc.layout() == [64, 0, 4, 8, 32, 44, 56, 60]
    for dt in (api.COMPONENT_DTYPE, cc.COMPONENT):
        assert dt.itemsize == 64
        assert [dt.fields[k][1] for k in ("root", "count", "sum", "lo", "hi", "tag", "reserved")] == [0, 4, 8, 32, 44, 56, 60]
    header = open(os.path.join(ROOT, "include", "dsm.h")).read()
    assert re.search(r"#define DSM_ABI_VERSION (\d+)", header).group(1) == "4"
    lib.dsm_abi_version.restype = C.c_int
    assert lib.dsm_abi_version() == 4
    assert (api.CONNECT_FACES, api.CONNECT_ALL) == (cc.FACES, cc.ALL) == tuple(int(v) for v in re.findall(r"#define DSM_CONNECT_\w+ (\d+)", header))
    q = surfel_map._FrontierQuery()
    surfel_map._bind(lib).dsm_frontier_query_init(C.byref(q))
    assert (q.struct_size, q.connectivity, q.min_count, q.has_from) == (C.sizeof(q), 26, 1, 0) and C.sizeof(q) == 28


def test_from_voxel_rule_at_a_lattice_plane():
    origin, voxel = (-1.5, 0.25, 10.0), 0.1
    # the plane between voxel 6 and voxel 7 of axis 0, as the rule itself places it: the smallest float whose quotient reaches 7
    def index(x):
        return int(np.floor((np.float64(np.float32(x)) - np.float64(np.float32(origin[0]))) / np.float64(np.float32(voxel))))
    on = np.float32(origin[0] + 7 * voxel)
    while index(np.nextafter(on, np.float32(-np.inf))) >= 7:
        on = np.nextafter(on, np.float32(-np.inf))
    while index(on) < 7:
        on = np.nextafter(on, np.float32(np.inf))
    below, above = np.nextafter(on, np.float32(-np.inf)), np.nextafter(on, np.float32(np.inf))
    assert cc.from_voxel((below, 0.25, 10.0), origin, voxel)[0] == 6
    assert cc.from_voxel((on, 0.25, 10.0), origin, voxel)[0] == 7
    assert cc.from_voxel((above, 0.25, 10.0), origin, voxel)[0] == 7
    # exactly on the origin: voxel 0 on every axis; just below it: -1 (floor, not truncation)
    assert cc.from_voxel(origin, origin, voxel) == (0, 0, 0)
    assert cc.from_voxel((np.nextafter(np.float32(-1.5), np.float32(-2)), 0.2, 9.99), origin, voxel) == (-1, -1, -1)
    # a negative coordinate well inside a grid with a negative origin, and a binary-exact voxel on a plane
    assert cc.from_voxel((-0.75, -3.0, -0.26), (-2.0, -4.0, -1.0), 0.25) == (5, 4, 2)
    assert cc.from_voxel((-1.0, -3.75, -0.5), (-2.0, -4.0, -1.0), 0.25) == (4, 1, 2)
    # far outside and not a number: clamped, outside every grid
    assert cc.from_voxel((1e30, -1e30, np.nan), (0, 0, 0), 0.1) == (2**31 - 1, -2**31, -2**31)


def test_census_of_the_cases():
    """each case reaches what it is built for, on the checker's output at the size the GPU runs (the two largest at their CPU size)"""
    k = cc.kernel_constants()
    assert {"kCompTileX", "kCompTileY", "kCompTileZ", "kCompBlockWords"} <= set(k)
    g = cc.SEAM_GRID
    assert all(g[a] > 64 and g[a] % 2 ** s for a in range(3) for s in (3, 5, 6))
    bounds = cc.seam_boundaries()
    assert bounds[0] == [32, 64, 128] and all(len(bounds[a]) >= 1 for a in (1, 2))
    for kind in ("face", "edge", "corner"):
        pairs = cc.seam_pairs(kind)
        for axis in range(3):
            for b in bounds[axis]:
                assert any(p[axis] == b - 1 and q[axis] == b for p, q in pairs), (kind, axis, b)
        for p, q in pairs:
            d = sorted(abs(p[a] - q[a]) for a in range(3))
            assert d == {"face": [0, 0, 1], "edge": [0, 1, 1], "corner": [1, 1, 1]}[kind]
        for conn in (cc.FACES, cc.ALL):
            n = cc.expected("seam %s pairs" % kind, conn)["n_all"]
            assert n == (len(pairs) if kind == "face" or conn == cc.ALL else 2 * len(pairs)), (kind, conn, n)
    for conn in (cc.FACES, cc.ALL):
        mid = cc.expected("percolation %d at %g" % (conn, cc.PERCOLATION[conn][1]), conn)
        assert cc.spans(mid, g), conn
        lo, hi = (cc.expected("percolation %d at %g" % (conn, d), conn) for d in (cc.PERCOLATION[conn][0], cc.PERCOLATION[conn][2]))
        assert lo["table"]["count"].max() < mid["table"]["count"].max() < hi["table"]["count"].max()
        assert lo["n_all"] > 1000 and hi["n_all"] > 100
    for name in ("serpentine", "serpentine mirrored"):
        v = cc.case(name).vox()
        assert v.shape == (3, 9, 66) and v[0, 0, 0] and v[2, 8, 65]
        e = cc.expected(name, cc.FACES)
        assert e["n_all"] == 1 and e["table"]["root"][0] == 0 and e["table"]["count"][0] == v.sum()
        assert tuple(e["table"]["lo"][0]) == (0, 0, 0) and tuple(e["table"]["hi"][0]) == (65, 8, 2)
    # the serpentine is a chain: without any one of its joints it falls apart
    v = np.array(cc.case("serpentine").vox())
    for z, y, x in ((1, 0, 65), (2, 1, 0), (1, 8, 0), (0, 7, 0)):
        assert v[z, y, x]
        v[z, y, x] = False
        assert cc.host_components(gc.pack(v), 66, cc.FACES)["n_all"] == 2
        v[z, y, x] = True
    u = np.array(cc.case("u shape").vox())
    assert cc.expected("u shape", cc.FACES)["n_all"] == 1
    u[0, 11, 30] = False
    assert cc.host_components(gc.pack(u), 70, cc.ALL)["n_all"] == 2
    assert cc.expected("empty", cc.ALL)["n_all"] == 0 and (cc.expected("empty", cc.ALL)["label"] == -1).all()
    assert cc.expected("all set 33x5x3", cc.FACES)["table"]["count"][0] == 33 * 5 * 3
    assert cc.expected("one voxel", cc.FACES)["n_all"] == 1
    assert cc.case("nx 1").vox().shape[2] == 1 and cc.expected("nx 1", cc.FACES)["n_all"] > 10
    assert cc.expected("checkerboard 34x6x4", cc.FACES)["n_all"] == 34 * 6 * 4 // 2 and cc.expected("checkerboard 34x6x4", cc.ALL)["n_all"] == 1
    assert 2 * sum(range(2000)) * 2000 > 2 ** 32  # sum[1] of the one component of 2 x 2000 x 2000
    small = cc.expected("all set 2x2000x2000", cc.FACES, cpu=True)
    assert small["n_all"] == 1 and small["table"]["sum"][0][1] == 2 * sum(range(40)) * 40
    words = 1500 * 1500  # of the large checkerboard (one word a row): more 256-word tiles than one trip of the count and scatter kernels takes
    assert (words + k["kCompBlockWords"] - 1) // k["kCompBlockWords"] > 8192 and words == 2_250_000
    board = cc.expected("checkerboard 2x1500x1500", cc.FACES, 2, cpu=True)
    assert board["n_all"] == 2 * 30 * 30 // 2 and board["n"] == 0
    sizes = cc.case("sizes 1 to 6")
    for mc, kept in ((1, 6), (3, 4), (6, 1), (7, 0)):
        for conn in sizes.conns:
            e = cc.expected(sizes.name, conn, mc)
            assert e["n_all"] == 6 and e["n"] == kept and sorted(e["table"]["count"]) == list(range(mc, 7)), (mc, conn)
            assert list(e["table"]["root"]) == sorted(e["table"]["root"])
