"""Free space and the three-state map on the host (no GPU): the brute-force checker of tests/space_host.cpp -- csrc/dsm_carve.h's
carve_voxel over every voxel and frame, and a neighbour-by-neighbour classification -- against an independent numpy restatement, a
census of carve_voxel's exits on a crafted case, frontiers placed by hand, pad bits, the OR semantics, the declarations, and a
sanitizer build of the checker as a program of its own.  Every comparison is bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import grid_cases as gc
import space_cases as sc

ROOT = sc.ROOT


# ------------------------------------------------------------------ 1. the checker against numpy
def test_carve_checker_against_numpy():
    cases = sc.case_list()
    assert len(cases) == len(sc.GRIDS) * len(sc.CAMS) * len(sc.POSES)
    freed = {}
    for g, cam, kind in cases:
        s, frames = sc.case(g, cam, kind)
        bits, n = sc.expected(g, cam, kind)
        _, _, exits = sc.host_carve(s, frames, exits=True)
        want, want_exits = sc.np_carve(s, frames)
        assert np.array_equal(exits, want_exits), (g, cam, kind, np.argwhere(exits != want_exits)[:3])
        assert np.array_equal(bits, gc.pack(want)) and n == int(want.sum()), (g, cam, kind)
        freed[(g, cam, kind)] = n
        # the flag changes the voxels behind +inf pixels and nothing else
        t = sc.with_flags(s, sc.TRUST_INFINITE)
        bits_t, n_t, exits_t = sc.host_carve(t, frames, exits=True)
        want_t, want_exits_t = sc.np_carve(t, frames)
        assert np.array_equal(exits_t, want_exits_t) and np.array_equal(bits_t, gc.pack(want_t)), (g, cam, kind, "trust infinite")
        assert np.array_equal(exits_t != exits, exits == sc.EXITS.index("infinite"))
    # the cases free something where they should, and nothing where the camera looks away
    for (g, cam, kind), n in freed.items():
        assert n == 0 if kind == "away" else n > 0 or g == (1, 1, 1), (g, cam, kind, n)
    assert all(freed[((37, 21, 13), cam, kind)] > 200 for cam in sc.CAMS for kind in sc.POSES if kind != "away"), freed
    # the caller's inverse is taken bit for bit: with the closed form the set differs somewhere on the larger grids
    differs = 0
    for g in sc.GRIDS[1:]:
        for cam in sc.CAMS:
            s, frames = sc.case(g, cam, "own inverse")
            closed = sc.host_carve(s, [(frames[0][0], None, frames[0][2])])[0]
            differs += int((closed != sc.expected(g, cam, "own inverse")[0]).any())
    print("own inverse: the set differs from the closed form's on", differs, "of", 2 * (len(sc.GRIDS) - 1), "cases")


def test_classify_checker_against_numpy():
    rng = np.random.default_rng(3)
    for g in sc.CLASSIFY_GRIDS:
        for name, (occ, fre) in sc.classify_sets(g).items():
            got = sc.host_classify(gc.pack(occ), gc.pack(fre), g[0])
            state, kf, fr = sc.np_classify(occ, fre)
            assert np.array_equal(got["state"], state), (g, name)
            assert np.array_equal(got["known_free"], gc.pack(kf)) and np.array_equal(got["frontier"], gc.pack(fr)), (g, name)
            assert np.array_equal(got["cells"], np.flatnonzero(fr.ravel())) and got["n_frontier"] == int(fr.sum()), (g, name)
            if name in ("all free", "full", "empty"):
                assert got["n_frontier"] == 0, (g, name)
            # 4. dirty pad bits change nothing, and the outputs have them 0
            dirty = sc.host_classify(sc.dirty_pads(gc.pack(occ), g[0], rng), sc.dirty_pads(gc.pack(fre), g[0], rng), g[0])
            for k in ("state", "known_free", "frontier", "cells"):
                assert np.array_equal(dirty[k], got[k]), (g, name, k, "pad bits")
            assert not (got["known_free"][..., -1] & gc.pad_mask(g[0])).any() and not (got["frontier"][..., -1] & gc.pad_mask(g[0])).any()
        big = sc.classify_sets(g)["sparse free"]
        assert g == (1, 1, 1) or sc.host_classify(gc.pack(big[0]), gc.pack(big[1]), g[0])["n_frontier"] > 0
    # the cap cuts the list and nothing else
    occ, fre = sc.classify_sets((37, 21, 13))["sparse free"]
    full = sc.host_classify(gc.pack(occ), gc.pack(fre), 37)
    cut = sc.host_classify(gc.pack(occ), gc.pack(fre), 37, cap=10)
    assert cut["n_frontier"] == full["n_frontier"] > 10 and np.array_equal(cut["cells"], full["cells"][:10])


# ------------------------------------------------------------------ 2. the census
def test_census_of_every_exit():
    s, frames, marks = sc.census_case()
    cam = sc.CAM_64
    bits, n, exits = sc.host_carve(s, frames, exits=True)
    want, want_exits = sc.np_carve(s, frames)
    assert np.array_equal(exits, want_exits) and np.array_equal(bits, gc.pack(want))
    E = {name: k for k, name in enumerate(sc.EXITS)}
    e0 = exits[0]
    qz, u, v = sc.host_project(s, sc.closed_form_inverse(frames[0][0]))
    plane = frames[0][2]
    assert set(np.unique(e0)) == set(range(6)), np.unique(e0)  # every exit, in one frame of one grid
    # Range on both sides
    assert ((e0 == E["range"]) & (qz <= np.float32(s.near_d))).any() and ((e0 == E["range"]) & (qz >= np.float32(s.far_d))).any()
    # Outside on all four image edges
    out = e0 == E["outside"]
    assert (out & (u < 0)).any() and (out & (u >= cam.w)).any() and (out & (v < 0)).any() and (out & (v >= cam.h)).any()
    assert not (out & (u >= 0) & (u < cam.w) & (v >= 0) & (v < cam.h)).any()
    # NoDepth for 0, a negative and a NaN; Infinite
    d = plane[np.clip(v, 0, cam.h - 1), np.clip(u, 0, cam.w - 1)]
    nod = e0 == E["nodepth"]
    assert (nod & (d == 0)).any() and (nod & (d < 0)).any() and (nod & np.isnan(d)).any()
    inf = e0 == E["infinite"]
    assert inf.any() and np.isposinf(d[inf]).all()
    # ... and with the flag the same voxels are free
    exits_t = sc.host_carve(sc.with_flags(s, sc.TRUST_INFINITE), frames, exits=True)[2]
    assert (exits_t[0][inf] == E["free"]).all() and not (exits_t[0] == E["infinite"]).any()
    assert (e0 == E["notinfront"]).any() and (e0 == E["free"]).any()
    # q.z + margin the float just below, equal to, just above d
    edge = lambda m: np.float32(qz[marks[m][1:]] + np.float32(s.margin))
    px = lambda m: plane[int(v[marks[m][1:]]), int(u[marks[m][1:]])]
    assert px("margin below") == np.nextafter(edge("margin below"), np.float32(np.inf)) and e0[marks["margin below"][1:]] == E["free"]
    assert px("margin equal") == edge("margin equal") and e0[marks["margin equal"][1:]] == E["notinfront"]
    assert px("margin above") == np.nextafter(edge("margin above"), np.float32(-np.inf)) and e0[marks["margin above"][1:]] == E["notinfront"]
    # a projection on both sides of a .5 pixel boundary: inverses one float apart, pixels one apart, different exits
    below, above = sc.inverses_of(frames)[1], sc.inverses_of(frames)[2]
    assert (below != above).sum() == 1 and np.nextafter(below[12], np.float32(1)) == above[12]
    i = marks["half below"][1:]
    assert marks["half above"][1:] == i
    u_b, u_a = sc.host_project(s, below)[1][i], sc.host_project(s, above)[1][i]
    assert u_a == u_b + 1
    (_, ub64, _), (_, ua64, _) = sc.np_project(s, below), sc.np_project(s, above)
    assert ub64[i] < u_a <= ua64[i] and ua64[i] - ub64[i] < 1e-4  # u + 0.5 crosses the integer between the two
    assert exits[1][i] == E["free"] and exits[2][i] == E["nodepth"]


# ------------------------------------------------------------------ 3. frontiers by hand
def test_frontier_by_hand():
    cases = sc.by_hand()
    assert len(cases) == 8
    for name, g, occ, fre, frontier in cases:
        got = sc.host_classify(gc.pack(sc.voxels(g, occ)), gc.pack(sc.voxels(g, fre)), g[0])
        want = sc.voxels(g, frontier)
        assert np.array_equal(gc.unpack(got["frontier"], g[0]), want), name
        assert np.array_equal(got["cells"], np.flatnonzero(want.ravel())) and got["n_frontier"] == len(frontier), name
        assert np.array_equal(sc.np_classify(sc.voxels(g, occ), sc.voxels(g, fre))[2], want), name
        state = got["state"]
        for x, y, z in occ:
            assert state[z, y, x] == sc.OCCUPIED
        for x, y, z in fre:
            assert state[z, y, x] == (sc.OCCUPIED if (x, y, z) in occ else sc.FREE)
        assert int((state == sc.UNKNOWN).sum()) == g[0] * g[1] * g[2] - len(set(occ) | set(fre)), name
    # occupied wins over free
    g = (5, 4, 3)
    both = sc.host_classify(gc.pack(sc.voxels(g, [(2, 2, 1)])), gc.pack(sc.voxels(g, [(2, 2, 1), (3, 2, 1)])), 5)
    assert both["state"][1, 2, 2] == sc.OCCUPIED and both["state"][1, 2, 3] == sc.FREE and not gc.unpack(both["known_free"], 5)[1, 2, 2]


# ------------------------------------------------------------------ 5. OR semantics
def test_or_semantics_on_the_host():
    rng = np.random.default_rng(11)
    for g, cam_name in (((37, 21, 13), "64x48"), ((65, 4, 3), "70x44"), ((130, 9, 5), "70x44")):
        cam = sc.CAMS[cam_name]
        s = sc.make(g, cam)
        a, b = sc.many_frames(cam, 2, seed=40)
        old = gc.pack(rng.random(g[::-1]) < 0.02)
        ab = sc.host_carve(s, [b], sc.host_carve(s, [a], old)[0])
        ba = sc.host_carve(s, [a], sc.host_carve(s, [b], old)[0])
        both = sc.host_carve(s, [a, b], old)
        assert np.array_equal(ab[0], ba[0]) and np.array_equal(ab[0], both[0]) and ab[1] == ba[1] == both[1] == int(gc.unpack(both[0], g[0]).sum())
        assert not (old & ~both[0]).any()  # the old contents are kept
        only_a, only_b = sc.host_carve(s, [a])[0], sc.host_carve(s, [b])[0]
        assert np.array_equal(both[0], old | only_a | only_b)
        assert (only_a & ~only_b).any() and (only_b & ~only_a).any()  # (each frame sees something the other does not)
        replaced = sc.host_carve(sc.with_flags(s, sc.REPLACE), [b], both[0])
        assert np.array_equal(replaced[0], only_b) and (replaced[0] != both[0]).any()
        # dirty pad bits in the old set are written 0
        if g[0] % 32:
            dirty = sc.dirty_pads(old, g[0], rng)
            assert (dirty != old).any() and np.array_equal(sc.host_carve(s, [a, b], dirty)[0], both[0])
        want, _ = sc.np_carve(s, [a, b], old)
        assert np.array_equal(both[0], gc.pack(want))


# ------------------------------------------------------------------ 7. the sanitizers
def test_host_program_under_sanitizers(tmp_path):
    exe = str(tmp_path / "space_host_main")
    r = sc.build_main(exe)
    assert r.returncode == 0, r.stderr[-3000:]
    rng = np.random.default_rng(6)
    files = []

    def add(s, frames):
        path = str(tmp_path / ("case%d.bin" % len(files)))
        g = (s.nx, s.ny, s.nz)
        old = sc.dirty_pads(gc.pack(rng.random(g[::-1]) < 0.05), g[0], rng)
        occ = sc.dirty_pads(gc.pack(rng.random(g[::-1]) < 0.2), g[0], rng)
        sc.write_case(path, s, sc.inverses_of(frames), np.stack([f[2] for f in frames]), old, occ)
        files.append(path)

    for g, cam, kind in (((1, 1, 1), "64x48", "identity"), ((33, 3, 2), "70x44", "oblique"), ((65, 4, 3), "70x44", "inside"), ((37, 21, 13), "64x48", "own inverse"),
                         ((130, 9, 5), "70x44", "away")):
        add(*sc.case(g, cam, kind))
    s, frames, _ = sc.census_case()
    add(s, frames)
    add(sc.with_flags(s, sc.TRUST_INFINITE | sc.REPLACE), frames)
    add(sc.make((65, 4, 3), sc.CAM_70), sc.many_frames(sc.CAM_70, 32))
    r = subprocess.run([exe] + files, capture_output=True, text=True, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "space_host: consistent" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert r.stdout.count("frames of") == len(files)


# ------------------------------------------------------------------ 6. declarations
def test_space_abi_declarations(tmp_path):
    from densesurfelmapping_amd import api, build, surfel_map
    build.build_library()
    lib = C.CDLL(api.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "dsm.h")).read()
    node_hdr = open(os.path.join(ROOT, "include", "dsm_surfel_map.h")).read()
    facade = open(os.path.join(ROOT, "include", "dsm_surfel_map.hpp")).read()
    for name in ("dsm_carve_params_init", "dsm_grid_carve", "dsm_grid_classify"):
        assert name in api.ABI_SYMBOLS and name + "(" in hdr and hasattr(lib, name), name
    node_names = ("dsm_surfel_map_set_free_space", "dsm_surfel_map_free_space_resets", "dsm_surfel_map_free_space", "dsm_surfel_map_free_space_device",
                  "dsm_surfel_map_space", "dsm_surfel_map_space_device", "dsm_surfel_map_carve_last")
    for name in node_names:
        assert name in surfel_map.ABI_SYMBOLS and name + "(" in node_hdr and hasattr(lib, name) and name + "(" in facade, name
    assert re.search(r"#define DSM_ABI_VERSION 4\b", hdr)
    lib.dsm_abi_version.restype = C.c_int
    assert lib.dsm_abi_version() == 4
    assert re.search(r"#define DSM_CARVE_MAX_FRAMES 32\b", hdr) and api.CARVE_MAX_FRAMES == 32 == sc.MAX_FRAMES
    assert re.search(r"#define DSM_CARVE_REPLACE 1u", hdr) and api.CARVE_REPLACE == 1 == sc.REPLACE
    assert re.search(r"#define DSM_CARVE_TRUST_INFINITE 2u", hdr) and api.CARVE_TRUST_INFINITE == 2 == sc.TRUST_INFINITE
    assert (api.SPACE_UNKNOWN, api.SPACE_FREE, api.SPACE_OCCUPIED) == (0, 1, 2) == (sc.UNKNOWN, sc.FREE, sc.OCCUPIED)
    for k, name in enumerate(("UNKNOWN", "FREE", "OCCUPIED")):
        assert re.search(r"#define DSM_SPACE_%s %d\b" % (name, k), hdr)
    assert [f[0] for f in api._CarveParams._fields_] == ["struct_size", "near_dist", "far_dist", "margin"] and C.sizeof(api._CarveParams) == 16
    assert [f[0] for f in api._SpacePlanes._fields_] == ["state", "known_free", "frontier", "cells", "cells_cap"] == list(api.SPACE_PLANES) + ["cells_cap"]
    assert C.sizeof(api._SpacePlanes) == 5 * C.sizeof(C.c_void_p) and C.sizeof(api._GridSpec) == 36
    # the defaults: 0.1 m .. 10 m, one voxel diagonal of a 0.1 m grid
    p = api.carve_params()
    assert p.struct_size == 16 and p.near_dist == np.float32(0.1) and p.far_dist == 10.0 and abs(p.margin - 0.1 * 3 ** 0.5) < 1e-6
    assert api.carve_params(margin=0.5).margin == 0.5
    # the layout the compiler gives the structs, and the headers as plain C
    src = tmp_path / "space_abi.c"
    src.write_text('''#include <stddef.h>
#include "dsm.h"
#include "dsm_surfel_map.h"
typedef char params_size[sizeof(dsm_carve_params) == 16 ? 1 : -1];
typedef char params_near[offsetof(dsm_carve_params, near_dist) == 4 ? 1 : -1];
typedef char params_far[offsetof(dsm_carve_params, far_dist) == 8 ? 1 : -1];
typedef char params_margin[offsetof(dsm_carve_params, margin) == 12 ? 1 : -1];
typedef char planes_size[sizeof(dsm_space_planes) == 5 * sizeof(void *) ? 1 : -1];
typedef char planes_state[offsetof(dsm_space_planes, state) == 0 ? 1 : -1];
typedef char planes_known[offsetof(dsm_space_planes, known_free) == sizeof(void *) ? 1 : -1];
typedef char planes_frontier[offsetof(dsm_space_planes, frontier) == 2 * sizeof(void *) ? 1 : -1];
typedef char planes_cells[offsetof(dsm_space_planes, cells) == 3 * sizeof(void *) ? 1 : -1];
typedef char planes_cap[offsetof(dsm_space_planes, cells_cap) == 4 * sizeof(void *) ? 1 : -1];
typedef char spec_size[sizeof(dsm_grid_spec) == 36 ? 1 : -1];
typedef char states[DSM_SPACE_UNKNOWN == 0 && DSM_SPACE_FREE == 1 && DSM_SPACE_OCCUPIED == 2 && DSM_CARVE_MAX_FRAMES == 32 ? 1 : -1];
int use(dsm_handle *h, dsm_surfel_map *m, void *free_set, const void *occupied, uint8_t *state) {
    dsm_grid_spec spec;
    dsm_carve_params params;
    dsm_space_planes planes = {0, 0, 0, 0, 0};
    const int32_t slot = 0;
    const float pose[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    int64_t n_free = 0;
    int32_t n = 0, n_frontier = 0;
    int rc;
    dsm_grid_spec_init(&spec);
    dsm_carve_params_init(&params);
    planes.state = state;
    rc = dsm_grid_carve(h, &spec, &params, DSM_CARVE_REPLACE | DSM_CARVE_TRUST_INFINITE, 1, &slot, pose, 0, free_set, &n_free);
    rc |= dsm_grid_classify(h, spec.nx, spec.ny, spec.nz, occupied, free_set, &planes, &n_frontier);
    rc |= dsm_surfel_map_set_free_space(m, &spec, &params, 0);
    rc |= dsm_surfel_map_free_space(m, (uint32_t *)free_set, &n_free) | dsm_surfel_map_free_space_device(m, free_set, &n_free);
    rc |= dsm_surfel_map_space(m, DSM_CLOUD_ALL, &planes, &n, &n_frontier) | dsm_surfel_map_space_device(m, DSM_CLOUD_ALL, &planes, &n, &n_frontier);
    rc |= dsm_surfel_map_carve_last(m, &spec, &params, 0, free_set);
    return rc + (int)dsm_surfel_map_free_space_resets(m);
}
''')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o", str(tmp_path / "space_abi.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    # every call refused with a NULL handle, before anything else is looked at
    lib.dsm_grid_carve.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_int32] + [C.c_void_p] * 5
    lib.dsm_grid_classify.argtypes = [C.c_void_p] + [C.c_int32] * 3 + [C.c_void_p] * 4
    spec, params, planes = api.grid_spec(), api.carve_params(), api._SpacePlanes()
    word, n64, n32 = C.c_uint32(0), C.c_int64(-7), C.c_int32(-7)
    slot, pose = C.c_int32(0), (C.c_float * 16)(*np.eye(4, dtype=np.float32).ravel())
    planes.known_free = C.addressof(word)
    assert lib.dsm_grid_carve(None, C.byref(spec), C.byref(params), 0, 1, C.byref(slot), pose, None, C.byref(word), C.byref(n64)) == api.DSM_E_INVALID
    assert lib.dsm_grid_classify(None, 1, 1, 1, C.byref(word), C.byref(word), C.byref(planes), C.byref(n32)) == api.DSM_E_INVALID
    lib.dsm_carve_params_init(None)  # (a NULL is ignored, as dsm_grid_spec_init does)
    surfel_map._bind(lib)
    assert lib.dsm_surfel_map_set_free_space(None, C.byref(spec), C.byref(params), 0) == api.DSM_E_INVALID
    assert lib.dsm_surfel_map_free_space(None, C.byref(word), C.byref(n64)) == api.DSM_E_INVALID
    assert lib.dsm_surfel_map_free_space_device(None, C.byref(word), C.byref(n64)) == api.DSM_E_INVALID
    assert lib.dsm_surfel_map_space(None, 2, C.byref(planes), C.byref(n32), C.byref(n32)) == api.DSM_E_INVALID
    assert lib.dsm_surfel_map_space_device(None, 2, C.byref(planes), C.byref(n32), C.byref(n32)) == api.DSM_E_INVALID
    assert lib.dsm_surfel_map_carve_last(None, C.byref(spec), C.byref(params), 0, C.byref(word)) == api.DSM_E_INVALID
    assert lib.dsm_surfel_map_free_space_resets(None) == 0
    assert word.value == 0 and n64.value == -7 and n32.value == -7
    assert "dsm_surfel_map_space.cpp" in build.SOURCES and "dsm_k_carve.h" in build.HEADERS and "dsm_carve.h" in build.HEADERS
    # msglog's options
    mlog = open(os.path.join(ROOT, "densesurfelmapping_amd", "msglog.py")).read()
    for opt in ("--save-space", "--carve-near", "--carve-far", "--carve-margin"):
        assert '"%s"' % opt in mlog, opt
