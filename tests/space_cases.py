"""Shared by tests/test_cpu_space.py and tests/test_gpu_space.py: the host build of the definitions of free space and the
three-state map (tests/space_host.cpp: csrc/dsm_carve.h's carve_voxel by brute force over every voxel and frame, and a
neighbour-by-neighbour classification), an independent numpy restatement of both, the grids, cameras, poses and depth frames, ONE
list of carve cases with the checker's result computed once per case and handed out read-only, the crafted census case, and the
bit sets of the classification."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import grid_cases as gc
import render_cases as rc

ROOT = gc.ROOT
SRC = os.path.join(ROOT, "tests", "space_host.cpp")
CSRC = os.path.join(ROOT, "densesurfelmapping_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "dsm_math.h"), os.path.join(CSRC, "dsm_align.h"), os.path.join(CSRC, "dsm_carve.h"), os.path.join(ROOT, "include", "dsm.h")]
REPLACE, TRUST_INFINITE, MAX_FRAMES = 1, 2, 32  # DSM_CARVE_REPLACE, DSM_CARVE_TRUST_INFINITE, DSM_CARVE_MAX_FRAMES of include/dsm.h
UNKNOWN, FREE, OCCUPIED = 0, 1, 2               # DSM_SPACE_*
EXITS = ("free", "range", "outside", "nodepth", "infinite", "notinfront")  # CarveExit of csrc/dsm_carve.h, in order
PAD_DEPTH = 50.0  # what the pad columns of a pitched plane hold: large and finite, so that a read of one frees voxels

_lib = None
_vp = C.c_void_p


class _Grid(C.Structure):  # SpaceHostGrid of space_host.cpp
    _fields_ = [("origin", C.c_float * 3), ("voxel", C.c_float), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("pitch", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("near_d", C.c_float), ("far_d", C.c_float),
                ("margin", C.c_float), ("flags", C.c_uint32)]


class Cam:
    """the camera of a handle: frame size and intrinsics, fx != fy; rows of a slot are `pitch` elements apart"""

    def __init__(self, w, h, fx, fy, cx, cy):
        self.w, self.h, self.fx, self.fy, self.cx, self.cy = w, h, fx, fy, cx, cy
        self.pitch = (w + 63) // 64 * 64


CAM_64 = Cam(64, 48, 57.25, 51.5, 31.3, 23.7)   # pitch == w
CAM_70 = Cam(70, 44, 61.0, 48.5, 34.6, 21.2)    # pitch 128: 58 pad columns a row
CAMS = {"64x48": CAM_64, "70x44": CAM_70}
# (nx, ny, nz): a row shorter than a wave; rows straddling one and two word boundaries; odd sizes in several rows and slices; a
# row of three words with a ragged last wave
GRIDS = ((1, 1, 1), (33, 3, 2), (65, 4, 3), (37, 21, 13), (130, 9, 5))
VOXEL = 0.1
NEAR, FAR, MARGIN = 0.3, 4.0, 0.17


def grid_id(g):
    return "%dx%dx%d" % g


def origin_of(g, centre=(0.0, 0.0, 1.6)):
    """the low corner that puts the grid's centre at `centre`"""
    return tuple(np.float32(centre[a] - g[a] * VOXEL / 2) for a in range(3))


def make(g, cam, origin=None, near=NEAR, far=FAR, margin=MARGIN, flags=0, voxel=VOXEL):
    s = _Grid()
    s.origin[:] = [float(v) for v in (origin_of(g) if origin is None else origin)]
    s.voxel = voxel
    s.nx, s.ny, s.nz = g
    s.w, s.h, s.pitch = cam.w, cam.h, cam.pitch
    s.fx, s.fy, s.cx, s.cy = cam.fx, cam.fy, cam.cx, cam.cy
    s.near_d, s.far_d, s.margin, s.flags = near, far, margin, flags
    return s


def with_flags(s, flags):
    t = _Grid.from_buffer_copy(s)
    t.flags = flags
    return t


def host_lib():
    global _lib
    if _lib is None:
        out = os.path.join(ROOT, "tests", "_build", "libspace_host.so")
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", out + ".tmp"], check=True)
            os.replace(out + ".tmp", out)
        lib = C.CDLL(out)
        lib.space_host_inverse.argtypes = [_vp, _vp]
        lib.space_host_inverse.restype = None
        lib.space_host_carve.argtypes = [C.POINTER(_Grid), C.c_int, _vp, _vp, _vp, _vp]
        lib.space_host_carve.restype = C.c_int64
        lib.space_host_project.argtypes = [C.POINTER(_Grid), _vp, _vp, _vp, _vp]
        lib.space_host_project.restype = None
        lib.space_host_classify.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, C.c_int32]
        lib.space_host_classify.restype = C.c_int32
        _lib = lib
    return _lib


def build_main(out, sanitize=True):
    """space_host.cpp as a stand-alone program (its own main behind SPACE_HOST_MAIN), with the sanitizers"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DSPACE_HOST_MAIN"] + (gc.SANITIZE if sanitize else []) + [SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def write_case(path, s, invs, depths, old, occ):
    """a case file of the stand-alone program: the grid struct, the frame count, the inverses, the pitched planes, the old free set
    and an occupied set"""
    with open(path, "wb") as f:
        f.write(bytes(s))
        f.write(np.array([len(invs)], np.int32).tobytes())
        f.write(np.ascontiguousarray(invs, np.float32).tobytes())
        f.write(np.ascontiguousarray(depths, np.float32).tobytes())
        f.write(np.ascontiguousarray(old, np.uint32).tobytes())
        f.write(np.ascontiguousarray(occ, np.uint32).tobytes())


def words(s):
    return (s.nz, s.ny, (s.nx + 31) // 32)


def closed_form_inverse(pose):
    """the library's inverse of a 4x4 row-major cam -> world pose, 16 column-major floats"""
    p = rc.pose_colmajor(pose)
    inv = np.zeros(16, np.float32)
    host_lib().space_host_inverse(p.ctypes.data, inv.ctypes.data)
    return inv


def inverses_of(frames):
    """[n, 16]: the caller's inverse where a frame has one, the closed form otherwise"""
    return np.stack([closed_form_inverse(pose) if inv is None else np.asarray(inv, np.float32).reshape(16) for pose, inv, _ in frames])


def host_carve(s, frames, old=None, exits=False):
    """the checker: (bits [nz, ny, wx] after carving `frames` = [(pose 4x4, inverse 16 or None, plane [h, pitch])] into `old` (None:
    an empty set), the population count[, the exits [n, nz, ny, nx]])"""
    bits = np.zeros(words(s), np.uint32) if old is None else np.array(old, np.uint32)
    invs = np.ascontiguousarray(inverses_of(frames))
    planes = np.ascontiguousarray(np.stack([np.asarray(d, np.float32) for _, _, d in frames]))
    assert planes.shape[1:] == (s.h, s.pitch) and bits.shape == words(s)
    ex = np.full((len(frames), s.nz, s.ny, s.nx), 9, np.uint8) if exits else None
    n = host_lib().space_host_carve(C.byref(s), len(frames), invs.ctypes.data, planes.ctypes.data, bits.ctypes.data, None if ex is None else ex.ctypes.data)
    return (bits, int(n), ex) if exits else (bits, int(n))


def host_project(s, inv16):
    """(q.z float32, u, v int32) [nz, ny, nx] of every voxel centre against one frame, as the checker computes them"""
    shape = (s.nz, s.ny, s.nx)
    qz, u, v = np.zeros(shape, np.float32), np.zeros(shape, np.int32), np.zeros(shape, np.int32)
    inv = np.ascontiguousarray(inv16, np.float32)
    host_lib().space_host_project(C.byref(s), inv.ctypes.data, qz.ctypes.data, u.ctypes.data, v.ctypes.data)
    return qz, u, v


def host_classify(occ, fre, nx, cap=None, planes=("state", "known_free", "frontier", "cells")):
    """the checker's planes of two bit sets [nz, ny, wx], plus "n_frontier"; cells cut to min(n_frontier, cap)"""
    o, f = np.ascontiguousarray(occ, np.uint32), np.ascontiguousarray(fre, np.uint32)
    nz, ny, wx = o.shape
    assert f.shape == o.shape and wx == (nx + 31) // 32
    cap = nx * ny * nz if cap is None else cap
    out = {"state": np.full((nz, ny, nx), 7, np.uint8), "known_free": np.full(o.shape, 7, np.uint32), "frontier": np.full(o.shape, 7, np.uint32),
           "cells": np.full(max(cap, 1), -7, np.int32)}
    n = host_lib().space_host_classify(o.ctypes.data, f.ctypes.data, nx, ny, nz, *(out[k].ctypes.data if k in planes else None for k in ("state", "known_free", "frontier", "cells")), cap)
    out = {k: a for k, a in out.items() if k in planes}
    if "cells" in out:
        out["cells"] = out["cells"][:min(n, cap)]
    out["n_frontier"] = int(n)
    return out


# ------------------------------------------------------------------ the numpy restatement
def np_project(s, inv16):
    """the definition's steps 1, 2 and 4 in numpy float32, in the order written: (q [3][nz, ny, nx], u, v as float64 before the cast)"""
    f = np.float32
    m = np.asarray(inv16, f)
    half, vox = f(0.5), f(s.voxel)
    c = [f(s.origin[a]) + (np.arange(n).astype(f) + half) * vox for a, n in enumerate((s.nx, s.ny, s.nz))]
    cx, cy, cz = np.meshgrid(c[0], c[1], c[2], indexing="ij")
    cx, cy, cz = (np.ascontiguousarray(a.transpose(2, 1, 0)) for a in (cx, cy, cz))  # [nz, ny, nx]
    with np.errstate(all="ignore"):
        q = [((m[i] * cx + m[4 + i] * cy) + m[8 + i] * cz) + m[12 + i] * f(1.0) for i in range(3)]
        u = ((q[0] * f(s.fx)) / q[2] + f(s.cx)).astype(np.float64) + 0.5
        v = ((q[1] * f(s.fy)) / q[2] + f(s.cy)).astype(np.float64) + 0.5
    return q, u, v


def np_carve(s, frames, old=None):
    """the definition restated: bools [nz, ny, nx] after carving, and the exits [n, nz, ny, nx]"""
    f = np.float32
    free = np.zeros((s.nz, s.ny, s.nx), bool) if old is None or (s.flags & REPLACE) else gc.unpack(old, s.nx)
    exits = []
    for (pose, inv, plane), inv16 in zip(frames, inverses_of(frames)):
        q, u, v = np_project(s, inv16)
        with np.errstate(all="ignore"):
            in_range = (f(s.near_d) < q[2]) & (q[2] < f(s.far_d))
            ok = lambda a: (a >= -2147483648.0) & (a < 2147483648.0)
            ui = np.where(ok(u), np.trunc(np.where(ok(u), u, 0.0)), -2147483648.0).astype(np.int64)
            vi = np.where(ok(v), np.trunc(np.where(ok(v), v, 0.0)), -2147483648.0).astype(np.int64)
            inside = (0 <= ui) & (ui < s.w) & (0 <= vi) & (vi < s.h)
            d = np.asarray(plane, f)[np.clip(vi, 0, s.h - 1), np.clip(ui, 0, s.w - 1)]
            has = d > 0
            infinite = np.isposinf(d) & (not (s.flags & TRUST_INFINITE))
            front = (q[2] + f(s.margin)) < d
        e = np.where(~in_range, 1, np.where(~inside, 2, np.where(~has, 3, np.where(infinite, 4, np.where(front, 0, 5))))).astype(np.uint8)
        exits.append(e)
        free = free | (e == 0)
    return free, np.stack(exits)


def np_classify(occ_vox, free_vox):
    """(state uint8, known_free bools, frontier bools) of two bool arrays [nz, ny, nx]"""
    state = np.where(occ_vox, OCCUPIED, np.where(free_vox, FREE, UNKNOWN)).astype(np.uint8)
    unknown = np.pad(state == UNKNOWN, 1, constant_values=False)  # outside the grid nothing is unknown
    near = np.zeros_like(occ_vox, bool)
    nz, ny, nx = occ_vox.shape
    for dz, dy, dx in ((0, 0, -1), (0, 0, 1), (0, -1, 0), (0, 1, 0), (-1, 0, 0), (1, 0, 0)):
        near |= unknown[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
    known_free = state == FREE
    return state, known_free, known_free & near


# ------------------------------------------------------------------ depth frames and poses
def depth_plane(cam, seed, holes=True):
    """a pitched plane [h, pitch]: a tilted wall 1.3 .. 2.6 m away with blocks of 0, negative, NaN and +inf; the pad columns hold
    PAD_DEPTH"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(cam.w), np.arange(cam.h))
    d = (1.9 + rng.uniform(-0.01, 0.01) * (u - cam.w / 2) + rng.uniform(-0.01, 0.01) * (v - cam.h / 2) + 0.1 * np.sin(u * 0.4 + seed)).astype(np.float32)
    if holes:
        for value in (0.0, -1.0, np.nan, np.inf):
            x, y = int(rng.integers(0, cam.w - 8)), int(rng.integers(0, cam.h - 8))
            d[y:y + 6, x:x + 7] = value
    plane = np.full((cam.h, cam.pitch), PAD_DEPTH, np.float32)
    plane[:, :cam.w] = d
    return plane


def pose_at(t=(0.0, 0.0, 0.0), yaw=0.0, pitch=0.0):
    """cam -> world, 4x4 row-major: turned about y by `yaw` and about x by `pitch`, then moved to t"""
    ry = np.array([[np.cos(yaw), 0, np.sin(yaw)], [0, 1, 0], [-np.sin(yaw), 0, np.cos(yaw)]])
    rx = np.array([[1, 0, 0], [0, np.cos(pitch), -np.sin(pitch)], [0, np.sin(pitch), np.cos(pitch)]])
    p = np.eye(4)
    p[:3, :3] = ry @ rx
    p[:3, 3] = t
    return p.astype(np.float32)


def ulp_inverse(pose, seed):
    """a caller's inverse that differs from the closed form in the last bit of some entries (inverse_cases' "near" family)"""
    import inverse_cases as ic
    base = closed_form_inverse(pose)
    inv = ic.ulp_move(base, ic.ulp_pattern(np.random.default_rng(seed)))
    assert (inv != base).any()
    return inv


POSES = ("identity", "oblique", "inside", "away", "own inverse")


def frame_of(kind, cam, seed, g=(37, 21, 13)):
    """(pose, inverse or None, plane) of one of POSES for the grid g"""
    plane = depth_plane(cam, seed)
    if kind == "identity":
        return rc.IDENTITY.copy(), None, plane
    if kind == "oblique":
        return rc.oblique_pose(), None, plane
    if kind == "inside":  # a camera inside the grid (centred at z = 1.6), a quarter of the way along x, looking along +x
        return pose_at((-g[0] * VOXEL / 4, 0.01, 1.59), yaw=np.pi / 2 - 0.1), None, plane
    if kind == "away":    # looking away from the grid: nothing is freed
        return pose_at((0.0, 0.0, 0.0), yaw=np.pi), None, plane
    pose = pose_at((0.1, 0.05, -0.2), yaw=-0.15, pitch=0.1)
    return pose, ulp_inverse(pose, seed), plane


@functools.lru_cache(maxsize=None)
def case_list():
    """[(grid, camera name, pose kind)]: the one list both test files run"""
    return tuple((g, c, p) for g in GRIDS for c in CAMS for p in POSES)


@functools.lru_cache(maxsize=None)
def case(g, cam_name, kind):
    """(grid struct, [frame]) of a case"""
    cam = CAMS[cam_name]
    return make(g, cam), [frame_of(kind, cam, 100 * GRIDS.index(g) + 10 * POSES.index(kind) + cam.w, g)]


@functools.lru_cache(maxsize=None)
def expected(g, cam_name, kind):
    """the checker's (bits, count) of a case carved into an empty set, computed once; read-only"""
    s, frames = case(g, cam_name, kind)
    bits, n = host_carve(s, frames)
    bits.setflags(write=False)
    return bits, n


def many_frames(cam, n, seed=5):
    """n frames with poses on an arc about the grid's centre, each with its own plane"""
    out = []
    for k in range(n):
        a = -0.5 + k / max(n - 1, 1)
        out.append((pose_at((1.6 * np.sin(a), 0.05 * (k % 3), 1.6 - 1.6 * np.cos(a)), yaw=-a), None, depth_plane(cam, seed + k)))
    return out


# ------------------------------------------------------------------ the crafted census case
CENSUS_GRID = (37, 21, 13)


@functools.lru_cache(maxsize=None)
def census_case():
    """One grid in which every exit of carve_voxel is taken.  Returns (grid struct, frames, marks): frame 0 is an identity camera in
    front of a grid that reaches past the near and the far distance and past all four image edges, with a wall at 1.7 m, blocks of 0,
    negative, NaN and +inf, and three pixels whose depth is set from the checker's own q.z + margin of a voxel projecting there: the
    float just below, equal and just above.  Frames 1 and 2 differ in one translation entry of the inverse by one float: between them
    the projection of one voxel crosses a .5 pixel boundary (found by bisection on the checker's own rounding), and the two pixels
    hold a free and an empty depth.  marks: {name: (frame, z, y, x)}."""
    cam = CAM_64
    s = make(CENSUS_GRID, cam, origin=origin_of(CENSUS_GRID, (0.0, 0.0, 1.65)), near=1.25, far=2.05, margin=MARGIN)
    ident = closed_form_inverse(rc.IDENTITY)
    qz, u, v = host_project(s, ident)
    plane = np.full((cam.h, cam.pitch), 1.7, np.float32)
    plane[4:10, 6:12], plane[4:10, 20:26], plane[30:36, 6:12], plane[30:36, 40:46] = 0.0, -2.0, np.nan, np.inf
    f = np.float32
    inside = (u >= 0) & (u < cam.w) & (v >= 0) & (v < cam.h) & (qz > f(s.near_d)) & (qz < f(s.far_d))
    marks, taken = {}, set()
    # three voxels in the plain part of the wall, each alone on its pixel among the marked ones
    cands = [tuple(i) for i in np.argwhere(inside) if 12 < v[tuple(i)] < 28 and 14 < u[tuple(i)] < 50]
    for name, move in (("margin below", np.inf), ("margin equal", None), ("margin above", -np.inf)):
        for i in cands:
            px = (int(v[i]), int(u[i]))
            if px in taken:
                continue
            taken.add(px)
            edge = f(qz[i] + f(s.margin))
            plane[px] = edge if move is None else np.nextafter(edge, f(move))
            marks[name] = (0,) + i
            break
    # the .5 boundary: a voxel on the optical axis' row, its u moved by the translation of the inverse
    i = next(tuple(i) for i in np.argwhere(inside) if (int(v[tuple(i)]), int(u[tuple(i)])) not in taken and 14 < u[tuple(i)] < 50 and 12 < v[tuple(i)] < 28)
    lo, hi = ident.copy(), ident.copy()
    hi[12] = f(0.05)  # 5 cm to the right: more than a pixel at any depth of the grid
    u_lo, u_hi = int(host_project(s, lo)[1][i]), int(host_project(s, hi)[1][i])
    assert u_hi > u_lo
    a, b = int(lo[12:13].view(np.int32)[0]), int(hi[12:13].view(np.int32)[0])  # (non-negative floats order as their bits)
    while b - a > 1:
        mid = ident.copy()
        mid[12:13] = np.array([(a + b) // 2], np.int32).view(np.float32)
        if int(host_project(s, mid)[1][i]) > u_lo:
            b = (a + b) // 2
        else:
            a = (a + b) // 2
    below, above = ident.copy(), ident.copy()
    below[12:13], above[12:13] = np.array([a], np.int32).view(np.float32), np.array([b], np.int32).view(np.float32)
    plane2 = np.full((cam.h, cam.pitch), 3.0, np.float32)  # everything in range is free ...
    plane2[:, u_lo + 1] = 0.0                               # ... but for the column just right of the boundary
    marks["half below"], marks["half above"] = (1,) + i, (2,) + i
    frames = [(rc.IDENTITY.copy(), None, plane), (rc.IDENTITY.copy(), below, plane2), (rc.IDENTITY.copy(), above, plane2)]
    return s, frames, marks


# ------------------------------------------------------------------ the sets of the classification
@functools.lru_cache(maxsize=None)
def classify_sets(g):
    """{name: (occupied, free) bools [nz, ny, nx]}"""
    nx, ny, nz = g
    n = (nz, ny, nx)
    rng = np.random.default_rng(7000 + 100 * nx + 10 * ny + nz)
    out = {}
    for density in (0.05, 0.5):
        out["random %g" % density] = (rng.random(n) < density, rng.random(n) < density)
    out["empty"] = (np.zeros(n, bool), np.zeros(n, bool))
    out["full"] = (np.ones(n, bool), np.ones(n, bool))
    out["all free"] = (np.zeros(n, bool), np.ones(n, bool))  # no frontier anywhere: the grid's border makes none
    out["sparse free"] = (rng.random(n) < 0.3, rng.random(n) < 0.9)
    for pair in out.values():
        for a in pair:
            a.setflags(write=False)
    return out


CLASSIFY_GRIDS = ((1, 1, 1), (33, 3, 2), (65, 4, 3), (37, 21, 13), (130, 9, 5), (64, 5, 3))


def by_hand():
    """[(name, dims, occupied voxels, free voxels, frontier voxels)] as (x, y, z) lists: the cases that can be checked by eye"""
    g = (70, 5, 4)
    six = lambda x, y, z: [(x - 1, y, z), (x + 1, y, z), (x, y - 1, z), (x, y + 1, z), (x, y, z - 1), (x, y, z + 1)]
    everything = [(x, y, z) for z in range(g[2]) for y in range(g[1]) for x in range(g[0])]
    return [
        ("a single free voxel in an unknown grid", g, [], [(40, 2, 1)], [(40, 2, 1)]),
        ("all six neighbours free", g, [], [(40, 2, 1)] + six(40, 2, 1), six(40, 2, 1)),
        ("all six neighbours occupied", g, six(40, 2, 1), [(40, 2, 1)], []),
        ("free at x = 31, the only unknown neighbour at x = 32", g, [n for n in six(31, 2, 1) if n != (32, 2, 1)], [(31, 2, 1)], [(31, 2, 1)]),
        ("free at x = 32, the only unknown neighbour at x = 31", g, [n for n in six(32, 2, 1) if n != (31, 2, 1)], [(32, 2, 1)], [(32, 2, 1)]),
        ("free at x = 63, the only unknown neighbour at x = 64", g, [n for n in six(63, 2, 1) if n != (64, 2, 1)], [(63, 2, 1)], [(63, 2, 1)]),
        ("free at x = 32 with x = 31 known: no carry", g, six(32, 2, 1), [(32, 2, 1)], []),
        ("free on the grid's faces with everything inside known", g, [p for p in everything if p not in ((0, 0, 0), (69, 4, 3), (31, 0, 2))],
         [(0, 0, 0), (69, 4, 3), (31, 0, 2)], []),
    ]


def voxels(g, points):
    b = np.zeros(g[::-1], bool)
    for x, y, z in points:
        b[z, y, x] = True
    return b


def dirty_pads(bits, nx, rng):
    """the bit set with random garbage in the pad bits of every row's last word"""
    d = np.array(bits, np.uint32)
    d[..., -1] |= gc.pad_mask(nx) & rng.integers(0, 1 << 32, d[..., -1].shape, dtype=np.uint64).astype(np.uint32)
    return d
