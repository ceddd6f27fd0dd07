"""Shared by tests/test_cpu_view.py and tests/test_gpu_view.py: the host build of the definition of the viewpoint gain
(tests/view_host.cpp: csrc/dsm_view.h by brute force over every pose, voxel and interior point of its line, the line by the closed
form), an independent numpy restatement, the grids, the view cameras, the poses and the three bit sets, ONE list of calls with the
checker's result computed once per call and handed out read-only, and the crafted census calls with their census."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import grid_cases as gc
import render_cases as rc
import space_cases as sc

ROOT = gc.ROOT
SRC = os.path.join(ROOT, "tests", "view_host.cpp")
CSRC = os.path.join(ROOT, "densesurfelmapping_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("dsm_math.h", "dsm_align.h", "dsm_carve.h", "dsm_view.h", "dsm_components.h")] + [os.path.join(ROOT, "include", "dsm.h")]
UNKNOWN_BLOCKS, MAX_REACH, MAX_POSES = 1, 4096, 4096  # DSM_VIEW_UNKNOWN_BLOCKS, DSM_VIEW_MAX_REACH, DSM_VIEW_MAX_POSES of include/dsm.h
EXITS = ("visible", "near", "far", "left", "right", "above", "below", "blocked")  # ViewExit of view_host.cpp, in order
SCORE_DTYPE = np.dtype([("in_view", np.int32), ("visible", np.int32), ("unknown", np.int32), ("free", np.int32), ("occupied", np.int32), ("target", np.int32),
                        ("reserved", np.int32, (2,))])
LINE_DTYPE = np.dtype([("n", np.int32), ("blockers", np.int32), ("k_first", np.int32), ("outside", np.int32)])  # ViewHostLine
VOXEL = sc.VOXEL

_lib = None
_vp = C.c_void_p


class _Grid(C.Structure):  # ViewHostGrid of view_host.cpp
    _fields_ = [("origin", C.c_float * 3), ("voxel", C.c_float), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32), ("w", C.c_int32), ("h", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("near_d", C.c_float), ("far_d", C.c_float), ("flags", C.c_uint32)]


class Cam:
    """a view camera (dsm_render_camera): a coarse sensor model, fx != fy"""

    def __init__(self, width, height, fx, fy, cx, cy, near_dist, far_dist):
        self.width, self.height, self.fx, self.fy, self.cx, self.cy, self.near_dist, self.far_dist = width, height, fx, fy, cx, cy, near_dist, far_dist


CAM_40 = Cam(40, 30, 30.5, 26.25, 19.6, 14.3, 0.25, 3.0)     # half angles 33 and 30 degrees; the far bound cuts the longer grids
CAM_NEAR = Cam(40, 30, 30.5, 26.25, 19.6, 14.3, 0.03, 3.6)   # the census: near enough for the camera's own voxel, far enough for the last word
CAM_REACH = Cam(9, 7, 30.5, 26.25, 4.4, 3.3, 0.25, 1000.0)   # a camera DSM_VIEW_MAX_REACH voxels away still has the grid in range
GRID_70, GRID_130, GRID_1, GRID_33, GRID_256 = (70, 33, 19), (130, 3, 2), (1, 1, 1), (33, 5, 3), (256, 64, 32)


def make(g, cam, flags=0, origin=None, voxel=VOXEL):
    s = _Grid()
    s.origin[:] = [float(v) for v in (sc.origin_of(g) if origin is None else origin)]
    s.voxel = voxel
    s.nx, s.ny, s.nz = g
    s.w, s.h = cam.width, cam.height
    s.fx, s.fy, s.cx, s.cy = cam.fx, cam.fy, cam.cx, cam.cy
    s.near_d, s.far_d, s.flags = cam.near_dist, cam.far_dist, flags
    return s


def with_flags(s, flags):
    t = _Grid.from_buffer_copy(s)
    t.flags = flags
    return t


def cam_of(s):
    return Cam(s.w, s.h, s.fx, s.fy, s.cx, s.cy, s.near_d, s.far_d)


def dims(s):
    return (s.nx, s.ny, s.nz)


def words(s):
    return (s.nz, s.ny, (s.nx + 31) // 32)


def host_lib():
    global _lib
    if _lib is None:
        out = os.path.join(ROOT, "tests", "_build", "libview_host.so")
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", out + ".tmp"], check=True)
            os.replace(out + ".tmp", out)
        lib = C.CDLL(out)
        lib.view_host_inverse.argtypes = [_vp, _vp]
        lib.view_host_inverse.restype = None
        lib.view_host_cam_voxel.argtypes = [C.POINTER(_Grid), _vp, _vp]
        lib.view_host_score.argtypes = [C.POINTER(_Grid), C.c_int] + [_vp] * 9
        lib.view_host_score.restype = C.c_int64
        for f in (lib.view_host_walk, lib.view_host_line):
            f.argtypes = [_vp, _vp, _vp, C.c_int32, C.c_int32]
            f.restype = C.c_int32
        _lib = lib
    return _lib


def build_main(out, sanitize=True):
    """view_host.cpp as a stand-alone program (its own main behind VIEW_HOST_MAIN), with the sanitizers"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DVIEW_HOST_MAIN"] + (gc.SANITIZE if sanitize else []) + [SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def closed_form_inverse(pose):
    """the library's inverse of a 4x4 row-major cam -> world pose, 16 column-major floats"""
    p = rc.pose_colmajor(pose)
    inv = np.zeros(16, np.float32)
    host_lib().view_host_inverse(p.ctypes.data, inv.ctypes.data)
    return inv


def inverses_of(poses, invs=None):
    """[n, 16]: the caller's inverse where a pose has one, the closed form otherwise"""
    invs = [None] * len(poses) if invs is None else invs
    return np.stack([closed_form_inverse(p) if i is None else np.asarray(i, np.float32).reshape(16) for p, i in zip(poses, invs)])


def cam_voxel(s, pose):
    """(the camera's voxel int32 [3] as the checker takes it, whether the reach rule admits it)"""
    a = np.zeros(3, np.int32)
    p = rc.pose_colmajor(pose)
    ok = host_lib().view_host_cam_voxel(C.byref(s), p.ctypes.data, a.ctypes.data)
    return a, bool(ok)


def write_case(path, s, poses, invs, occ, fre, target):
    """a case file of the stand-alone program: the grid struct, the pose count, whether a target follows, the inverses, the cameras'
    voxels, the sets"""
    with open(path, "wb") as f:
        f.write(bytes(s))
        f.write(np.array([len(poses), 0 if target is None else 1], np.int32).tobytes())
        f.write(np.ascontiguousarray(inverses_of(poses, invs), np.float32).tobytes())
        f.write(np.ascontiguousarray(np.stack([cam_voxel(s, p)[0] for p in poses]), np.int32).tobytes())
        for b in (occ, fre) + (() if target is None else (target,)):
            f.write(np.ascontiguousarray(b, np.uint32).tobytes())


def host_view(s, poses, occ, fre, target=None, invs=None, detail=False):
    """the checker: {"scores" SCORE_DTYPE [n], "visible" uint32 [n, nz, ny, wx], "steps"[, "exits" uint8 [n, nz, ny, nx], "lines"
    LINE_DTYPE [n, nz, ny, nx], "cams" int32 [n, 3]]}"""
    n = len(poses)
    inv = np.ascontiguousarray(inverses_of(poses, invs))
    cams = np.ascontiguousarray(np.stack([cam_voxel(s, p)[0] for p in poses]))
    assert all(cam_voxel(s, p)[1] for p in poses), "a camera beyond the reach"
    o, f = np.ascontiguousarray(occ, np.uint32), np.ascontiguousarray(fre, np.uint32)
    t = None if target is None else np.ascontiguousarray(target, np.uint32)
    assert o.shape == words(s) == f.shape and (t is None or t.shape == o.shape)
    out = {"scores": np.full(n, -7, np.int32).repeat(8).view(SCORE_DTYPE), "visible": np.full((n,) + words(s), 0xdeadbeef, np.uint32), "cams": cams}
    if detail:
        out["exits"] = np.full((n, s.nz, s.ny, s.nx), 9, np.uint8)
        out["lines"] = np.zeros((n, s.nz, s.ny, s.nx), LINE_DTYPE)
    steps = host_lib().view_host_score(C.byref(s), n, inv.ctypes.data, cams.ctypes.data, o.ctypes.data, f.ctypes.data, None if t is None else t.ctypes.data,
                                       out["scores"].ctypes.data, out["visible"].ctypes.data, out["exits"].ctypes.data if detail else None,
                                       out["lines"].ctypes.data if detail else None)
    assert steps >= 0
    out["steps"] = int(steps)
    return out


def host_walk(a, v, closed=False, skip=0, cap=None):
    """the interior points k = skip + 1 .. (all of them, or `cap`) of the line from a towards v, [.., 3]: by ViewWalk's error terms
    stepped from k = 1, or by the checker's closed form"""
    a, v = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(v, np.int32)
    n = int(np.abs(v.astype(np.int64) - a).max())
    m = max(min(n - 1 - skip, n - 1 if cap is None else cap), 0)
    out = np.zeros((max(m, 1), 3), np.int32)
    got = (host_lib().view_host_line if closed else host_lib().view_host_walk)(a.ctypes.data, v.ctypes.data, out.ctypes.data, skip, m)
    assert got == n
    return out[:m]


# ------------------------------------------------------------------ the numpy restatement
def np_line_points(a, d, n, k, truncate=False):
    """point k of the lines from a (int64 [3]) with differences d [..., 3] and lengths n [...]: a + floor((2 k d + n) / (2 n)), the
    floor by numpy's floor_divide on int64 (truncate: C's quotient instead, the mistake the census looks for)"""
    num, den = 2 * k * d + n[..., None], 2 * np.maximum(n, 1)[..., None]
    q = np.sign(num) * (np.abs(num) // den) if truncate else np.floor_divide(num, den)
    return a + q


def np_view(s, poses, occ, fre, target=None, invs=None, truncate=False):
    """the definition restated: {"scores", "visible" (bools [n, nz, ny, nx]), "exits", "lines"} for every pose and voxel"""
    f = np.float32
    o, fr = gc.unpack(occ, s.nx), gc.unpack(fre, s.nx)
    tg = None if target is None else gc.unpack(target, s.nx)
    blockers = (o | ~fr) if (s.flags & UNKNOWN_BLOCKS) else o
    zz, yy, xx = np.meshgrid(np.arange(s.nz), np.arange(s.ny), np.arange(s.nx), indexing="ij")
    vox = np.stack([xx, yy, zz], -1).astype(np.int64)
    hi = np.array(dims(s), np.int64)
    scores = np.zeros(len(poses), SCORE_DTYPE)
    vis_all, exits_all, lines_all = [], [], []
    for p, (pose, inv16) in enumerate(zip(poses, inverses_of(poses, invs))):
        q, u, v = sc.np_project(s, inv16)
        with np.errstate(all="ignore"):
            near_ok, far_ok = f(s.near_d) < q[2], q[2] < f(s.far_d)
            ok = lambda a: (a >= -2147483648.0) & (a < 2147483648.0)
            ui = np.where(ok(u), np.trunc(np.where(ok(u), u, 0.0)), -2147483648.0).astype(np.int64)
            vi = np.where(ok(v), np.trunc(np.where(ok(v), v, 0.0)), -2147483648.0).astype(np.int64)
        e = np.where(~(near_ok & far_ok), np.where(far_ok, 1, 2), np.where(ui < 0, 3, np.where(ui >= s.w, 4, np.where(vi < 0, 5, np.where(vi >= s.h, 6, 0))))).astype(np.uint8)
        a = np.floor((np.asarray(pose, f)[:3, 3].astype(np.float64) - np.array(s.origin[:], f).astype(np.float64)) / np.float64(f(s.voxel))).astype(np.int64)
        d = vox - a
        n = np.abs(d).max(-1)
        lines = np.zeros(n.shape, LINE_DTYPE)
        lines["n"] = n
        for k in range(1, int(n.max())):
            live = k < n
            pt = np_line_points(a, d, n, k, truncate)
            inside = live & ((pt >= 0) & (pt < hi)).all(-1)
            c = np.clip(pt, 0, hi - 1)
            hit = inside & blockers[c[..., 2], c[..., 1], c[..., 0]]
            lines["k_first"] = np.where(hit & (lines["blockers"] == 0), k, lines["k_first"])
            lines["blockers"] += hit
            lines["outside"] += live & ~inside
        in_view = e == 0
        e = np.where(in_view & (lines["blockers"] > 0), 7, e).astype(np.uint8)
        vis = e == 0
        state = np.where(o, 2, np.where(fr, 1, 0))
        scores[p] = (in_view.sum(), vis.sum(), (vis & (state == 0)).sum(), (vis & (state == 1)).sum(), (vis & (state == 2)).sum(),
                     0 if tg is None else (vis & tg).sum(), (0, 0))
        vis_all.append(vis)
        exits_all.append(e)
        lines_all.append(lines)
    return {"scores": scores, "visible": np.stack(vis_all), "exits": np.stack(exits_all), "lines": np.stack(lines_all)}


def pack_planes(vis):
    return np.stack([gc.pack(v) for v in vis])


# ------------------------------------------------------------------ poses
def look(forward, t, roll=0.0):
    """cam -> world, 4x4 row-major: the camera (x right, y down, z forward) at t looking along `forward`"""
    z = np.asarray(forward, np.float64) / np.linalg.norm(forward)
    h = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(h, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    cr, sr = np.cos(roll), np.sin(roll)
    p = np.eye(4)
    p[:3, 0], p[:3, 1], p[:3, 2], p[:3, 3] = cr * x + sr * y, cr * y - sr * x, z, t
    return p.astype(np.float32)


def centre_of(s, v):
    """the world position of the centre of voxel v (float64)"""
    return np.array(s.origin[:], np.float64) + (np.asarray(v, np.float64) + 0.5) * float(np.float32(s.voxel))


def pose_set(s, n, seed):
    """n poses for the grid of s, each looking at a random point of the grid: in turn a camera inside the grid (where the grid is at
    least a metre long) and one 0.4 to 2 m from that point in a random direction, mostly outside a thin grid; every seventh one
    stands outside and looks away (it sees nothing).  The directions spread over the sphere, so every axis dominates some lines."""
    rng = np.random.default_rng(seed)
    lo = np.array(s.origin[:], np.float64)
    size = np.array(dims(s), np.float64) * VOXEL
    out = []
    for k in range(n):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        at = lo + rng.uniform(0.1, 0.9, 3) * size
        if k % 7 == 6:
            t = lo + size / 2 + np.sign(d) * (size / 2 + 0.4)
        elif k % 2 == 0 and size.max() >= 1.0:
            t = lo + rng.uniform(0.05, 0.95, 3) * size
            if np.linalg.norm(at - t) > 0.3:
                d = at - t
        else:
            t = at - d * rng.uniform(0.4, 2.0)
        out.append(look(d, t, rng.uniform(-0.3, 0.3)))
    return out


def reach_pose(s, axis, side):
    """a camera whose voxel along `axis` is -MAX_REACH ("low"), n + MAX_REACH - 1 ("high"), or one further out ("low-1", "high+1": what
    the reach rule refuses); it stands on the grid's centre line and looks at the grid"""
    n = dims(s)[axis]
    a = {"low": -MAX_REACH, "low-1": -MAX_REACH - 1, "high": n + MAX_REACH - 1, "high+1": n + MAX_REACH}[side]
    v = np.array(dims(s), np.float64) / 2 - 0.5
    v[axis] = a
    t = centre_of(s, v)
    fwd = np.zeros(3)
    fwd[axis] = 1.0 if side.startswith("low") else -1.0
    pose = look(fwd, t)
    got, ok = cam_voxel(s, pose)
    assert got[axis] == a and ok == (side in ("low", "high")), (got, a, side)
    return pose


# ------------------------------------------------------------------ the sets
def sets_of(s, seed, pads=True):
    """(occupied, free, target) bit sets [nz, ny, wx] for the grid of s: occupied = a tilted sheet one voxel thick in |n|_1 plus 1 % of
    noise, free = a ball round the grid's centre plus 30 % of noise (so that free and occupied overlap), target = 10 % of noise; the
    pad bits of all three hold garbage"""
    rng = np.random.default_rng(seed)
    g = dims(s)
    zz, yy, xx = np.meshgrid(np.arange(g[2]), np.arange(g[1]), np.arange(g[0]), indexing="ij")
    nrm = rng.normal(size=3)
    nrm /= np.abs(nrm).sum()
    e = nrm[0] * (xx - g[0] * 0.7) + nrm[1] * (yy - g[1] * 0.5) + nrm[2] * (zz - g[2] * 0.5)
    occ = (np.abs(e) <= 0.5) | (rng.random(g[::-1]) < 0.01)
    r2 = (xx - g[0] / 2) ** 2 + (yy - g[1] / 2) ** 2 + (zz - g[2] / 2) ** 2
    fre = (r2 < (max(g) * 0.35) ** 2) | (rng.random(g[::-1]) < 0.3)
    tgt = rng.random(g[::-1]) < 0.1
    out = tuple(gc.pack(b) for b in (occ, fre, tgt))
    return tuple(sc.dirty_pads(b, g[0], rng) for b in out) if pads else out


# ------------------------------------------------------------------ ONE list of calls
# name: (grid, camera, number of poses, seed); the poses of "reach" are the four admitted ends along x of a 130-voxel row
CALLS = {
    "70x33x19/1": (GRID_70, CAM_40, 1, 15), "70x33x19/3": (GRID_70, CAM_40, 3, 12), "70x33x19/65": (GRID_70, CAM_40, 65, 13),
    "130x3x2/1": (GRID_130, CAM_40, 1, 21), "130x3x2/3": (GRID_130, CAM_40, 3, 22), "130x3x2/65": (GRID_130, CAM_40, 65, 23),
    "1x1x1/1": (GRID_1, CAM_40, 1, 31), "1x1x1/3": (GRID_1, CAM_40, 3, 32),
    "33x5x3/4096": (GRID_33, CAM_40, MAX_POSES, 41),
    "256x64x32/8": (GRID_256, CAM_40, 8, 51),
    "130x3x2/reach": (GRID_130, CAM_REACH, 0, 61), "1x1x1/reach": (GRID_1, CAM_REACH, 0, 62),
}


@functools.lru_cache(maxsize=None)
def call(name):
    """(grid struct, poses, occupied, free, target) of one of CALLS"""
    g, cam, n, seed = CALLS[name]
    s = make(g, cam)
    if name.endswith("/reach"):
        poses = [reach_pose(s, axis, side) for axis in range(3) for side in ("low", "high")]
    else:
        poses = pose_set(s, n, seed)
    occ, fre, tgt = sets_of(s, seed)
    for b in (occ, fre, tgt):
        b.setflags(write=False)
    return s, poses, occ, fre, tgt


@functools.lru_cache(maxsize=None)
def expected(name, flags=0, target=True):
    """the checker's result for a call, computed once and read-only"""
    s, poses, occ, fre, tgt = call(name)
    out = host_view(with_flags(s, flags), poses, occ, fre, tgt if target else None)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ------------------------------------------------------------------ the census
CENSUS_GRID = GRID_70
CENSUS_CAM_VOXEL = (35, 16, 9)


def census_call():
    """(grid struct, poses, occupied, free, target, marks): six cameras in one voxel near the grid's centre, at its back face along
    each axis so that the voxel's own centre is in view, one camera 1.2 m outside the low x face looking in, and one outside looking
    away.  The occupied set is placed by hand: a neighbour of the camera's voxel, the camera's voxel itself, patches on both sides of
    the word seams and in the last word, and a sprinkle; the free set leaves corridors of unknown voxels."""
    s = make(CENSUS_GRID, CAM_NEAR)
    g = CENSUS_GRID
    a = np.array(CENSUS_CAM_VOXEL)
    poses = []
    for axis in range(3):
        for sign in (1.0, -1.0):
            fwd = np.zeros(3)
            fwd[axis] = sign
            poses.append(look(fwd, centre_of(s, a) - fwd * 0.045))
    c = centre_of(s, a)
    poses.append(look((1.0, 0.02, 0.01), (float(s.origin[0]) - 1.2, c[1], c[2])))            # outside, looking in along the row
    poses.append(look((-1.0, 0.0, 0.0), (float(s.origin[0]) - 0.4, c[1], c[2])))             # outside, looking away
    for p in poses[:6]:
        assert tuple(cam_voxel(s, p)[0]) == CENSUS_CAM_VOXEL
    rng = np.random.default_rng(71)
    occ = rng.random(g[::-1]) < 0.004
    occ[a[2] - 2:a[2] + 3, a[1] - 2:a[1] + 3, a[0] - 2:a[0] + 3] = False
    occ[a[2], a[1], a[0]] = True            # the camera's own voxel: it never blocks
    occ[a[2], a[1] + 1, a[0]] = True        # a neighbour: what lies behind it is blocked at k = 1
    for x, y0 in ((63, 8), (64, 14), (67, 20), (32, 8), (31, 14)):  # both sides of the seams 31|32 and 63|64, and the last, partial word
        occ[7:12, y0:y0 + 4, x] = True
    occ[:, :, 0:6] &= rng.random((g[2], g[1], 6)) < 0.3  # thin near the low x face, where pose 6 enters
    fre = rng.random(g[::-1]) < 0.85
    tgt = rng.random(g[::-1]) < 0.1
    bits = tuple(sc.dirty_pads(gc.pack(b), g[0], rng) for b in (occ, fre, tgt))
    marks = {"camera": tuple(a), "neighbour": (a[0], a[1] + 1, a[2]), "outside pose": 6, "away pose": 7, "seam xs": (31, 32, 63, 64), "last word": range(64, 70)}
    return (s, poses) + bits + (marks,)


def inverse_call():
    """(grid struct, pose, the closed-form inverse, a caller's inverse one ulp away in one entry) with the far bound of the camera set
    ON the depth of a slice of voxel centres: the caller's inverse moves voxels across the bound.  The entry and the direction are
    searched for here, deterministically; the census asserts that the search found one."""
    cam = Cam(40, 30, 30.5, 26.25, 19.6, 14.3, 0.25, 3.0)
    s = make(CENSUS_GRID, cam)
    pose = look((1.0, 0.0, 0.0), centre_of(s, (4, 16, 9)))
    base = closed_form_inverse(pose)
    qz = sc.np_project(s, base)[0][2]
    cam.far_dist = float(qz[9, 16, 30])  # the depth of the centre of voxel (30, 16, 9): that slice sits on the bound
    s = make(CENSUS_GRID, cam)
    for k in (12, 13, 14, 0, 1, 2, 4, 5, 6, 8, 9, 10):
        for toward in (-np.inf, np.inf):
            inv = base.copy()
            inv[k] = np.nextafter(inv[k], np.float32(toward))
            e0 = np_exits_in_view(s, base)
            e1 = np_exits_in_view(s, inv)
            if (e0 != e1).any():
                return s, pose, base, inv
    return s, pose, base, None


def np_exits_in_view(s, inv16):
    f = np.float32
    q, u, v = sc.np_project(s, inv16)
    with np.errstate(all="ignore"):
        return (f(s.near_d) < q[2]) & (q[2] < f(s.far_d)) & (np.trunc(u) >= 0) & (np.trunc(u) < s.w) & (np.trunc(v) >= 0) & (np.trunc(v) < s.h) & (u > -1) & (v > -1)


def census(s, poses, occ, fre, tgt, marks, res, res_unknown, res_trunc):
    """What the census call contains, from the checker's detailed result `res` (flags 0), its result with UNKNOWN_BLOCKS, and the numpy
    restatement with the floor replaced by truncation: a dict of counts, every one of which the tests assert to be positive."""
    e, ln, cams = res["exits"], res["lines"], res["cams"]
    g = dims(s)
    zz, yy, xx = np.meshgrid(np.arange(g[2]), np.arange(g[1]), np.arange(g[0]), indexing="ij")
    vox = np.stack([xx, yy, zz], -1).astype(np.int64)
    out = {"exit " + name: int((e == k).sum()) for k, name in enumerate(EXITS)}
    in_view = (e == 0) | (e == 7)
    blocked, one = e == 7, ln["blockers"] == 1
    out["blocked at k = 1 only"] = int((blocked & one & (ln["k_first"] == 1) & (ln["n"] > 2)).sum())
    out["blocked at k = n - 1 only"] = int((blocked & one & (ln["k_first"] == ln["n"] - 1) & (ln["n"] > 2)).sum())
    p_out = marks["outside pose"]
    out["camera outside: blocked only beyond a stretch outside the grid"] = int((blocked[p_out] & one[p_out] & (ln["outside"][p_out] > 0)).sum())
    out["camera outside"] = int(not ((cams[p_out] >= 0) & (cams[p_out] < g)).all())
    out["n = 0 in view"] = int((in_view & (ln["n"] == 0)).sum())
    out["n = 1 in view"] = int((in_view & (ln["n"] == 1)).sum())
    tie = np.zeros(e.shape, bool)
    dom = {}
    for p in range(len(poses)):
        d = vox - cams[p].astype(np.int64)
        n = np.abs(d).max(-1)
        tie[p] = (n == 2) & ((2 * d + 2) % 4 == 0).any(-1) & (np.abs(d) == 1).any(-1)
        for axis in range(3):
            for sign in (1, -1):
                alone = (np.abs(d[..., axis]) == n) & (np.delete(np.abs(d), axis, -1).max(-1) < n) & (np.sign(d[..., axis]) == sign) & (n > 1)
                dom[(axis, sign)] = dom.get((axis, sign), 0) + int((alone & in_view[p]).sum())
    out["n = 2 with a tie in view"] = int((in_view & tie).sum())
    for (axis, sign), c in dom.items():
        out["dominant axis %s%s" % ("+" if sign > 0 else "-", "xyz"[axis])] = c
    out["outcome changes under truncation"] = int((in_view & ((res_trunc["exits"] == 7) != blocked)).sum())
    cam_vox = marks["camera"]
    out["camera's voxel occupied"] = int(gc.unpack(occ, g[0])[cam_vox[2], cam_vox[1], cam_vox[0]]) * int((e[:6] == 0).sum() > 0)
    # where the first blocker of a blocked pair lies
    first_x = {}
    for p in range(len(poses)):
        a = cams[p].astype(np.int64)
        m = blocked[p]
        d, n, k = (vox - a)[m], ln["n"][p][m].astype(np.int64), ln["k_first"][p][m].astype(np.int64)
        pt = np_line_points(a, d, n, k[..., None])
        for x in pt[..., 0]:
            first_x[int(x)] = first_x.get(int(x), 0) + 1
    for x in marks["seam xs"]:
        out["first blocker at x = %d" % x] = first_x.get(x, 0)
    out["first blocker in the last word"] = sum(first_x.get(x, 0) for x in marks["last word"])
    pad = gc.pad_mask(g[0])
    out["pad bits set in all three sources"] = int(all((b[..., -1] & pad).any() for b in (occ, fre, tgt)))
    out["blocks only with UNKNOWN_BLOCKS"] = int(((e == 0) & (res_unknown["exits"] == 7)).sum())
    out["a pose seeing nothing"] = int(res["scores"]["in_view"][marks["away pose"]] == 0)
    out["fx != fy"] = int(s.fx != s.fy)
    return out
