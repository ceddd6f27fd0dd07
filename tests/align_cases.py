"""Shared by tests/test_cpu_align.py and tests/test_gpu_align.py: the host build of the alignment's definition
(tests/align_host.cpp over csrc/dsm_align.h), an independent numpy restatement of one evaluation, the crafted planes that sit on
every exit of the per-pixel rule, random planes and the room-corner scene."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import render_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "align_host.cpp")
CSRC = os.path.join(ROOT, "densesurfelmapping_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "dsm_math.h"), os.path.join(CSRC, "dsm_align.h"), os.path.join(ROOT, "include", "dsm.h")]
N_SUMS = 29
# AlignExit of csrc/dsm_align.h
PASS, X_DEPTH, X_RANGE_Z, X_RANGE_Q, X_OUTSIDE, X_MODEL_DEPTH, X_NORMAL, X_DISTANCE, X_VIEW_COS, N_EXITS = range(10)
f32 = np.float32
_vp = C.c_void_p
_lib = None


class FrameDesc(C.Structure):
    """align_host_frame_desc of tests/align_host.cpp: the handle's side of an evaluation"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("pitch", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("near_dist", C.c_float), ("far_dist", C.c_float)]


class Params(C.Structure):
    """dsm_align_params of include/dsm.h"""
    _fields_ = [("struct_size", C.c_uint32), ("max_iterations", C.c_int32), ("stride", C.c_int32), ("dist_max", C.c_float),
                ("min_view_cos", C.c_float), ("huber", C.c_float), ("min_pixels", C.c_int32), ("stop_translation", C.c_float),
                ("stop_rotation", C.c_float)]


class Result(C.Structure):
    """dsm_align_result of include/dsm.h"""
    _fields_ = [("pose16", C.c_float * 16), ("T16", C.c_float * 16), ("status", C.c_int32), ("iterations", C.c_int32), ("n_pixels", C.c_int32),
                ("scale_log2", C.c_int32), ("rms", C.c_double), ("sums", C.c_int64 * N_SUMS)]


CONVERGED, MAX_ITERATIONS, TOO_FEW, SINGULAR = range(4)


def params(**kw):
    p = Params(C.sizeof(Params), 10, 2, 0.25, 0.2, 0.05, 200, 1e-4, 1e-4)
    for k, v in kw.items():
        assert k in dict(Params._fields_), k
        setattr(p, k, v)
    return p


def same_params(p, **kw):
    q = Params.from_buffer_copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


# the handles of the GPU tests (FusionFunctions.initialize's arguments) as the frame side; the pitch is the caller's
FRAME_64 = dict(width=64, height=32, fx=57.25, fy=55.5, cx=31.3, cy=15.7, near_dist=0.3, far_dist=30.0)
FRAME_100 = dict(width=100, height=52, fx=88.5, fy=91.25, cx=48.7, cy=26.4, near_dist=0.3, far_dist=30.0)


def frame_desc(fr, pitch=None):
    return FrameDesc(fr["width"], fr["height"], pitch or fr["width"], fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["near_dist"], fr["far_dist"])


def pitched(depth, pitch, fill=0.0):
    """tight [h, w] depth -> [h, pitch] with `fill` in the pad columns"""
    out = np.full((depth.shape[0], pitch), fill, f32)
    out[:, :depth.shape[1]] = depth
    return out


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS)


def host_lib():
    global _lib
    if _lib is None:
        out = os.path.join(ROOT, "tests", "_build", "libalign_host.so")
        if _stale(out):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", out + ".tmp"], check=True)
            os.replace(out + ".tmp", out)
        lib = C.CDLL(out)
        cam_p, fr_p, par_p = C.POINTER(rc.Camera), C.POINTER(FrameDesc), C.POINTER(Params)
        lib.align_host_qmax.argtypes = [cam_p]
        lib.align_host_qmax.restype = C.c_float
        lib.align_host_scale.argtypes = [cam_p, C.c_int64]
        lib.align_host_equations.argtypes = [fr_p, _vp, cam_p, _vp, _vp, _vp, par_p, _vp, C.c_int64, _vp, _vp, _vp, _vp]
        lib.align_host_equations_wide.argtypes = [fr_p, _vp, cam_p, _vp, _vp, _vp, par_p, _vp, _vp]
        lib.align_host_frame.argtypes = [fr_p, _vp, cam_p, _vp, _vp, _vp, par_p, C.POINTER(Result)]
        _lib = lib
    return _lib


SANITIZE = rc.SANITIZE


def build_main(out, sanitize=True):
    """align_host.cpp as a stand-alone program (its own main behind ALIGN_HOST_MAIN), with the sanitizers"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DALIGN_HOST_MAIN"] + (SANITIZE if sanitize else []) + [SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def write_case(path, fd, depth, cam, zm, nm):
    """the case file align_host.cpp's main reads"""
    with open(path, "wb") as f:
        f.write(bytes(fd))
        f.write(bytes(rc.as_camera(cam)))
        for a in (depth, zm, nm):
            f.write(np.ascontiguousarray(a, f32).tobytes())


def colmajor(T):
    t = np.asarray(T, f32)
    return np.ascontiguousarray(t.T).ravel() if t.shape == (4, 4) else np.ascontiguousarray(t.reshape(16))


def n_sampled(fd, stride):
    return ((fd.width + stride - 1) // stride) * ((fd.height + stride - 1) // stride)


def host_equations(fd, depth, cam, zm, nm, T, p, order=None, census=False):
    """the checker's evaluation: (sums int64 [29], scale_log2) -- with census=True also (counts [N_EXITS], exit of every sampled pixel)"""
    depth, zm, nm = (np.ascontiguousarray(a, f32) for a in (depth, zm, nm))
    assert depth.shape == (fd.height, fd.pitch) and zm.shape == (cam.height, cam.width) and nm.shape == (cam.height, cam.width, 3)
    t = colmajor(T)
    sums = np.full(N_SUMS, 7, np.int64)
    k = C.c_int32(-7)
    cen = np.zeros(N_EXITS, np.int64)
    ex = np.full(n_sampled(fd, max(p.stride, 1)), -1, np.int8)  # (a stride the checker refuses still gets an array)
    o = None if order is None else np.ascontiguousarray(order, np.int64)
    rcode = host_lib().align_host_equations(C.byref(fd), depth.ctypes.data, C.byref(rc.as_camera(cam)), zm.ctypes.data, nm.ctypes.data, t.ctypes.data,
                                            C.byref(p), None if o is None else o.ctypes.data, 0 if o is None else len(o), sums.ctypes.data,
                                            C.addressof(k), cen.ctypes.data, ex.ctypes.data)
    if rcode:
        return None
    return (sums, k.value, cen, ex) if census else (sums, k.value)


def host_frame(fd, depth, cam, zm, nm, pose_guess, p):
    """the checker's loop over given model planes: a Result, or None when the arguments are refused"""
    depth, zm, nm = (np.ascontiguousarray(a, f32) for a in (depth, zm, nm))
    assert depth.shape == (fd.height, fd.pitch) and zm.shape == (cam.height, cam.width) and nm.shape == (cam.height, cam.width, 3)
    g = colmajor(pose_guess)
    r = Result()
    rcode = host_lib().align_host_frame(C.byref(fd), depth.ctypes.data, C.byref(rc.as_camera(cam)), zm.ctypes.data, nm.ctypes.data, g.ctypes.data,
                                        C.byref(p), C.byref(r))
    return None if rcode else r


def result_fields(r):
    """every field of a Result / api._AlignResult as comparable bytes and values"""
    return {"pose16": bytes(r.pose16), "T16": bytes(r.T16), "status": r.status, "iterations": r.iterations, "n_pixels": r.n_pixels,
            "scale_log2": r.scale_log2, "rms": np.float64(r.rms).tobytes(), "sums": list(r.sums)}


# ------------------------------------------------------------------ the numpy restatement (independent of csrc/dsm_align.h)
def np_ray(u, c, f):
    return (np.asarray(u).astype(f32) - f32(c)) / f32(f)


def np_qmax(cam):
    xa, xb = (abs(np.float64(np_ray(u, cam.cx, cam.fx))) for u in (-1, cam.width))
    ya, yb = (abs(np.float64(np_ray(v, cam.cy, cam.fy))) for v in (-1, cam.height))
    rx, ry = max(xa, xb), max(ya, yb)
    return f32(np.float64(f32(cam.far_dist)) * np.sqrt((rx * rx + ry * ry) + 1.0))


def np_scale(cam, n):
    q = max(float(np_qmax(cam)), 1.0)
    M = 2.0 * q * q
    room = 2.0 ** 62 / float(n)
    for k in range(40, -1, -1):
        if math.ldexp(M, k) + 0.5 <= room:
            return k
    return -1


def np_round_px(u):
    """int(u + 0.5): the sum in double, truncated toward zero; INT_MIN outside int"""
    ud = u.astype(np.float64) + 0.5
    ok = (ud >= -2147483648.0) & (ud < 2147483648.0)
    return np.where(ok, np.trunc(np.where(ok, ud, 0.0)), -2147483648.0).astype(np.int64)


def np_geometry(fd, cam, T, u, v, d):
    """steps 2-5 for arrays of pixels and depths, float32 step by step: q [n, 3], |q|^2, um, vm"""
    t = colmajor(T)
    u, v, d = np.asarray(u), np.asarray(v), np.asarray(d, f32)
    with np.errstate(all="ignore"):
        px, py = np_ray(u, fd.cx, fd.fx) * d, np_ray(v, fd.cy, fd.fy) * d
        q = np.stack([((t[i] * px + t[4 + i] * py) + t[8 + i] * d) + t[12 + i] for i in range(3)], -1).astype(f32)
        q2 = (q[..., 0] * q[..., 0] + q[..., 1] * q[..., 1]) + q[..., 2] * q[..., 2]
        um = np_round_px((q[..., 0] * f32(cam.fx)) / q[..., 2] + f32(cam.cx))
        vm = np_round_px((q[..., 1] * f32(cam.fy)) / q[..., 2] + f32(cam.cy))
    return q, q2, um, vm


def np_equations(fd, depth, cam, zm, nm, T, p, k=None):
    """One evaluation restated: float32 step by step, float64 for the terms, np.rint for the rounding, Python integers for the sums.
    Returns (sums as a list of 29 ints, the exit of every sampled pixel, the weight of every sampled pixel)."""
    cam = rc.as_camera(cam)
    depth, zm, nm = np.asarray(depth, f32), np.asarray(zm, f32), np.asarray(nm, f32)
    if k is None:
        k = np_scale(cam, n_sampled(fd, p.stride))
    V, U = np.meshgrid(np.arange(0, fd.height, p.stride), np.arange(0, fd.width, p.stride), indexing="ij")
    U, V = U.ravel(), V.ravel()
    n = len(U)
    exits = np.full(n, -1, np.int64)
    weight = np.zeros(n)

    def leave(mask, code):
        exits[(exits < 0) & mask] = code

    with np.errstate(all="ignore"):
        d = depth[V, U]
        leave(~(np.isfinite(d) & (d > f32(fd.near_dist)) & (d < f32(fd.far_dist))), X_DEPTH)
        q, q2, um, vm = np_geometry(fd, cam, T, U, V, d)
        leave(~((q[:, 2] > f32(cam.near_dist)) & (q[:, 2] < f32(cam.far_dist))), X_RANGE_Z)
        qmax = np_qmax(cam)
        leave(~(q2 <= qmax * qmax), X_RANGE_Q)
        leave((um < 0) | (um >= cam.width) | (vm < 0) | (vm >= cam.height), X_OUTSIDE)
        uc, vc = np.clip(um, 0, cam.width - 1), np.clip(vm, 0, cam.height - 1)
        z = zm[vc, uc]
        leave(~(z > 0), X_MODEL_DEPTH)
        nn = nm[vc, uc]
        n2 = (nn[:, 0] * nn[:, 0] + nn[:, 1] * nn[:, 1]) + nn[:, 2] * nn[:, 2]
        leave(~((n2 >= f32(0.5)) & (n2 <= f32(2.0))), X_NORMAL)
        e = np.stack([q[:, 0] - np_ray(uc, cam.cx, cam.fx) * z, q[:, 1] - np_ray(vc, cam.cy, cam.fy) * z, q[:, 2] - z], -1).astype(f32)
        e2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        leave(~(e2 <= f32(p.dist_max) * f32(p.dist_max)), X_DISTANCE)
        nq = (nn[:, 0] * q[:, 0] + nn[:, 1] * q[:, 1]) + nn[:, 2] * q[:, 2]
        leave(~(nq * nq >= (f32(p.min_view_cos) * f32(p.min_view_cos)) * q2), X_VIEW_COS)
    ok = exits < 0
    exits[ok] = PASS
    sums = [0] * N_SUMS
    if ok.any():
        n64, q64, e64 = nn[ok].astype(np.float64), q[ok].astype(np.float64), e[ok].astype(np.float64)
        r = (n64[:, 0] * e64[:, 0] + n64[:, 1] * e64[:, 1]) + n64[:, 2] * e64[:, 2]
        J = [n64[:, 0], n64[:, 1], n64[:, 2], q64[:, 1] * n64[:, 2] - q64[:, 2] * n64[:, 1], q64[:, 2] * n64[:, 0] - q64[:, 0] * n64[:, 2],
             q64[:, 0] * n64[:, 1] - q64[:, 1] * n64[:, 0]]
        w = np.ones(len(r))
        hub = np.float64(f32(p.huber))
        if hub > 0:
            ar = np.abs(r)
            big = ar > hub
            w[big] = hub / ar[big]
        weight[ok] = w
        scale = 2.0 ** k

        def fixed(term):
            return int(np.rint(term * scale).astype(np.int64).astype(object).sum())

        s = 0
        for i in range(6):
            wj = w * J[i]
            for j in range(i, 6):
                sums[s] = fixed(wj * J[j])
                s += 1
            sums[21 + i] = fixed(wj * r)
        sums[27] = fixed((w * r) * r)
        sums[28] = int(ok.sum())
    return sums, exits, weight


# ------------------------------------------------------------------ transforms
def rigid(rotvec=(0, 0, 0), t=(0, 0, 0)):
    """4x4 float64 from a rotation vector (Rodrigues) and a translation"""
    w = np.asarray(rotvec, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return m


IDENTITY = np.eye(4, dtype=f32)
CRAFTED_T = rigid((0, 0, 0), (0.01, -0.015, -0.2)).astype(f32)  # the camera moved forward: the frame spills over every model edge
FAR_T = rigid((0, 0, 0), (0.0, 0.0, 0.2)).astype(f32)  # ... and back: depths near the frame's far cross the model's far
WIDE_T = rigid((0, 0, 0), (-2.5, -1.2, -0.05)).astype(f32)  # ... and aside: the frame's far corner leaves the sphere of radius qmax
OBLIQUE_T = rigid((0.02, -0.03, 0.015), (0.03, -0.02, 0.04)).astype(f32)


def pose_error(pose, truth):
    """(translation error in metres, rotation error in degrees) between two cam -> world matrices"""
    d = np.linalg.inv(np.asarray(truth, np.float64)) @ np.asarray(pose, np.float64)
    # |R - I|_F = 2 sqrt(2) sin(angle / 2): linear in the roundings of a float32 pose, where acos((trace - 1) / 2) takes their root
    s = min(np.linalg.norm(d[:3, :3] - np.eye(3)) / (2.0 * np.sqrt(2.0)), 1.0)
    return float(np.linalg.norm(d[:3, 3])), float(np.degrees(2.0 * np.arcsin(s)))


# ------------------------------------------------------------------ crafted planes
CRAFTED_PARAMS = dict(dist_max=0.1, min_view_cos=0.3, huber=0.02)
LATTICE = 6  # crafted pixels sit where u % 6 == 0 and v % 6 == 0: strides 1, 2 and 3 all sample them


def _boundary(pred, lo, hi):
    """adjacent float32 a < b in [lo, hi] with pred(a) != pred(b)"""
    lo, hi = f32(lo), f32(hi)
    assert pred(lo) != pred(hi), (lo, hi)
    while True:
        mid = f32((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            return lo, hi
        if pred(mid) == pred(lo):
            lo = mid
        else:
            hi = mid


def crafted_case(fr=FRAME_64, cam=rc.CAM_70):
    """(tight depth [h, w], zm, nm, cases): cases = [(T, names)] for CRAFTED_T, FAR_T and WIDE_T, names[(u, v)] = (what the pixel is
    for, the exits it may take under that T -- one, but for the pixels whose purpose is to pass an early gate).  Built for
    CRAFTED_PARAMS; every other frame pixel has depth 0."""
    cam = rc.as_camera(cam)
    fd = frame_desc(fr)
    p = params(**CRAFTED_PARAMS)
    T = CRAFTED_T
    depth = np.zeros((fd.height, fd.width), f32)
    zm = np.zeros((cam.height, cam.width), f32)
    nm = np.zeros((cam.height, cam.width, 3), f32)
    names, names_far, names_wide = {}, {}, {}
    past_range_z = (PASS, X_RANGE_Q, X_OUTSIDE, X_MODEL_DEPTH, X_NORMAL, X_DISTANCE, X_VIEW_COS)
    free = [(u, v) for v in range(0, fd.height, LATTICE) for u in range(0, fd.width, LATTICE)]
    taken = set()

    def geo(uv, d):
        q, q2, um, vm = np_geometry(fd, cam, T, uv[0], uv[1], f32(d))
        return q, f32(q2), int(um), int(vm)

    def place(name, exit_, d, uv=None, z_off=0.01, n=(0.0, 0.0, -1.0), z=None):
        """frame pixel uv (the next free lattice pixel) at depth d; the model pixel it lands on shows depth q.z - z_off (or z) and normal n"""
        if uv is None:
            uv = next(c for c in free if c not in names and geo(c, d)[2:] not in taken and 2 <= geo(c, d)[2] < cam.width - 2 and 2 <= geo(c, d)[3] < cam.height - 2)
        assert uv not in names, (name, uv)
        depth[uv[1], uv[0]] = d
        names[uv] = (name, exit_ if isinstance(exit_, tuple) else (exit_,))
        with np.errstate(all="ignore"):
            q, q2, um, vm = geo(uv, d)
        if 0 <= um < cam.width and 0 <= vm < cam.height and np.isfinite(f32(d)):
            assert (um, vm) not in taken, (name, um, vm)
            taken.add((um, vm))
            zm[vm, um] = f32(q[2] - f32(z_off)) if z is None else z
            nm[vm, um] = n
        return uv, q, (um, vm)

    mid = (30, 12)
    # 1. the frame's depth
    place("depth 0", X_DEPTH, 0.0, (0, 12))
    place("depth NaN", X_DEPTH, np.nan, (6, 12))
    place("depth +inf", X_DEPTH, np.inf, (12, 12))
    place("depth -inf", X_DEPTH, -np.inf, (18, 12))
    place("depth = near", X_DEPTH, f32(fd.near_dist), (24, 12))
    place("depth just above near: q.z below the model's near", X_RANGE_Z, np.nextafter(f32(fd.near_dist), f32(1)), (30, 18))
    place("depth = far", X_DEPTH, f32(fd.far_dist), (36, 12))
    place("depth just below far", past_range_z, np.nextafter(f32(fd.far_dist), f32(0)), (30, 12), z_off=0.0)
    # 4. q.z at the model's near and far
    a, b = _boundary(lambda d: geo((36, 18), d)[0][2] > f32(cam.near_dist), 0.4, 0.6)
    place("q.z at the model's near", X_RANGE_Z, a, (36, 18))
    place("q.z just above the model's near", PASS, b, (42, 18), z_off=0.0)
    # (with the same far on both sides q.z reaches the model's far only when T moves the camera back: FAR_T)
    geo_far = lambda uv, d: np_geometry(fd, cam, FAR_T, uv[0], uv[1], f32(d))[0][2]
    a, b = _boundary(lambda d: geo_far((42, 12), d) < f32(cam.far_dist), 29.0, 29.99)
    place("q.z just below the model's far under FAR_T", past_range_z, a, (42, 12))
    place("q.z at the model's far under FAR_T", past_range_z, b, (48, 12))
    names_far[(42, 12)] = ("q.z just below the model's far", past_range_z)
    names_far[(48, 12)] = ("q.z at the model's far", (X_RANGE_Z,))
    # |q| beyond qmax while q.z is below the model's far: the frame's far corner, moved aside (WIDE_T)
    place("the far corner", past_range_z, np.nextafter(f32(fd.far_dist), f32(0)), (0, 0))
    names_wide[(0, 0)] = ("|q| beyond qmax, q.z inside", (X_RANGE_Q,))
    # 5. the .5 boundary of the rounding, and one pixel outside each edge
    um0 = geo((24, 18), 2.0)[2]
    a, b = _boundary(lambda d: geo((24, 18), d)[2] == um0, 1.0, 2.0)
    place("projection on one side of a .5 boundary", PASS, a, (24, 18), z_off=0.0)
    a2, b2 = _boundary(lambda d: geo((18, 18), d)[2] == geo((18, 18), 2.0)[2], 1.0, 2.0)
    place("projection on the other side of a .5 boundary", PASS, b2, (18, 18), z_off=0.0)
    assert geo((24, 18), a)[2] != geo((24, 18), b)[2] and geo((18, 18), a2)[2] != geo((18, 18), b2)[2]

    def edge(name, uv, want, axis, lo, hi):
        a, b = _boundary(lambda d: (geo(uv, d)[2 + axis] >= want) if want <= 0 else (geo(uv, d)[2 + axis] <= want), lo, hi)
        d = a if geo(uv, a)[2 + axis] == want else b
        assert geo(uv, d)[2 + axis] == want, (name, geo(uv, a), geo(uv, b))
        place(name, X_OUTSIDE, d, uv)

    edge("one pixel left of the model image", (0, 18), -1, 0, 0.55, 5.0)
    edge("one pixel right of the model image", (60, 18), cam.width, 0, 0.55, 5.0)
    edge("one pixel above the model image", (30, 0), -1, 1, 0.55, 5.0)
    edge("one pixel below the model image", (30, 30), cam.height, 1, 0.55, 5.0)
    # 6. the model's depth
    place("model depth 0", X_MODEL_DEPTH, 2.0, z=f32(0.0))
    place("model depth NaN", X_MODEL_DEPTH, 2.1, z=f32(np.nan))
    place("model depth negative", X_MODEL_DEPTH, 2.2, z=f32(-2.0))
    # 7. the normal
    place("zero normal", X_NORMAL, 2.3, n=(0, 0, 0))
    place("NaN normal", X_NORMAL, 2.4, n=(0, np.nan, -1))
    lo, hi = _boundary(lambda s: f32(s) * f32(s) >= f32(0.5), 0.6, 0.8)
    place("normal of length^2 just below 0.5", X_NORMAL, 2.5, n=(0, 0, -lo))
    place("normal of length^2 0.5", PASS, 2.6, n=(0, 0, -hi))
    lo, hi = _boundary(lambda s: f32(s) * f32(s) <= f32(2.0), 1.3, 1.5)
    place("normal of length^2 2", PASS, 2.7, n=(0, 0, -lo))
    place("normal of length^2 just above 2", X_NORMAL, 2.8, n=(0, 0, -hi))
    place("non-unit normal inside the band", PASS, 2.9, n=(0.3, -0.2, -1.1))
    # 8. the distance gate: the offset along z at which |e|^2 crosses dist_max^2
    for name, exit_, side in (("|e|^2 just inside dist_max^2", PASS, 0), ("|e|^2 just outside dist_max^2", X_DISTANCE, 1)):
        d = 1.6 + 0.1 * side
        uv = next(c for c in free if c not in names and geo(c, d)[2:] not in taken and 2 <= geo(c, d)[2] < cam.width - 2 and 2 <= geo(c, d)[3] < cam.height - 2)
        q, _, um, vm = geo(uv, d)

        def inside(off):
            z = f32(q[2] - f32(off))
            e = np.array([q[0] - np_ray(um, cam.cx, cam.fx) * z, q[1] - np_ray(vm, cam.cy, cam.fy) * z, q[2] - z], f32)
            return bool((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2] <= f32(p.dist_max) * f32(p.dist_max))

        lo, hi = _boundary(inside, 0.0, 0.2)
        place(name, exit_, d, uv, z_off=(lo, hi)[side], n=(0.0, 0.8, -0.6))
    # 9. the view-cos gate: a normal turned away from the ray until (n . q)^2 crosses min_view_cos^2 |q|^2
    for name, exit_, side in (("view-cos gate just inside", PASS, 0), ("view-cos gate just outside", X_VIEW_COS, 1)):
        d = 1.2 + 0.1 * side
        uv = next(c for c in free if c not in names and geo(c, d)[2:] not in taken and 2 <= geo(c, d)[2] < cam.width - 2 and 2 <= geo(c, d)[3] < cam.height - 2)
        q, q2, um, vm = geo(uv, d)
        qh = q.astype(np.float64) / np.linalg.norm(q.astype(np.float64))
        perp = np.cross(qh, [0.0, 1.0, 0.0])
        perp /= np.linalg.norm(perp)

        def normal(th):
            return (-np.cos(np.float64(th)) * qh + np.sin(np.float64(th)) * perp).astype(f32)

        def inside(th):
            n = normal(th)
            nq = (n[0] * q[0] + n[1] * q[1]) + n[2] * q[2]
            return bool(nq * nq >= (f32(p.min_view_cos) * f32(p.min_view_cos)) * q2)

        lo, hi = _boundary(inside, 1.0, 1.5)
        place(name, exit_, d, uv, z_off=0.0, n=tuple(normal((lo, hi)[side])))
    # 10. |r| on both sides of huber: n = (0, 0, -1), so r = -(q.z - zm) exactly
    for name, side in (("|r| just inside huber", 0), ("|r| just outside huber", 1)):
        d = 1.4 + 0.1 * side
        uv = next(c for c in free if c not in names and geo(c, d)[2:] not in taken and 2 <= geo(c, d)[2] < cam.width - 2 and 2 <= geo(c, d)[3] < cam.height - 2)
        q = geo(uv, d)[0]
        lo, hi = _boundary(lambda off: abs(np.float64(f32(q[2] - f32(q[2] - f32(off))))) <= np.float64(f32(p.huber)), 0.0, 0.05)
        place(name, PASS, d, uv, z_off=(lo, hi)[side])
    # and plain passing pixels with tilted normals, so that the sums have six dimensions
    for i in range(12):
        a, b = 0.5 * np.cos(1.3 * i), 0.5 * np.sin(2.1 * i)
        n = np.array([a, b, -1.0]) / np.sqrt(a * a + b * b + 1.0)
        place("ordinary %d" % i, PASS, 1.0 + 0.17 * i, z_off=0.004 * (i - 5), n=tuple(n))
    return depth, zm, nm, [(CRAFTED_T, names), (FAR_T, names_far), (WIDE_T, names_wide)]


def sampled_index(fd, stride, u, v):
    """the position of frame pixel (u, v) among the sampled pixels, row-major"""
    assert u % stride == 0 and v % stride == 0
    return (v // stride) * ((fd.width + stride - 1) // stride) + u // stride


# ------------------------------------------------------------------ random planes
def random_planes(rng, fr, cam, garbage=True):
    """a frame and a model that mostly agree (a surface about 2 m away seen through a small transform), sprinkled with zeros,
    infinities, NaNs, arbitrary bits, normals across the length band and depths near the gates: (tight depth, zm, nm)"""
    cam = rc.as_camera(cam)
    h, w = fr["height"], fr["width"]
    depth = (2.0 + 0.3 * np.sin(np.arange(w) / 9.0)[None, :] + rng.normal(0, 0.02, (h, w))).astype(f32)
    zm = (2.0 + 0.3 * np.sin(np.arange(cam.width) / 9.5)[None, :] + rng.normal(0, 0.02, (cam.height, cam.width))).astype(f32)
    nn = np.concatenate([rng.normal(0, 0.3, (cam.height, cam.width, 2)), -np.ones((cam.height, cam.width, 1))], -1)
    nn /= np.linalg.norm(nn, axis=-1, keepdims=True)
    nm = (nn * rng.uniform(0.65, 1.48, (cam.height, cam.width, 1))).astype(f32)
    if garbage:
        for plane, vals in ((depth, (0.0, np.nan, np.inf, -1.0, 0.3, 29.9, 31.0, 1e-30)), (zm, (0.0, np.nan, np.inf, -2.0, 1e-30, 25.0))):
            for val in vals:
                plane[rng.random(plane.shape) < 0.01] = val
        bits = rng.integers(0, 2 ** 32, nm.shape, dtype=np.uint64).astype(np.uint32).view(f32)
        pick = rng.random(nm.shape[:2]) < 0.03
        nm[pick] = bits[pick]
        nm[rng.random(nm.shape[:2]) < 0.01] = 0.0
    return depth, zm, nm


# ------------------------------------------------------------------ the room corner: a floor and two walls
ROOM_PLANES = (((0.0, 1.0, 0.0), 0.3),                                # the floor y = 0.3 (y points down)
               ((math.sqrt(0.5), 0.0, math.sqrt(0.5)), 3.0 * math.sqrt(0.5)),   # the wall x + z = 3
               ((-math.sqrt(0.5), 0.0, math.sqrt(0.5)), 3.0 * math.sqrt(0.5)))  # the wall -x + z = 3


def room_surfels(surfel_dtype, planes=ROOM_PLANES, spacing=0.04):
    """surfels on the planes n . x = c, a grid of `spacing`, radius 0.9 spacing (the discs cover the plane), normals towards the origin"""
    out = []
    for n, c in planes:
        n = np.asarray(n, np.float64)
        a = np.cross(n, [0.0, 0.0, 1.0] if abs(n[2]) < 0.9 else [1.0, 0.0, 0.0])
        a /= np.linalg.norm(a)
        b = np.cross(n, a)
        g = np.arange(-3.2, 3.2, spacing)
        A, B = np.meshgrid(g, g)
        pts = c * n + A.reshape(-1, 1) * a + B.reshape(-1, 1) * b
        # what a camera near the origin can see of the room: in front of it, inside the other planes
        keep = (pts[:, 2] > 0.2) & (pts[:, 1] > -1.4)
        for m, cc in planes:
            keep &= pts @ np.asarray(m) <= cc + 1e-9
        pts = pts[keep]
        s = np.zeros(len(pts), surfel_dtype)
        s["px"], s["py"], s["pz"] = pts.T
        s["nx"], s["ny"], s["nz"] = -n
        s["size"] = 0.9 * spacing
        s["color"], s["weight"], s["update_times"], s["last_update"] = 100.0, 1.0, 7, 1
        out.append(s)
    return np.concatenate(out)


def room_depth(fr, pose, planes=ROOM_PLANES):
    """the analytic depth image of the room for a camera at `pose` (cam -> world): the nearest plane along every pixel's ray"""
    P = np.asarray(pose, np.float64)
    V, U = np.meshgrid(np.arange(fr["height"]), np.arange(fr["width"]), indexing="ij")
    ray = np.stack([(U - np.float64(f32(fr["cx"]))) / np.float64(f32(fr["fx"])), (V - np.float64(f32(fr["cy"]))) / np.float64(f32(fr["fy"])), np.ones(U.shape)], -1)
    dw = ray @ P[:3, :3].T
    best = np.full(U.shape, np.inf)
    for n, c in planes:
        n = np.asarray(n, np.float64)
        with np.errstate(all="ignore"):
            t = (c - n @ P[:3, 3]) / (dw @ n)
        t = np.where(t > 0, t, np.inf)
        best = np.minimum(best, t)
    return np.where(np.isfinite(best), best, 0.0).astype(f32)


ROOM_TRUTH = rigid((0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
# 30 mm and 1.5 degrees off
ROOM_GUESS = rigid(np.radians(1.5) * np.array([0.6, -0.64, 0.48]), 0.03 * np.array([0.48, 0.6, -0.64]))
# The input is noise-free, yet the fixed point is not the truth to the last place: a frame pixel within a pixel of a crease can land
# on a model pixel that shows the OTHER plane, and its residual at the truth is its distance from that plane -- up to 3 cm here, 5.8 mm
# rms over the image (some 90 of 2048 pixels).  A Huber width of a millimetre, fit for noise-free input, lets those pixels weigh little:
# the loop ends 0.10 mm and 0.006 degrees from the truth (0.05 m: 1.9 mm and 0.10 degrees; the error is proportional to the width).
ROOM_PARAMS = dict(max_iterations=30, stride=1, dist_max=0.25, min_view_cos=0.1, huber=0.001, min_pixels=200, stop_translation=1e-5, stop_rotation=1e-5)
