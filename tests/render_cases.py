"""Shared by tests/test_cpu_render.py and tests/test_gpu_render.py: the host build of the renderer's definition
(tests/render_host.cpp: the boxed and the brute-force renderer over csrc/dsm_math.h's render_setup / render_hit / render_key),
cameras, poses and the crafted records."""
import ctypes as C
import os
import subprocess

import numpy as np

import mesh_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CULL_BACKFACES = 1
PLANES = ("depth", "index", "normal", "intensity")
SRC = os.path.join(ROOT, "tests", "render_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "densesurfelmapping_amd", "csrc", "dsm_math.h"), os.path.join(ROOT, "include", "dsm.h")]

_lib = None
_vp = C.c_void_p


class Camera(C.Structure):
    """dsm_render_camera of include/dsm.h"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("near_dist", C.c_float), ("far_dist", C.c_float)]


# widths that are no multiple of 16 or 64
CAM_70 = Camera(70, 37, 60.5, 58.25, 34.3, 18.1, 0.3, 30.0)
CAM_96 = Camera(96, 64, 83.0, 85.5, 47.6, 31.2, 0.3, 30.0)
CAM_48 = Camera(48, 32, 40.5, 38.25, 23.3, 15.6, 0.3, 30.0)


def as_camera(c):
    """any object with dsm_render_camera's fields (api._RenderCamera for one) as a Camera"""
    return c if isinstance(c, Camera) else Camera(*(getattr(c, f[0]) for f in Camera._fields_))


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS)


def host_lib():
    global _lib
    if _lib is None:
        out = os.path.join(ROOT, "tests", "_build", "librender_host.so")
        if _stale(out):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", out + ".tmp"], check=True)
            os.replace(out + ".tmp", out)
        lib = C.CDLL(out)
        lib.render_host.argtypes = [_vp, C.c_int64, C.POINTER(Camera), _vp, C.c_uint32, C.c_int, C.c_int, _vp, _vp, _vp, _vp]
        lib.render_host.restype = None
        lib.render_host_boxes.argtypes = [_vp, C.c_int64, C.POINTER(Camera), _vp, C.c_uint32, C.c_int, _vp, _vp]
        lib.render_host_boxes.restype = None
        lib.render_host_inverse.argtypes = [_vp, _vp]
        lib.render_host_inverse.restype = None
        _lib = lib
    return _lib


# (the runtimes linked statically: the program then runs the same whatever else the process environment preloads)
SANITIZE = ["-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def build_main(out, sanitize=True):
    """render_host.cpp as a stand-alone program (its own main behind RENDER_HOST_MAIN), with the sanitizers"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DRENDER_HOST_MAIN"] + (SANITIZE if sanitize else []) + [SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def pose_colmajor(pose):
    """4x4 row-major cam -> world matrix (or 16 column-major floats) -> 16 column-major float32"""
    p = np.asarray(pose, np.float32)
    return np.ascontiguousarray(p.T).ravel() if p.shape == (4, 4) else np.ascontiguousarray(p.reshape(16))


def closed_form_inverse(pose):
    p = pose_colmajor(pose)
    inv = np.zeros(16, np.float32)
    host_lib().render_host_inverse(p.ctypes.data, inv.ctypes.data)
    return inv


def host_render(surfels, cam, pose, inv=None, flags=0, eigen33=False, brute=True):
    """the planes of the sequence `surfels` (already in render order) as a dict of numpy arrays"""
    s = np.ascontiguousarray(surfels)
    assert s.dtype.itemsize == 44
    cam = as_camera(cam)
    inv16 = closed_form_inverse(pose) if inv is None else pose_colmajor(inv)
    h, w = cam.height, cam.width
    out = {"depth": np.full((h, w), 7.0, np.float32), "index": np.full((h, w), 7, np.int32),
           "normal": np.full((h, w, 3), 7.0, np.float32), "intensity": np.full((h, w), 7, np.uint8)}
    host_lib().render_host(s.ctypes.data, len(s), C.byref(cam), inv16.ctypes.data, flags, int(eigen33), int(brute),
                           out["depth"].ctypes.data, out["index"].ctypes.data, out["normal"].ctypes.data, out["intensity"].ctypes.data)
    return out


def host_boxes(surfels, cam, pose, flags=0, eigen33=False):
    """(boxes (n, 4) int32 x0 y0 x1 y1, keep (n,) bool): render_setup's verdict on every record"""
    s = np.ascontiguousarray(surfels)
    cam = as_camera(cam)
    inv16 = closed_form_inverse(pose)
    box = np.zeros((len(s), 4), np.int32)
    keep = np.zeros(len(s), np.uint8)
    if len(s):
        host_lib().render_host_boxes(s.ctypes.data, len(s), C.byref(cam), inv16.ctypes.data, flags, int(eigen33), box.ctypes.data, keep.ctypes.data)
    return box, keep.astype(bool)


def same_planes(got, exp, what=""):
    """bit for bit on every plane both hold (NaN == NaN; no plane of a render can hold one, so that never excuses anything)"""
    for k in PLANES:
        if k in got and k in exp:
            a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
            assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
            if a.dtype == np.uint8:
                bad = np.argwhere(a != b)
                assert bad.size == 0, (what, k, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])
            else:
                mc.same_bits(a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1), (what, k))


def keep_select(m, select):
    if select == 0:
        return m[:0]
    return m[m["update_times"] >= 5] if select == 1 else m[m["update_times"] != 0]


IDENTITY = np.eye(4, dtype=np.float32)


def oblique_pose():
    """a camera turned about two axes and moved off the origin (cam -> world, 4x4 row-major)"""
    a, b = 0.35, -0.2
    ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
    p = np.eye(4)
    p[:3, :3] = ry @ rx
    p[:3, 3] = (0.3, -0.2, 0.4)
    return p.astype(np.float32)


def crafted_records(surfel_dtype, cam=CAM_70):
    """the records the definition's edge cases turn on, placed for `cam` at the identity pose; returns (records, names)"""
    rows, names = [], []

    def add(name, **kw):
        r = dict(px=0.0, py=0.0, pz=2.0, nx=0.0, ny=0.0, nz=-1.0, size=0.25, color=128.0, weight=1.0, update_times=7, last_update=1)
        r.update(kw)
        rows.append(r)
        names.append(name)

    w, h = cam.width, cam.height

    def at(fu, fv, z):  # the point of depth z on the ray of pixel (fu (w - 1), fv (h - 1)), rounded to a pixel
        u, v = round(fu * (w - 1)), round(fv * (h - 1))
        return dict(px=(u - cam.cx) / cam.fx * z, py=(v - cam.cy) / cam.fy * z, pz=z)

    def unit(x, y, z):
        n = np.array([x, y, z], np.float64)
        n /= np.linalg.norm(n)
        return dict(nx=n[0], ny=n[1], nz=n[2])

    add("fronto-parallel", **at(0.3, 0.3, 2.0), size=0.1, color=10.0)
    add("fronto-parallel, normal towards +z", **at(0.45, 0.7, 2.5), nz=1.0, size=0.12, color=20.0)
    add("tilted", **at(0.65, 0.25, 1.5), **unit(0.5, 0.2, -0.8), size=0.1, color=30.0)
    add("tilted 75 degrees", **at(0.75, 0.75, 1.8), **unit(0.9659, 0.0, -0.2588), size=0.15, color=40.0)
    add("edge-on through the centre: denominator 0 on its column", px=0.0, py=0.0, pz=2.0, nx=1.0, ny=0.0, nz=0.0)
    add("edge-on plane x = 0.5", px=0.5, py=-0.3, pz=2.0, nx=1.0, ny=0.0, nz=0.0, size=0.1, color=50.0)
    add("zero normal", nx=0.0, ny=0.0, nz=0.0)
    add("minus-zero normal", nx=-0.0, ny=-0.0, nz=-0.0)
    add("behind the camera", pz=-2.0)
    add("behind the camera, tilted, large", pz=-0.5, **unit(0.3, 0.3, 0.9), size=3.0)
    add("straddles the near plane", **at(0.08, 0.9, cam.near_dist), **unit(0.6, 0.0, -0.8), size=0.03, color=60.0)
    add("straddles the far plane", **at(0.2, 0.12, cam.far_dist), **unit(0.0, 0.6, -0.8), size=3.0, color=70.0)
    add("left border", **at(0.0, 0.5, 3.0), size=0.12, color=80.0)
    add("right border", **at(1.0, 0.3, 2.0), size=0.1, color=90.0)
    add("top border", **at(0.5, 0.0, 3.0), size=0.12, color=100.0)
    add("bottom border", **at(0.35, 1.0, 3.0), size=0.12, color=110.0)
    add("corner", **at(1.0, 1.0, 2.0), **unit(0.2, 0.2, -0.9), size=0.1, color=120.0)
    add("wholly outside, left", **at(-0.6, 0.3, 2.0))
    add("size 0", **at(0.1, 0.1, 2.0), size=0.0)
    add("size 0 off the rays", px=0.0123, py=0.0456, pz=2.0, size=0.0)
    add("negative size", **at(0.15, 0.55, 2.0), size=-0.08, color=130.0)
    add("inf size", pz=29.8, size=np.inf, color=140.0)
    add("-inf size", pz=29.85, size=-np.inf, color=141.0)
    add("NaN size", size=np.nan)
    add("huge size: the square overflows", pz=29.9, size=1e30, color=142.0)
    add("denormal size", size=float(np.float32(1e-42)))
    add("NaN position", px=np.nan)
    add("inf position", py=np.inf)
    add("-inf depth", pz=-np.inf)
    add("NaN normal", ny=np.nan)
    add("inf normal", nz=-np.inf)
    add("huge finite position", px=3e38, py=-3e38, pz=3e38)
    add("covers the whole image", pz=29.5, nz=1.0, size=80.0, color=150.0)
    add("the camera centre in the disc's plane, exactly", px=0.0, py=0.0, pz=1.0, nx=1.0, ny=0.0, nz=0.0, size=5.0)
    add("the camera centre almost in the disc's plane", px=0.2, py=0.1, pz=1.0, **unit(1.0, 0.0, -0.2), size=5.0, color=160.0)
    add("the camera centre inside a disc's reach: the plane x = 2.5", px=2.5, py=0.0, pz=0.5, nx=1.0, ny=0.0, nz=0.0, size=9.0, color=170.0)
    add("duplicate a", **at(0.55, 0.5, 1.2), **unit(0.1, -0.3, -0.9), size=0.06, color=180.0)
    add("duplicate b", **at(0.55, 0.5, 1.2), **unit(0.1, -0.3, -0.9), size=0.06, color=181.0)
    add("update_times 0", **at(0.2, 0.85, 1.0), size=0.04, update_times=0, color=190.0)
    add("update_times 4", **at(0.3, 0.85, 1.0), size=0.04, update_times=4, color=200.0)
    add("update_times 5", **at(0.4, 0.85, 1.0), size=0.04, update_times=5, color=210.0)
    add("colour NaN", **at(0.8, 0.5, 1.0), size=0.04, color=np.nan)
    add("colour 300", **at(0.87, 0.5, 1.0), size=0.04, color=300.0)
    add("colour -3", **at(0.94, 0.5, 1.0), size=0.04, color=-3.0)
    a = np.zeros(len(rows), surfel_dtype)
    for i, r in enumerate(rows):
        for k, v in r.items():
            a[k][i] = v
    return a, names


def render_records(rng, n, surfel_dtype, ut=None):
    """finite surfels in front of a camera at the origin looking down +z: every one a candidate for a pixel"""
    a = np.zeros(n, surfel_dtype)
    z = rng.uniform(0.2, 6.0, n)
    a["px"], a["py"], a["pz"] = rng.uniform(-0.7, 0.7, n) * z, rng.uniform(-0.5, 0.5, n) * z, z
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a["nx"], a["ny"], a["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    a["size"] = rng.uniform(0.005, 0.12, n) * z
    a["color"] = rng.uniform(-20, 300, n)
    a["weight"] = rng.uniform(0, 50, n)
    a["update_times"] = ut if ut is not None else rng.integers(0, 12, n)
    a["last_update"] = rng.integers(0, 8, n)
    return a


def mixed_records(rng, n, surfel_dtype, ut=None):
    """a third arbitrary bit patterns, two thirds surfels a camera at the origin can see, interleaved at random"""
    a = mc.random_records(rng, n, surfel_dtype, ut)
    b = render_records(rng, n, surfel_dtype, ut)
    pick = rng.random(n) < 0.67
    a[pick] = b[pick]
    return a
