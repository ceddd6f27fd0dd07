"""Shared by tests/test_cpu_mesh.py and tests/test_gpu_mesh.py: the host build of the mesh arithmetic (tests/mesh_host.cpp),
a numpy restatement of the reference's push_a_surfel, crafted records, and a reader for the binary PLY."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF6, XYZ_RGBA8 = 0, 1
FLOATS = {REF6: 36, XYZ_RGBA8: 24}
FACES = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [4, 3, 5]], np.int64)  # surfel_map.cpp:1274-1277
INT_MIN = -2 ** 31

_lib = None


def host_lib():
    """tests/mesh_host.cpp: csrc/dsm_math.h's surfel_hexagon and csrc/dsm_mesh_ply.h for the host, no FMA contraction"""
    global _lib
    if _lib is None:
        out = os.path.join(ROOT, "tests", "_build", "libmesh_host.so")
        src = os.path.join(ROOT, "tests", "mesh_host.cpp")
        deps = [src, os.path.join(ROOT, "densesurfelmapping_amd", "csrc", "dsm_math.h"),
                os.path.join(ROOT, "densesurfelmapping_amd", "csrc", "dsm_mesh_ply.h"), os.path.join(ROOT, "include", "dsm.h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out + ".tmp"], check=True)
            os.replace(out + ".tmp", out)
        lib = C.CDLL(out)
        lib.mesh_host_vertices.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
        lib.mesh_host_vertices.restype = None
        lib.mesh_host_color_int.argtypes = [C.c_float]
        lib.mesh_host_print.argtypes = [C.c_char_p, C.c_void_p, C.c_int64]
        lib.mesh_host_ply_binary.argtypes = [C.c_char_p, C.c_void_p, C.c_int64]
        _lib = lib
    return _lib


def host_vertices(surfels, layout=REF6):
    """(n, 36) or (n, 24) float32: the host corner function on every record"""
    s = np.ascontiguousarray(surfels)
    assert s.dtype.itemsize == 44
    out = np.zeros((len(s), FLOATS[layout]), np.float32)
    if len(s):
        host_lib().mesh_host_vertices(s.ctypes.data, len(s), layout, out.ctypes.data)
    return out


def print_ref6(path, ref6):
    v = np.ascontiguousarray(ref6, np.float32).reshape(-1, 36)
    assert host_lib().mesh_host_print(str(path).encode(), v.ctypes.data, len(v)) == 0


def same_bits(a, b, what=""):
    """bit for bit, NaN == NaN; rows of 4-byte words"""
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not a.size:
        return
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    same = ua == ub
    if a.dtype == np.float32:
        same |= np.isnan(a) & np.isnan(b)
    bad = np.argwhere(~same)
    assert bad.size == 0, (what, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])


def same_vertices(a, b, layout, what=""):
    """vertex buffers: floats bit for bit with NaN == NaN; the RGBA word of XYZ_RGBA8 (which may look like a NaN) exactly"""
    a = np.ascontiguousarray(a, np.float32).reshape(-1, FLOATS[layout])
    b = np.ascontiguousarray(b, np.float32).reshape(-1, FLOATS[layout])
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if layout == XYZ_RGBA8 and a.size:
        a4, b4 = a.reshape(-1, 4), b.reshape(-1, 4)
        same_bits(a4[:, :3], b4[:, :3], what)
        same_bits(a4[:, 3].view(np.uint32), b4[:, 3].view(np.uint32), (what, "rgba"))
    else:
        same_bits(a, b, what)


def np_color_int(color):
    """(int)color of the reference's x86 build: cvttss2si, INT_MIN for a NaN and outside int"""
    c = np.asarray(color, np.float32)
    with np.errstate(all="ignore"):
        ok = (c >= np.float32(-2147483648.0)) & (c < np.float32(2147483648.0))
        return np.where(ok, np.trunc(np.where(ok, c, 0)).astype(np.int64), INT_MIN).astype(np.int32)


def np_hexagon(s):
    """SurfelMap::push_a_surfel (surfel_fusion/src/surfel_map.cpp:1176-1216), statement by statement, in numpy float32 /
    float64 (one rounding per operation, nothing contracted): (n, 36) float32 in the layout of `vertexs`"""
    f32, f64 = np.float32, np.float64
    n = len(s)
    with np.errstate(all="ignore"):
        surfel_color = np_color_int(s["color"])                                   # int surfel_color = this_surfel.color
        pos = [s["px"].astype(f32), s["py"].astype(f32), s["pz"].astype(f32)]     # Vector3f surfel_position
        nrm = [s["nx"].astype(f32), s["ny"].astype(f32), s["nz"].astype(f32)]     # Vector3f surfel_norm
        x_dir = [f32(-1) * nrm[1], nrm[0].copy(), np.zeros(n, f32)]               # x_dir << -1 * ny, nx, 0
        z = x_dir[0] * x_dir[0] + (x_dir[1] * x_dir[1] + x_dir[2] * x_dir[2])     # x_dir.normalize(): squaredNorm ...
        nn = np.sqrt(z)
        x_dir = [np.where(z > 0, x / nn, x) for x in x_dir]                       # ... / sqrt when positive
        y_dir = [nrm[1] * x_dir[2] - nrm[2] * x_dir[1],                           # y_dir = surfel_norm.cross(x_dir)
                 nrm[2] * x_dir[0] - nrm[0] * x_dir[2],
                 nrm[0] * x_dir[1] - nrm[1] * x_dir[0]]
        radius = s["size"].astype(f32)
        h_r = (radius.astype(f64) * f64(0.5)).astype(f32)                         # float h_r = radius * 0.5
        t_r = (radius.astype(f64) * f64(0.86603)).astype(f32)                     # float t_r = radius * 0.86603
        out = np.zeros((n, 6, 6), f32)
        for i in range(3):
            out[:, 0, i] = (pos[i] - x_dir[i] * h_r) - y_dir[i] * t_r
            out[:, 1, i] = (pos[i] + x_dir[i] * h_r) - y_dir[i] * t_r
            out[:, 2, i] = pos[i] - x_dir[i] * radius
            out[:, 3, i] = pos[i] + x_dir[i] * radius
            out[:, 4, i] = (pos[i] - x_dir[i] * h_r) + y_dir[i] * t_r
            out[:, 5, i] = (pos[i] + x_dir[i] * h_r) + y_dir[i] * t_r
        out[:, :, 3:] = surfel_color.astype(f32)[:, None, None]                   # push_back(surfel_color) x 3, as float
    return out.reshape(n, 36)


def ref6_to_rgba8(ref6):
    """what the XYZ_RGBA8 layout must hold for a REF6 buffer: positions as they are, bytes r g b 255 = the int colour clamped"""
    v = np.ascontiguousarray(ref6, np.float32).reshape(-1, 6)
    out = np.zeros((len(v), 4), np.float32)
    out[:, :3] = v[:, :3]
    with np.errstate(all="ignore"):
        b = np.clip(np.where(np.isnan(v[:, 3]), 0, v[:, 3]), 0, 255).astype(np.uint32)
    out[:, 3] = (b | (b << 8) | (b << 16) | np.uint32(0xff000000)).astype(np.uint32).view(np.float32)
    return out.reshape(-1, 24)


def random_records(rng, n, surfel_dtype, ut=None):
    """arbitrary bit patterns in every float field (NaN payloads, inf, denormals), update_times from an adversarial set --
    _random_map of tests/test_gpu_clouds.py"""
    a = np.zeros(n, surfel_dtype)
    raw = rng.integers(0, 1 << 32, size=(n, 11), dtype=np.uint64).astype(np.uint32)
    for k, f in enumerate(("px", "py", "pz", "nx", "ny", "nz", "size", "color", "weight")):
        a[f] = raw[:, k].view(np.float32)
    a["update_times"] = ut if ut is not None else rng.choice(np.array([0, 1, 4, 5, 6, -1, -5, 2**31 - 1, -2**31, 100], np.int32), n)
    a["last_update"] = rng.integers(0, 8, n)
    return a


def plausible_records(rng, n, surfel_dtype, ut=None):
    """finite records of ordinary magnitude: every corner is a number, so the arithmetic (not the NaN mask) is compared"""
    a = np.zeros(n, surfel_dtype)
    for f in ("px", "py", "pz"):
        a[f] = rng.normal(0, 20, n)
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    a["nx"], a["ny"], a["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    a["size"] = rng.uniform(1e-3, 2.0, n)
    a["color"] = rng.uniform(-20, 300, n)
    a["weight"] = rng.uniform(0, 50, n)
    a["update_times"] = ut if ut is not None else rng.integers(0, 12, n)
    a["last_update"] = rng.integers(0, 8, n)
    return a


CRAFTED_COLORS = [0.0, 255.9, -1.0, 300.0, np.nan, 3e9, -3e9, 2147483520.0, 2147483648.0, -2147483648.0, -0.5, np.inf, -np.inf]


def crafted_records(surfel_dtype):
    """the records the edge cases of push_a_surfel turn on; returns (records, names)"""
    f32 = np.float32
    rows, names = [], []

    def add(name, **kw):
        r = dict(px=1.5, py=-2.25, pz=3.125, nx=0.6, ny=0.0, nz=0.8, size=0.37, color=128.0, weight=1.0, update_times=7, last_update=1)
        r.update(kw)
        rows.append(r)
        names.append(name)

    add("nx = ny = 0", nx=0.0, ny=0.0, nz=1.0)
    add("nx = ny = -0", nx=-0.0, ny=-0.0, nz=-1.0)
    add("nx = +0, ny = -0", nx=0.0, ny=-0.0, nz=1.0)
    add("nz = -0", nx=0.3, ny=-0.4, nz=-0.0)
    add("all normals -0", nx=-0.0, ny=-0.0, nz=-0.0)
    add("denormal normal: z underflows to 0", nx=1e-30, ny=-1e-30, nz=1.0)
    add("denormal normal: z a denormal", nx=1e-20, ny=3e-23, nz=1.0)
    add("huge normal: z overflows", nx=3e20, ny=1e25, nz=1.0)
    add("denormal size", size=float(f32(1e-42)))
    add("smallest denormal size", size=float(np.uint32(1).view(f32)))
    add("inf size", size=np.inf)
    add("-inf size", size=-np.inf)
    add("zero size", size=0.0)
    add("NaN size", size=np.nan)
    add("NaN nx", nx=np.nan)
    add("NaN ny", ny=np.nan)
    add("NaN nz", nz=np.nan)
    add("inf nx", nx=np.inf)
    add("NaN position", px=np.nan)
    for c in CRAFTED_COLORS:
        add("colour %r" % c, color=c)
    a = np.zeros(len(rows), surfel_dtype)
    for i, r in enumerate(rows):
        for k, v in r.items():
            a[k][i] = v
    return a, names


def read_ply_binary(path):
    """(positions (n_vertices, 3) float32, colours (n_vertices, 3) uint8, faces (n_faces, 3) int32, header lines)"""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    nv = int([ln for ln in head if ln.startswith("element vertex")][0].split()[2])
    nf = int([ln for ln in head if ln.startswith("element face")][0].split()[2])
    assert len(data) == end + nv * 15 + nf * 13, (len(data), end, nv, nf)
    vt = np.dtype([("p", "<f4", 3), ("c", "u1", 3)])
    ft = np.dtype([("k", "u1"), ("i", "<i4", 3)])
    assert vt.itemsize == 15 and ft.itemsize == 13
    v = np.frombuffer(data, vt, nv, end)
    f = np.frombuffer(data, ft, nf, end + nv * 15)
    assert (f["k"] == 3).all()
    return v["p"].copy(), v["c"].copy(), f["i"].copy(), head


def expect_faces(n_surfels):
    return (np.arange(n_surfels, dtype=np.int64)[:, None, None] * 6 + FACES[None]).reshape(-1, 3)
