"""Shared by tests/test_cpu_grid.py and tests/test_gpu_grid.py: the host build of the voxel grid's definition (tests/grid_host.cpp:
the boxed and the brute-force voxelisation over csrc/dsm_math.h's grid_setup / grid_covers / grid_centre, the brute-force
inflation, the cell list), the grids, the crafted records, the random records and the bit sets of the inflation cases."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CELLS_OF_INFLATED = 1
SRC = os.path.join(ROOT, "tests", "grid_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "densesurfelmapping_amd", "csrc", "dsm_math.h"), os.path.join(ROOT, "densesurfelmapping_amd", "csrc", "dsm_align.h"),
        os.path.join(ROOT, "include", "dsm.h")]
SMALL_W, SMALL_ROWS = 16, 256  # kGridSmallW, kGridSmallRows of csrc/dsm_device.h
f32 = np.float32

_lib = None
_vp = C.c_void_p


class Spec(C.Structure):
    """dsm_grid_spec of include/dsm.h"""
    _fields_ = [("struct_size", C.c_uint32), ("origin", C.c_float * 3), ("voxel", C.c_float), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("inflate", C.c_int32)]


def spec(origin, voxel, dims, inflate=0):
    return Spec(C.sizeof(Spec), (C.c_float * 3)(*origin), voxel, dims[0], dims[1], dims[2], inflate)


def as_spec(s):
    """any object with dsm_grid_spec's fields (api._GridSpec for one) as a Spec"""
    return s if isinstance(s, Spec) else Spec(s.struct_size, (C.c_float * 3)(*s.origin[:]), s.voxel, s.nx, s.ny, s.nz, s.inflate)


def with_inflate(s, r):
    return Spec(s.struct_size, (C.c_float * 3)(*s.origin[:]), s.voxel, s.nx, s.ny, s.nz, r)


# dyadic origin and voxel: centres, faces and corners are exact floats; an origin of ordinary magnitude far from zero; a row of
# three words with a pad; one voxel; one full word per row
GRID_37 = spec((-4.5, -2.5, -1.5), 0.25, (37, 21, 13))
GRID_33 = spec((100.3, -250.7, 3.2), 0.1, (33, 9, 5))
GRID_70 = spec((-7.1, -0.85, -0.45), 0.2, (70, 9, 5))
GRID_1 = spec((0.5, -0.25, 1.0), 0.5, (1, 1, 1))
GRID_32 = spec((-3.2, -0.8, -0.4), 0.2, (32, 8, 4))
MAIN_GRIDS = {"37x21x13": GRID_37, "33x9x5": GRID_33, "70x9x5": GRID_70}
ALL_GRIDS = dict(MAIN_GRIDS, **{"1x1x1": GRID_1, "32x8x4": GRID_32})


def dims(s):
    return s.nx, s.ny, s.nz


def words(s):
    return (s.nx + 31) // 32


def centres(s, axis):
    """grid_centre of every voxel along an axis, in float32 as the definition computes it"""
    n = dims(s)[axis]
    return (f32(s.origin[axis]) + (np.arange(n).astype(f32) + f32(0.5)) * f32(s.voxel)).astype(f32)


def _stale(out):
    return not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS)


def host_lib():
    global _lib
    if _lib is None:
        out = os.path.join(ROOT, "tests", "_build", "libgrid_host.so")
        if _stale(out):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", out + ".tmp"], check=True)
            os.replace(out + ".tmp", out)
        lib = C.CDLL(out)
        lib.grid_host.argtypes = [_vp, C.c_int64, C.POINTER(Spec), C.c_int, _vp, _vp]
        lib.grid_host.restype = None
        lib.grid_host_pairs.argtypes = [_vp, C.c_int64, C.POINTER(Spec), _vp]
        lib.grid_host_pairs.restype = None
        lib.grid_host_boxes.argtypes = [_vp, C.c_int64, C.POINTER(Spec), _vp, _vp]
        lib.grid_host_boxes.restype = None
        lib.grid_host_inflate.argtypes = [_vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int]
        lib.grid_host_inflate.restype = None
        lib.grid_host_cells.argtypes = [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int64]
        lib.grid_host_cells.restype = C.c_int64
        lib.grid_host_inflate_width.argtypes = [C.c_int, C.c_int]
        _lib = lib
    return _lib


# (the runtimes linked statically: the program then runs the same whatever else the process environment preloads)
SANITIZE = ["-fsanitize=address,undefined", "-fsanitize=float-cast-overflow", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def build_main(out, sanitize=True):
    """grid_host.cpp as a stand-alone program (its own main behind GRID_HOST_MAIN), with the sanitizers"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-DGRID_HOST_MAIN"] + (SANITIZE if sanitize else []) + [SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def write_case(path, s, surfels):
    """a case file of the stand-alone program: the dsm_grid_spec, then the records"""
    with open(path, "wb") as f:
        f.write(bytes(as_spec(s)))
        f.write(np.ascontiguousarray(surfels).tobytes())


def host_grid(surfels, s, brute=True):
    """{"index" int32 [nz, ny, nx], "occupied" uint32 [nz, ny, wx]} of the sequence `surfels` (already in order)"""
    a = np.ascontiguousarray(surfels)
    assert a.dtype.itemsize == 44
    s = as_spec(s)
    out = {"index": np.full((s.nz, s.ny, s.nx), 7, np.int32), "occupied": np.full((s.nz, s.ny, words(s)), 7, np.uint32)}
    host_lib().grid_host(a.ctypes.data, len(a), C.byref(s), int(brute), out["index"].ctypes.data, out["occupied"].ctypes.data)
    return out


def host_pairs(surfels, s):
    """bool [n, nz * ny * nx]: the checker's verdict on every (surfel, voxel) pair"""
    a = np.ascontiguousarray(surfels)
    s = as_spec(s)
    out = np.zeros((len(a), s.nx * s.ny * s.nz), np.uint8)
    if len(a):
        host_lib().grid_host_pairs(a.ctypes.data, len(a), C.byref(s), out.ctypes.data)
    return out.astype(bool)


def host_boxes(surfels, s):
    """(lo (n, 3), hi (n, 3) int32 as x y z, keep (n,) bool): grid_setup's verdict on every record"""
    a = np.ascontiguousarray(surfels)
    s = as_spec(s)
    box = np.zeros((len(a), 6), np.int32)
    keep = np.zeros(len(a), np.uint8)
    if len(a):
        host_lib().grid_host_boxes(a.ctypes.data, len(a), C.byref(s), box.ctypes.data, keep.ctypes.data)
    return box[:, :3], box[:, 3:], keep.astype(bool)


def tiers(lo, hi, keep):
    """(small, big): the list grid_emit puts every survivor on"""
    ext = (hi - lo).astype(np.int64)
    small = keep & (ext[:, 0] <= SMALL_W) & (ext[:, 1] * ext[:, 2] <= SMALL_ROWS)
    return small, keep & ~small


def host_inflate(bits, nx, r):
    b = np.ascontiguousarray(bits, np.uint32)
    nz, ny, wx = b.shape
    assert wx == (nx + 31) // 32
    out = np.full_like(b, 7)
    host_lib().grid_host_inflate(b.ctypes.data, out.ctypes.data, nx, ny, nz, r)
    return out


def host_cells(bits, nx):
    b = np.ascontiguousarray(bits, np.uint32)
    nz, ny, wx = b.shape
    out = np.zeros(max(nx * ny * nz, 1), np.int32)
    n = host_lib().grid_host_cells(b.ctypes.data, nx, ny, nz, out.ctypes.data, len(out))
    return out[:n].copy()


def host_all(surfels, s, flags=0, brute=True):
    """every output of dsm_grid_compose from the checker: index, occupied, inflated (by s.inflate), cells"""
    s = as_spec(s)
    out = host_grid(surfels, s, brute)
    out["inflated"] = host_inflate(out["occupied"], s.nx, s.inflate)
    out["cells"] = host_cells(out["inflated" if flags & CELLS_OF_INFLATED else "occupied"], s.nx)
    return out


def unpack(bits, nx):
    """a bit set [nz, ny, wx] as bools [nz, ny, nx]"""
    b = np.ascontiguousarray(bits, np.uint32)
    x = np.arange(nx)
    return ((b[..., x >> 5] >> (x & 31).astype(np.uint32)) & 1).astype(bool)


def pack(vox):
    """bools [nz, ny, nx] as a bit set [nz, ny, wx], pad bits 0"""
    nz, ny, nx = vox.shape
    wx = (nx + 31) // 32
    padded = np.zeros((nz, ny, wx * 32), np.uint64)
    padded[..., :nx] = vox
    return (padded.reshape(nz, ny, wx, 32) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)


def pad_mask(nx):
    """the pad bits of the last word of a row"""
    return np.uint32(0) if nx % 32 == 0 else np.uint32((0xffffffff << (nx % 32)) & 0xffffffff)


def same_grids(got, exp, what=""):
    """bit for bit on every output both hold"""
    for k in ("index", "occupied", "inflated", "cells"):
        if k in got and k in exp:
            a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
            assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
            bad = np.argwhere(a != b)
            assert bad.size == 0, (what, k, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])


def keep_select(m, select):
    if select == 0:
        return m[:0]
    return m[m["update_times"] >= 5] if select == 1 else m[m["update_times"] != 0]


# ------------------------------------------------------------------ records
def crafted_records(surfel_dtype, s):
    """the records the definition's exits and margins turn on, placed for the grid `s`; returns (records, names).  The three
    update_times records come first: a voxel shows the lowest number that covers it."""
    s = as_spec(s)
    rows, names = [], []
    o = np.array(s.origin[:], np.float64)
    v, h = float(s.voxel), float(s.voxel) / 2
    n = np.array(dims(s))
    ext = n * v
    mid = o + ext / 2

    def add(name, p=None, **kw):
        r = dict(px=mid[0], py=mid[1], pz=mid[2], nx=0.0, ny=0.0, nz=1.0, size=0.3 * v, color=128.0, weight=1.0, update_times=7, last_update=1)
        if p is not None:
            r.update(px=p[0], py=p[1], pz=p[2])
        r.update(kw)
        rows.append(r)
        names.append(name)

    def at(fx, fy, fz):  # the centre of the voxel at these fractions of the grid
        i = np.minimum((np.array([fx, fy, fz]) * n).astype(int), n - 1)
        return [float(centres(s, a)[i[a]]) for a in range(3)]

    def unit(x, y, z):
        q = np.array([x, y, z], np.float64)
        q /= np.linalg.norm(q)
        return dict(nx=q[0], ny=q[1], nz=q[2])

    add("update_times 0", at(0.1, 0.1, 0.1), update_times=0, size=0.0)
    add("update_times 4", at(0.3, 0.1, 0.1), update_times=4, size=0.0)
    add("update_times 5", at(0.5, 0.1, 0.1), update_times=5, size=0.0)
    add("zero normal", nz=0.0)
    add("minus-zero normal", nx=-0.0, ny=-0.0, nz=-0.0)
    for f in ("px", "py", "pz"):
        add("NaN " + f, **{f: np.nan})
        add("+inf " + f, **{f: np.inf})
        add("-inf " + f, **{f: -np.inf})
    add("NaN size", at(0.2, 0.5, 0.5), size=np.nan)
    add("negative size", at(0.2, 0.6, 0.5), size=-0.5 * v)
    add("-inf size", at(0.2, 0.7, 0.5), size=-np.inf)
    add("zero size at a voxel centre", at(0.7, 0.3, 0.3), size=0.0)
    add("inf size: the whole slab", at(0.9, 0.9, 0.9), size=np.inf, **unit(0.1, 0.2, 1.0))
    add("huge size: (size + h)^2 overflows", at(0.8, 0.2, 0.6), size=1e30, **unit(1.0, 0.1, 0.0))
    add("nn overflows", nx=3e19, ny=3e19, nz=0.0)
    add("NaN normal", ny=np.nan)
    add("inf normal", nx=np.inf)
    add("huge normal, nn finite", at(0.6, 0.6, 0.6), nx=0.0, ny=1e18, nz=1e18)
    add("tiny normal: nn a denormal", at(0.4, 0.6, 0.4), nx=1e-20, ny=0.0, nz=1e-20)
    add("tiny normal: nn underflows to 0", nx=1e-30, ny=0.0, nz=1e-30)
    add("normal of length 1e-3", at(0.4, 0.7, 0.4), nx=0.0, ny=6e-4, nz=8e-4, size=0.7 * v)
    add("normal of length 40", at(0.4, 0.8, 0.6), nx=24.0, ny=0.0, nz=32.0, size=0.7 * v)
    # the plane exactly on a cube face: normal along an axis, the centre half a voxel from a voxel centre (e2 == ta on both sides)
    for a, f in enumerate(("x", "y", "z")):
        c = at(0.5, 0.5, 0.5)
        c[a] = float(f32(c[a]) - f32(s.voxel) * f32(0.5))
        add("plane on a cube face, normal along " + f, c, nx=float(a == 0), ny=float(a == 1), nz=float(a == 2), size=0.4 * v)
    corner = at(0.3, 0.4, 0.6)
    corner = [float(f32(corner[a]) - f32(s.voxel) * f32(0.5)) for a in range(3)]
    add("centre on a voxel corner", corner, **unit(1.0, 1.0, 1.0), size=0.2 * v)
    add("centre on a voxel corner, axis normal", corner, size=0.5 * v)
    for a, f in enumerate(("x", "y", "z")):
        for side, tag in ((0, "low"), (1, "high")):
            out, on = list(mid), list(mid)
            out[a] = o[a] + (ext[a] + 2.5 * v if side else -2.5 * v)
            on[a] = o[a] + (ext[a] if side else 0.0)
            tilt = unit(*(np.where(np.arange(3) == a, 0.3, 1.0)))
            add("outside the %s %s face" % (tag, f), out, size=0.4 * v, **tilt)
            add("just outside the %s %s face, reaching in" % (tag, f), [on[k] + (0.3 * v * (1 if side else -1) if k == a else 0) for k in range(3)],
                size=1.2 * v, **tilt)
            add("straddles the %s %s face" % (tag, f), on, size=0.8 * v, **tilt)
    add("far outside, large", [mid[0] + 50 * ext[0], mid[1], mid[2]], size=3 * v)
    add("huge finite position", [3e38, -3e38, 3e38])
    add("huge finite position, huge size", [3e38, -3e38, 3e38], size=3e38)
    add("through the whole grid", mid, size=1e3 * float(ext.max()), **unit(0.3, -0.5, 1.0))
    add("wide along x", at(0.5, 0.2, 0.8), size=12 * v, **unit(0.0, 1.0, 0.2))
    add("wide along y and z", at(0.5, 0.5, 0.5), size=12 * v, **unit(1.0, 0.05, 0.0))
    add("duplicate a", at(0.8, 0.8, 0.2), size=1.1 * v, **unit(0.2, 0.1, 1.0))
    add("duplicate b", at(0.8, 0.8, 0.2), size=1.1 * v, **unit(0.2, 0.1, 1.0))
    a = np.zeros(len(rows), surfel_dtype)
    for i, r in enumerate(rows):
        for k, val in r.items():
            a[k][i] = val
    return a, names


def grid_records(rng, n, surfel_dtype, s, ut=None, spread=(-0.5, 1.5), sizes=(0.02, 0.8), scales=(1e-3, 1.0, 40.0)):
    """random surfels spread over `spread` of the grid's extent on every axis, normals of the lengths `scales`"""
    s = as_spec(s)
    a = np.zeros(n, surfel_dtype)
    o, ext = np.array(s.origin[:], np.float64), np.array(dims(s)) * float(s.voxel)
    p = o + rng.uniform(spread[0], spread[1], (n, 3)) * ext
    a["px"], a["py"], a["pz"] = p.T
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm *= rng.choice(np.array(scales), n)[:, None]
    a["nx"], a["ny"], a["nz"] = nrm.T
    a["size"] = rng.uniform(sizes[0], sizes[1], n)
    a["color"] = rng.uniform(0, 255, n)
    a["weight"] = rng.uniform(0, 50, n)
    a["update_times"] = ut if ut is not None else rng.integers(0, 12, n)
    a["last_update"] = rng.integers(0, 8, n)
    return a


# ------------------------------------------------------------------ the float64 restatement
def np_cover64(surfels, s, chunk=256):
    """The definition restated in numpy float64 from the same float32 inputs, for every (surfel, voxel) pair:
    (covered, near, inside), bool [n, voxels] each.  near: |E^2 - TA| <= 1e-4 (TA + Q NN) or |LHS - RHS| <= 1e-4 (RHS + Q NN);
    inside: |d_a| <= size + 3h + voxel on every axis."""
    s = as_spec(s)
    f64 = np.float64
    cz, cy, cx = np.meshgrid(*(f64(s.origin[a]) + (np.arange(dims(s)[a]) + 0.5) * f64(s.voxel) for a in (2, 1, 0)), indexing="ij")
    c = np.stack([cx.ravel(), cy.ravel(), cz.ravel()], 0)  # [3, voxels], x fastest
    n = len(surfels)
    covered, near, inside = (np.zeros((n, c.shape[1]), bool) for _ in range(3))
    h = f64(s.voxel) * 0.5
    for b in range(0, n, chunk):
        r = surfels[b:b + chunk]
        p = np.stack([r["px"], r["py"], r["pz"]], 1).astype(f64)
        nr = np.stack([r["nx"], r["ny"], r["nz"]], 1).astype(f64)
        size = r["size"].astype(f64)
        with np.errstate(all="ignore"):
            ok = np.isfinite(p).all(1) & (size >= 0) & np.isfinite((nr * nr).sum(1)) & ((nr * nr).sum(1) > 0)
            NN = (nr * nr).sum(1)[:, None]
            TA = ((h * np.abs(nr).sum(1)) ** 2)[:, None]
            RB = ((size + h) ** 2)[:, None] * NN
            d = c[None, :, :] - p[:, :, None]  # [m, 3, voxels]
            E2 = (nr[:, :, None] * d).sum(1) ** 2
            Q = (d * d).sum(1)
            LHS = Q * NN - E2
            covered[b:b + chunk] = ok[:, None] & (E2 <= TA) & (LHS <= RB)
            near[b:b + chunk] = (np.abs(E2 - TA) <= 1e-4 * (TA + Q * NN)) | (np.abs(LHS - RB) <= 1e-4 * (RB + Q * NN))
            inside[b:b + chunk] = (np.abs(d) <= (size + 3 * h + f64(s.voxel))[:, None, None]).all(1)
    return covered, near, inside


def np_inflate(vox, r):
    """brute-force dilation of bools [nz, ny, nx] by the voxels within radius r; outside the grid everything is free"""
    nz, ny, nx = vox.shape
    padded = np.zeros((nz + 2 * r, ny + 2 * r, nx + 2 * r), bool)
    padded[r:r + nz, r:r + ny, r:r + nx] = vox
    out = np.zeros_like(vox)
    for dz in range(-r, r + 1):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                if dx * dx + dy * dy + dz * dz <= r * r:
                    out |= padded[r + dz:r + dz + nz, r + dy:r + dy + ny, r + dx:r + dx + nx]
    return out


INFLATE_RADII = (0, 1, 2, 3, 5, 8, 16)
INFLATE_NX = (1, 31, 32, 33, 64, 70)


@functools.lru_cache(maxsize=None)
def inflate_sets():
    """[(name, bools [nz, ny, nx])]: for every nx of INFLATE_NX a sparse and a dense random set in 7 x 5 rows (11 x 6 for nx = 70:
    more than one tile of rows and of slices); single bits at every corner and at the middle of every edge; and a row of ten
    words (more than one tile of words) with bits about the word boundaries"""
    rng = np.random.default_rng(77)
    out = []
    for nx in INFLATE_NX:
        ny, nz = (11, 6) if nx == 70 else (7, 5)
        out.append(("sparse nx=%d" % nx, rng.random((nz, ny, nx)) < 0.02))
        out.append(("dense nx=%d" % nx, rng.random((nz, ny, nx)) < 0.6))
    nz, ny, nx = 5, 7, 33
    ends = lambda n: (0, n // 2, n - 1)
    for z in ends(nz):
        for y in ends(ny):
            for x in ends(nx):
                if [z in (0, nz - 1), y in (0, ny - 1), x in (0, nx - 1)].count(True) >= 2:  # the 8 corners and the 12 edge middles
                    b = np.zeros((nz, ny, nx), bool)
                    b[z, y, x] = True
                    out.append(("single bit %d %d %d" % (x, y, z), b))
    wide = np.zeros((3, 9, 300), bool)
    wide[1, 4, [0, 31, 32, 63, 64, 255, 256, 257, 299]] = True
    wide[0, 0, 150] = wide[2, 8, 287] = True
    out.append(("ten words", wide))
    for _, b in out:
        b.setflags(write=False)
    return out
