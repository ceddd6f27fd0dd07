"""Shared by tests/test_cpu_field.py and tests/test_gpu_field.py: the host build of the distance field's definition
(tests/field_host.cpp: the minimum of csrc/dsm_math.h's field_key over the set voxels within R, by brute force), the grids, the
radii, the bit sets and ONE case list, with the checker's planes computed once per case and handed out read-only."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np

import grid_cases as gc

ROOT = gc.ROOT
SRC = os.path.join(ROOT, "tests", "field_host.cpp")
DEPS = [SRC, os.path.join(ROOT, "densesurfelmapping_amd", "csrc", "dsm_math.h"), os.path.join(ROOT, "densesurfelmapping_amd", "csrc", "dsm_align.h"),
        os.path.join(ROOT, "include", "dsm.h")]
FAR, MAX_DIST = 65535, 64   # DSM_FIELD_FAR, DSM_FIELD_MAX_DIST of include/dsm.h
PLANES = ("dist2", "nearest", "distance")
TYPES = {"dist2": np.uint16, "nearest": np.int32, "distance": np.float32}
VOXEL = 0.25

# (nx, ny, nz): one voxel; smaller than any radius; 31 / 32 / 33 / 65 about the word boundaries; odd sizes in several tiles of rows
# and slices; a full tile; lines longer than any tile along x, y and z
GRIDS = ((1, 1, 1), (2, 3, 4), (31, 3, 2), (32, 3, 2), (33, 3, 2), (65, 4, 3), (37, 21, 13), (64, 64, 8), (300, 5, 3), (5, 300, 3), (3, 5, 300))
RADII = (1, 3, 16, 63, 64)
NUMPY_MAX_VOXELS = 37 * 21 * 13  # the grids the numpy restatement is run on

_lib = None
_vp = C.c_void_p


def grid_id(g):
    return "%dx%dx%d" % g


def host_lib():
    global _lib
    if _lib is None:
        out = os.path.join(ROOT, "tests", "_build", "libfield_host.so")
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-std=c++17", "-O2", "-fopenmp", "-shared", "-fPIC", SRC, "-o", out + ".tmp"], check=True)
            os.replace(out + ".tmp", out)
        lib = C.CDLL(out)
        lib.field_host.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_int, _vp, _vp, _vp]
        lib.field_host.restype = None
        lib.field_host_table.argtypes = [C.c_float, C.c_int, _vp]
        lib.field_host_table.restype = None
        _lib = lib
    return _lib


def build_main(out, sanitize=True):
    """field_host.cpp as a stand-alone program (its own main behind FIELD_HOST_MAIN), with the sanitizers"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-DFIELD_HOST_MAIN"] + (gc.SANITIZE if sanitize else []) + [SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def write_case(path, bits, nx, r, voxel=VOXEL):
    """a case file of the stand-alone program: nx ny nz R, the voxel edge, the words"""
    b = np.ascontiguousarray(bits, np.uint32)
    nz, ny, _ = b.shape
    with open(path, "wb") as f:
        f.write(np.array([nx, ny, nz, r], np.int32).tobytes())
        f.write(np.float32(voxel).tobytes())
        f.write(b.tobytes())


def host_field(bits, nx, r, voxel=VOXEL, form=0):
    """the checker's planes {"dist2", "nearest", "distance"} [nz, ny, nx] of a bit set [nz, ny, wx]"""
    b = np.ascontiguousarray(bits, np.uint32)
    nz, ny, wx = b.shape
    assert wx == (nx + 31) // 32
    out = {k: np.full((nz, ny, nx), 7, TYPES[k]) for k in PLANES}
    host_lib().field_host(b.ctypes.data, nx, ny, nz, r, voxel, form, *(out[k].ctypes.data for k in PLANES))
    return out


def host_table(voxel, r):
    t = np.zeros(r * r + 1, np.float32)
    host_lib().field_host_table(voxel, r, t.ctypes.data)
    return t


def np_field(vox, r):
    """The definition restated in numpy: every voxel against every set voxel (in chunks of about a million pairs), argmin of the
    packed key.  (dist2, nearest) [nz, ny, nx]"""
    nz, ny, nx = vox.shape
    o = np.argwhere(vox).astype(np.int64)                     # (m, 3) as z y x, ascending linear index
    v = np.argwhere(np.ones_like(vox)).astype(np.int64)
    dist2, nearest = np.full(len(v), FAR, np.uint16), np.full(len(v), -1, np.int32)
    if len(o):
        chunk = max(16, (1 << 20) // len(o))
        lin = ((o[:, 0] * ny + o[:, 1]) * nx + o[:, 2]).astype(np.uint64)
        for b in range(0, len(v), chunk):
            d2 = ((v[b:b + chunk, None, :] - o[None, :, :]) ** 2).sum(-1).astype(np.uint64)
            key = np.where(d2 <= r * r, (d2 << np.uint64(32)) | lin[None, :], np.uint64(0xffffffffffffffff))
            k = key[np.arange(len(key)), key.argmin(1)]
            have = k != np.uint64(0xffffffffffffffff)
            dist2[b:b + chunk][have] = (k[have] >> np.uint64(32)).astype(np.uint16)
            nearest[b:b + chunk][have] = (k[have] & np.uint64(0xffffffff)).astype(np.int32)
    return dist2.reshape(vox.shape), nearest.reshape(vox.shape)


def dirty_pads(bits, nx, rng):
    """the bit set with random garbage in the pad bits of every row's last word"""
    d = np.array(bits, np.uint32)
    d[..., -1] |= gc.pad_mask(nx) & rng.integers(0, 1 << 32, d[..., -1].shape, dtype=np.uint64).astype(np.uint32)
    return d


# ------------------------------------------------------------------ the sets
@functools.lru_cache(maxsize=None)
def sets(g):
    """{name: bools [nz, ny, nx]} for the grid g = (nx, ny, nz); a set that does not fit the grid is left out"""
    nx, ny, nz = g
    n = (nz, ny, nx)
    rng = np.random.default_rng(1000 * nx + 10 * ny + nz)
    out = {}

    def put(name, *voxels):  # voxels as (x, y, z)
        if all(0 <= p[a] < g[a] for p in voxels for a in range(3)):
            b = np.zeros(n, bool)
            for x, y, z in voxels:
                b[z, y, x] = True
            out[name] = b

    out["empty"] = np.zeros(n, bool)
    out["full"] = np.ones(n, bool)
    for c in range(8):
        put("corner %d" % c, tuple((g[a] - 1) * ((c >> a) & 1) for a in range(3)))
    mid = (nx // 2, ny // 2, nz // 2)
    put("centre", mid)
    # two voxels with a third exactly between them: the tie goes to the lower linear index
    for a, name in enumerate("xyz"):
        lo, hi = list(mid), list(mid)
        lo[a], hi[a] = mid[a] - 1, mid[a] + 1
        put("tie along " + name, tuple(lo), tuple(hi))
    put("tie diagonal", tuple(m - 1 for m in mid), tuple(m + 1 for m in mid))
    put("tie across y and x", (mid[0] + 1, mid[1] - 1, mid[2]), (mid[0] - 1, mid[1] + 1, mid[2]))
    # both sides of the truncation at R = 64: the voxel at 69 is 64 from the one at 5 and 65 from the one at 134, the voxel at 70
    # the other way round, 198 is the last in reach of 134; and set voxels 64 and 65 apart (20, 84, 149)
    for a, name in enumerate("xyz"):
        for tag, at in (("129 apart along ", (5, 134)), ("64 and 65 apart along ", (20, 84, 149))):
            ps = []
            for p in at:
                q = list(mid)
                q[a] = p
                ps.append(tuple(q))
            put(tag + name, *ps)
    plane = np.zeros(n, bool)
    plane[nz // 2] = True
    out["plane"] = plane
    for density in (0.001, 0.05, 0.5):
        out["random %g" % density] = rng.random(n) < density
    for b in out.values():
        b.setflags(write=False)
    return out


def radii_of(g, k, name):
    """the radii the k-th set of grid g is run at: all of them on the small grids and for the sets about the truncation (they are
    sparse: cheap for the checker), two in rotation on the larger grids (every radius is met by every fifth set, and the sets
    number more than twenty)"""
    if g[0] * g[1] * g[2] <= 2048 or "apart" in name:
        return RADII
    return (RADII[k % 5], RADII[(k + 2) % 5])


@functools.lru_cache(maxsize=None)
def case_list():
    """[(grid, set name, R)]: the one list both test files run"""
    return tuple((g, name, r) for g in GRIDS for k, name in enumerate(sets(g)) for r in radii_of(g, k, name))


@functools.lru_cache(maxsize=None)
def expected(g, name, r):
    """the checker's planes of a case, computed once; read-only"""
    out = host_field(gc.pack(sets(g)[name]), g[0], r)
    for a in out.values():
        a.setflags(write=False)
    return out


def same_fields(got, exp, what=""):
    """bit for bit on every plane both hold"""
    for k in PLANES:
        if k in got and k in exp:
            a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(exp[k])
            assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
            bad = np.argwhere(a.view(np.uint32 if k == "distance" else a.dtype) != b.view(np.uint32 if k == "distance" else b.dtype))
            assert bad.size == 0, (what, k, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])
