"""Shared by tests/test_cpu_components.py and tests/test_gpu_components.py: the host build of the connected-component definition
(tests/components_host.cpp: a flood fill in ascending index order and, independently, a sequential union-find), the tile constants
read from the kernel header, and ONE case list -- every case with the size the GPU runs it at and, where that is large, a smaller
size of the same construction for the CPU tests -- with the checker's results computed once per (case, connectivity, min_count) and
handed out read-only."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np

import grid_cases as gc

ROOT = gc.ROOT
SRC = os.path.join(ROOT, "tests", "components_host.cpp")
CSRC = os.path.join(ROOT, "densesurfelmapping_amd", "csrc")
DEPS = [SRC, os.path.join(CSRC, "dsm_components.h"), os.path.join(ROOT, "include", "dsm.h")]
FACES, ALL = 6, 26  # DSM_CONNECT_FACES, DSM_CONNECT_ALL of include/dsm.h
COMPONENT = np.dtype([("root", np.int32), ("count", np.int32), ("sum", np.int64, (3,)), ("lo", np.int32, (3,)), ("hi", np.int32, (3,)),
                      ("tag", np.int32), ("reserved", np.int32)])
SEAM_GRID = (130, 70, 67)  # more than one tile on every axis for any tile up to 64, odd remainders

_lib = None
_vp = C.c_void_p


def kernel_constants():
    """the constexpr ints of csrc/dsm_k_components.h by name: the tiles are read from the header, never copied"""
    text = open(os.path.join(CSRC, "dsm_k_components.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (kComp\w+) = (\d+);", text)}


def host_lib():
    global _lib
    if _lib is None:
        out = os.path.join(ROOT, "tests", "_build", "libcomponents_host.so")
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in DEPS):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", SRC, "-o", out + ".tmp"], check=True)
            os.replace(out + ".tmp", out)
        lib = C.CDLL(out)
        lib.components_host.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, _vp, C.c_int32, _vp]
        lib.components_host.restype = C.c_int32
        lib.components_host_from_voxel.argtypes = [_vp, _vp, C.c_float, _vp]
        lib.components_host_from_voxel.restype = None
        lib.components_host_layout.argtypes = [_vp]
        lib.components_host_layout.restype = None
        _lib = lib
    return _lib


def build_main(out, sanitize=True):
    """components_host.cpp as a stand-alone program (its own main behind COMPONENTS_HOST_MAIN), with the sanitizers"""
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-DCOMPONENTS_HOST_MAIN"] + (gc.SANITIZE if sanitize else []) + [SRC, "-o", out]
    return subprocess.run(cmd, capture_output=True, text=True)


def write_case(path, vox, conn, min_count=1, tags=None):
    """a case file of the stand-alone program: nx ny nz connectivity min_count has_tags, the words, the tag plane"""
    nz, ny, nx = vox.shape
    with open(path, "wb") as f:
        f.write(np.array([nx, ny, nz, conn, min_count, 0 if tags is None else 1], np.int32).tobytes())
        f.write(np.ascontiguousarray(gc.pack(vox), np.uint32).tobytes())
        if tags is not None:
            f.write(np.ascontiguousarray(tags, np.int32).tobytes())


def host_components(bits, nx, conn, min_count=1, tags=None, form=0, cap=None):
    """the checker on a bit set [nz, ny, wx]: {"label" int32 [nz, ny, nx], "table" COMPONENT[min(kept, cap)], "n" kept, "n_all"}"""
    b = np.ascontiguousarray(bits, np.uint32)
    nz, ny, wx = b.shape
    assert wx == (nx + 31) // 32
    t = None if tags is None else np.ascontiguousarray(tags, np.int32)
    assert t is None or t.shape == (nz, ny, nx)
    label = np.full((nz, ny, nx), 7, np.int32)
    n_all = C.c_int32(0)
    lib = host_lib()
    kept = lib.components_host(b.ctypes.data, nx, ny, nz, conn, min_count, None if t is None else t.ctypes.data, form, label.ctypes.data, None, 0, C.byref(n_all))
    cap = kept if cap is None else min(cap, kept)
    table = np.zeros(cap, COMPONENT)
    if cap:
        lib.components_host(b.ctypes.data, nx, ny, nz, conn, min_count, None if t is None else t.ctypes.data, form, None, table.ctypes.data, cap, None)
    return {"label": label, "table": table, "n": kept, "n_all": n_all.value}


def from_voxel(point, origin, voxel):
    p, o, out = np.ascontiguousarray(point, np.float32), np.ascontiguousarray(origin, np.float32), np.zeros(3, np.int32)
    host_lib().components_host_from_voxel(p.ctypes.data, o.ctypes.data, float(voxel), out.ctypes.data)
    return tuple(int(v) for v in out)


def layout():
    out = np.zeros(8, np.int32)
    host_lib().components_host_layout(out.ctypes.data)
    return [int(v) for v in out]


def np_components(vox, conn):
    """The definition restated in plain Python and numpy: a stack flood fill over a dict of set voxels.  (label [nz, ny, nx],
    {root: (count, sums xyz, lo xyz, hi xyz)})"""
    nz, ny, nx = vox.shape
    offs = [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)
            if (dx, dy, dz) != (0, 0, 0) and (abs(dx) + abs(dy) + abs(dz) == 1 if conn == FACES else True)]
    label = np.full(vox.shape, -1, np.int32)
    stats = {}
    for z0, y0, x0 in np.argwhere(vox):  # ascending linear index
        if label[z0, y0, x0] >= 0:
            continue
        root = int((z0 * ny + y0) * nx + x0)
        label[z0, y0, x0] = root
        stack, members = [(int(x0), int(y0), int(z0))], []
        while stack:
            x, y, z = stack.pop()
            members.append((x, y, z))
            for dx, dy, dz in offs:
                a, b, c = x + dx, y + dy, z + dz
                if 0 <= a < nx and 0 <= b < ny and 0 <= c < nz and vox[c, b, a] and label[c, b, a] < 0:
                    label[c, b, a] = root
                    stack.append((a, b, c))
        m = np.array(members, np.int64)
        stats[root] = (len(m), tuple(m.sum(0)), tuple(m.min(0)), tuple(m.max(0)))
    return label, stats


# ------------------------------------------------------------------ the sets
def _empty(g):
    return np.zeros(g[::-1], bool)


def seam_boundaries():
    """{axis: the indices b at which voxel b - 1 and voxel b lie in different tiles of the kernels}, from the header's constants, on
    SEAM_GRID: the word and wave seams 32, 64, 128 along x; along y and z every multiple of the tile among 1, 8, 32, 64"""
    k = kernel_constants()
    assert k["kCompTileX"] == 32, "the x seams below are the word seams"
    out = {0: [32, 64, 128]}
    for axis, name in ((1, "kCompTileY"), (2, "kCompTileZ")):
        out[axis] = [b for b in (1, 8, 32, 64) if b % k[name] == 0 and b < SEAM_GRID[axis]]
        assert out[axis], name
    return out


def seam_pairs(kind):
    """[(p, q)] voxels (x, y, z): two-voxel pairs straddling every boundary of seam_boundaries(), as `kind` = "face" / "edge" /
    "corner" neighbours, each edge and corner pair in every diagonal sense; the pairs sit on a lattice of anchors, and the census of
    tests/test_cpu_components.py shows on the checker's counts that no two of them touch"""
    bounds = seam_boundaries()
    pairs, slot = [], 0
    for axis in range(3):
        u, v = [a for a in range(3) if a != axis]
        for b in bounds[axis]:
            steps = {"face": [(0, 0)], "edge": [(1, 0), (-1, 0), (0, 1), (0, -1)], "corner": [(1, 1), (-1, 1), (1, -1), (-1, -1)]}[kind]
            for du, dv in steps:
                # the anchor of the pair in the two other axes: a lattice of spacing 5, away from the borders
                p = [0, 0, 0]
                p[axis] = b - 1
                p[u] = 3 + 5 * (slot % 11)
                p[v] = 3 + 5 * (slot // 11)
                slot += 1
                q = list(p)
                q[axis], q[u], q[v] = b, p[u] + du, p[v] + dv
                assert all(0 <= c[a] < SEAM_GRID[a] for c in (p, q) for a in range(3)), (p, q)
                pairs.append((tuple(p), tuple(q)))
    return pairs


def seam_set(kind):
    vox = _empty(SEAM_GRID)
    for p, q in seam_pairs(kind):
        vox[p[2], p[1], p[0]] = vox[q[2], q[1], q[0]] = True
    return vox


def random_set(g, density, seed):
    return np.random.default_rng(seed).random(g[::-1]) < density


PERCOLATION = {FACES: (0.25, 0.31, 0.40), ALL: (0.06, 0.10, 0.15)}


def spans(res, g):
    """does the largest component of a checker result span more than half of every axis?"""
    t = res["table"]
    if not len(t):
        return False
    c = t[np.argmax(t["count"])]
    return all(int(c["hi"][a]) - int(c["lo"][a]) + 1 > g[a] / 2 for a in range(3))


@functools.lru_cache(maxsize=None)
def percolation_seed(conn, g=SEAM_GRID):
    """the first seed at which the largest component of the middle density spans more than half of every axis"""
    for seed in range(100, 164):
        if spans(host_components(gc.pack(random_set(g, PERCOLATION[conn][1], seed)), g[0], conn), g):
            return seed
    raise AssertionError("no spanning seed")


def serpentine(mirrored=False):
    """66 x 9 x 3, one 6-connected chain: full rows at (y even, z in {0, 2}), joined in turn at x = 65 through z = 1 and at x = 0
    through the odd rows; the last join is at x = 0, so that the chain runs from voxel 0 to the highest index.  mirrored: the point
    reflection, whose root is the far end of the original."""
    g = (66, 9, 3)
    vox = _empty(g)
    for y in range(0, 9, 2):
        vox[0, y, :] = vox[2, y, :] = True
        vox[1, y, 0 if y == 8 else 65] = True
    for y in range(1, 9, 2):
        vox[2 if y % 4 == 1 else 0, y, 0] = True
    return vox[::-1, ::-1, ::-1].copy() if mirrored else vox


def u_shape():
    """70 x 12 x 2: two arms along y at x = 1 and x = 68 that join only through the row y = 11"""
    vox = _empty((70, 12, 2))
    vox[0, :, 1] = vox[0, :, 68] = True
    vox[0, 11, 1:69] = True
    return vox


def checkerboard(g):
    z, y, x = np.indices(g[::-1])
    return (x + y + z) % 2 == 0


def sized_components():
    """40 x 13 x 2: six straight components of 1 .. 6 voxels along x, two rows apart"""
    vox = _empty((40, 13, 2))
    for k in range(1, 7):
        vox[0, 2 * k - 1, 30:30 + k] = True  # across the word seam at 32 from k = 3 on
    return vox


class Case:
    def __init__(self, name, gpu, cpu=None, conns=(FACES, ALL), min_counts=(1,), table=True):
        self.name, self._gpu, self._cpu, self.conns, self.min_counts, self.table = name, gpu, cpu, conns, min_counts, table

    @functools.lru_cache(maxsize=None)
    def vox(self, cpu=False):
        v = (self._cpu if cpu and self._cpu else self._gpu)()
        v.setflags(write=False)
        return v


@functools.lru_cache(maxsize=None)
def cases():
    out = [Case("seam %s pairs" % k, functools.partial(seam_set, k)) for k in ("face", "edge", "corner")]
    for conn in (FACES, ALL):
        for k, d in enumerate(PERCOLATION[conn]):
            out.append(Case("percolation %d at %g" % (conn, d), functools.partial(lambda c, dd: random_set(SEAM_GRID, dd, percolation_seed(c)), conn, d),
                            conns=(conn,)))
    out += [
        Case("serpentine", serpentine),
        Case("serpentine mirrored", functools.partial(serpentine, True)),
        Case("u shape", u_shape),
        Case("empty", lambda: _empty((37, 5, 3))),
        Case("all set 33x5x3", lambda: np.ones((3, 5, 33), bool)),
        Case("one voxel", lambda: np.ones((1, 1, 1), bool)),
        Case("nx 1", lambda: random_set((1, 40, 9), 0.5, 5)),
        Case("checkerboard 34x6x4", lambda: checkerboard((34, 6, 4))),
        Case("all set 2x2000x2000", lambda: np.ones((2000, 2000, 2), bool), cpu=lambda: np.ones((40, 40, 2), bool), conns=(FACES,)),
        Case("checkerboard 2x1500x1500", lambda: checkerboard((2, 1500, 1500)), cpu=lambda: checkerboard((2, 30, 30)), conns=(FACES,), min_counts=(2,),
             table=False),
        Case("sizes 1 to 6", sized_components, min_counts=(1, 3, 6, 7)),
    ]
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def expected(name, conn, min_count=1, cpu=False):
    """the checker's result of a case, computed once; read-only"""
    v = case(name).vox(cpu)
    res = host_components(gc.pack(v), v.shape[2], conn, min_count)
    for a in (res["label"], res["table"]):
        a.setflags(write=False)
    return res
