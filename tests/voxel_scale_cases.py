"""Shared by tests/test_cpu_voxel_scale.py and tests/test_gpu_voxel_scale.py: the voxel kernels' cases at their tile seams and past
their launch caps, as pure-numpy builders over the checkers of field_cases, space_cases and grid_cases.  Every case carries its
CONDITIONS: facts about the checker's output that show the case reaches what it is built for (a nearest voxel in another tile on
every axis, the first and the last halo row, every bit alignment of the x pass, the second trip of a grid-stride loop, frontier
cells behind a launch cap).  The CPU file asserts them; the GPU file runs the cases.
  A1  the distance field with more than one tile on every axis at once
  A2  the first and the last halo row of the y and the z pass
  A3  the x pass at every bit alignment
  A4  the field's level sets against the inflation across its own tile seams
  B1  the carve past one trip of its loop
  B2  the classification past every launch cap
  B3  two depth planes for the public upload paths"""
import functools

import numpy as np

import field_cases as fc
import grid_cases as gc
import space_cases as sc

TILE = 64  # kFieldTile of csrc/dsm_k_field.h, and the 64 voxels of x a workgroup of the y and z passes takes


def _frozen(a):
    a.setflags(write=False)
    return a


def _lin(g, x, y, z):
    return (z * g[1] + y) * g[0] + x


# ------------------------------------------------------------------ A1. more than one tile on every axis
A1_GRID = (130, 70, 67)  # the y pass splits its blocks over (3, 2, 67), the z pass over (3, 70, 2): all factors distinct
A1_RADII = (3, 16, 63, 64)
A1_MAX_SET = 1000        # the checker's list form then visits at most 6.1e8 pairs a case
A1_SETS = ("random and corners", "about the seams' corner", "slabs about the seams")


@functools.lru_cache(maxsize=None)
def a1_set(name):
    """bools [nz, ny, nx]"""
    nx, ny, nz = A1_GRID
    rng = np.random.default_rng(130 + A1_SETS.index(name))
    b = np.zeros((nz, ny, nx), bool)
    if name == "random and corners":
        b.ravel()[rng.choice(b.size, 200, replace=False)] = True
        for c in range(8):
            b[(nz - 1) * ((c >> 2) & 1), (ny - 1) * ((c >> 1) & 1), (nx - 1) * (c & 1)] = True
    elif name == "about the seams' corner":
        b[63:65, 63:65, 63:65] = True
        b[66, 69, 129] = True
    else:  # three voxels either side of the seams x = 64, x = 128, y = 64 and z = 64
        slab = np.zeros_like(b)
        slab[:, :, 61:67] = slab[:, :, 125:131] = slab[:, 61:67, :] = slab[61:67, :, :] = True
        b = slab & (rng.random(b.shape) < 0.005)
    assert 0 < b.sum() <= A1_MAX_SET, (name, int(b.sum()))
    return _frozen(b)


@functools.lru_cache(maxsize=None)
def a1_bits(name):
    """(the packed set, the same with garbage in the pad bits: nx mod 32 = 2)"""
    bits = gc.pack(a1_set(name))
    dirty = fc.dirty_pads(bits, A1_GRID[0], np.random.default_rng(7 + A1_SETS.index(name)))
    assert (dirty != bits).any()
    return _frozen(bits), _frozen(dirty)


@functools.lru_cache(maxsize=None)
def a1_expected(name, r):
    out = fc.host_field(a1_bits(name)[0], A1_GRID[0], r)
    for a in out.values():
        a.setflags(write=False)
    return out


def a1_conditions(name, r):
    """{condition: count} of the checker's planes: at R = 64 the voxels whose nearest set voxel lies in another tile along x, y and
    z; at the small radii the voxels with and without a set voxel in reach"""
    nx, ny, nz = A1_GRID
    near = a1_expected(name, r)["nearest"].astype(np.int64)
    have = near >= 0
    z, y, x = np.indices(near.shape)
    tiles = {"x": (x // TILE, near % nx // TILE), "y": (y // TILE, near // nx % ny // TILE), "z": (z // TILE, near // (nx * ny) // TILE)}
    out = {"nearest in another %s tile" % a: int((have & (own != other)).sum()) for a, (own, other) in tiles.items()}
    out["none in reach"], out["one in reach"] = int((~have).sum()), int(have.sum())
    return out


# ------------------------------------------------------------------ A2. the first and the last halo row
A2_AXES = ("y", "z")
A2_RADII = (1, 3, 16, 63, 64)
A2_X0 = 2
A2_VARIANTS = ("column", "row")  # "row": three further set voxels in the row of the voxel at 64 - R


def a2_grid(axis):
    return (5, 3 * TILE, 3) if axis == "y" else (5, 3, 3 * TILE)


def a2_at(axis, x, p):
    """(x, y, z) of position p along the axis, in the middle of the third axis"""
    return (x, p, 1) if axis == "y" else (x, 1, p)


@functools.lru_cache(maxsize=None)
def a2_set(axis, r, variant):
    """bools [nz, ny, nx]: set voxels at 64 - R and 127 + R along the axis in column x0 -- exactly R from the first and the last row
    of tile 1, across its seams, at halo rows 0 and 63 + 2R of that tile's workgroup.  "row": the x pass hands the later pass a
    non-zero offset at the halo row in the columns beside"""
    g = a2_grid(axis)
    voxels = [a2_at(axis, A2_X0, TILE - r), a2_at(axis, A2_X0, 2 * TILE - 1 + r)]
    if variant == "row":
        voxels += [a2_at(axis, x, TILE - r) for x in (A2_X0 - 1, A2_X0 + 1, g[0] - 1)]
    return _frozen(sc.voxels(g, voxels))


def a2_cases():
    return [(axis, r, v) for axis in A2_AXES for r in A2_RADII for v in A2_VARIANTS]


def a2_expected(axis, r, variant):
    return fc.host_field(gc.pack(a2_set(axis, r, variant)), 5, r)


def a2_conditions(axis, r, variant, exp):
    """what the checker's planes `exp` must show for the case to reach the halo's extremes; raises AssertionError with the figures"""
    g = a2_grid(axis)
    first, last = TILE, 2 * TILE - 1  # the first and the last row of tile 1
    at = lambda x, p: (int(exp["dist2"][a2_at(axis, x, p)[::-1]]), int(exp["nearest"][a2_at(axis, x, p)[::-1]]))
    lin = lambda x, p: _lin(g, *a2_at(axis, x, p))
    what = (axis, r, variant)
    far = (fc.FAR, -1)
    # column x0: the first and the last row of tile 1 reach the voxel across the seam at exactly R; the rows between reach nothing
    assert at(A2_X0, first) == (r * r, lin(A2_X0, TILE - r)), (what, at(A2_X0, first))
    assert at(A2_X0, last) == (r * r, lin(A2_X0, last + r)), (what, at(A2_X0, last))
    between = [at(A2_X0, p) for p in range(first + 1, last)]
    assert all(v == far for v in between), (what, sum(v != far for v in between))
    # a column beside: its entries lie at R^2 + 1 from those rows, so it is not empty, the walk runs, and every entry is rejected ...
    assert at(A2_X0 + 1, last) == far, (what, at(A2_X0 + 1, last))
    assert at(A2_X0 + 1, last + 1) == ((r - 1) ** 2 + 1, lin(A2_X0, last + r)), (what, at(A2_X0 + 1, last + 1))  # ... one row on they are in reach
    if variant == "column":
        assert at(A2_X0 + 1, first) == far, (what, at(A2_X0 + 1, first))
        assert at(A2_X0 + 1, first - 1) == ((r - 1) ** 2 + 1, lin(A2_X0, TILE - r)), (what, at(A2_X0 + 1, first - 1))
    else:  # column 0 takes the offset + 1 from the x pass at the halo row; the further voxels' own columns reach them at offset 0
        assert at(0, first) == far, (what, at(0, first))
        assert at(0, first - 1) == ((r - 1) ** 2 + 1, lin(1, TILE - r)), (what, at(0, first - 1))
        for x in (A2_X0 - 1, A2_X0 + 1, g[0] - 1):
            assert at(x, first) == (r * r, lin(x, TILE - r)), (what, x, at(x, first))


# ------------------------------------------------------------------ A3. the x pass at every bit alignment
A3_NX = (193, 200)
A3_RADII = fc.RADII


@functools.lru_cache(maxsize=None)
def a3_sets(nx):
    """[(name, set x positions)] of the one-row grid (nx, 1, 1): for every alignment a = 0 .. 31 a pair 129 apart (64 from the voxel
    at a + 64, 65 from the one at a + 65) and the same with a third voxel between; the last voxel with one 64 and one 65 below it"""
    out = []
    for a in range(32):
        out.append(("a=%d pair" % a, (a, a + 129)))
        out.append(("a=%d triple" % a, (a, a + 64, a + 129)))
    out.append(("last and 64 below", (nx - 1, nx - 65)))
    out.append(("last and 65 below", (nx - 1, nx - 66)))
    assert all(0 <= x < nx for _, xs in out for x in xs)
    return out


def a3_vox(nx, xs):
    b = np.zeros((1, 1, nx), bool)
    b[0, 0, list(xs)] = True
    return b


def a3_conditions(a, exp):
    """the pair of alignment a at R = 64: the voxel at a + 64 reaches a, the one at a + 65 reaches a + 129 and not a, both at 64"""
    d2, near = exp["dist2"][0, 0], exp["nearest"][0, 0]
    assert (int(d2[a + 64]), int(near[a + 64])) == (4096, a), (a, int(d2[a + 64]), int(near[a + 64]))
    assert (int(d2[a + 65]), int(near[a + 65])) == (4096, a + 129), (a, int(d2[a + 65]), int(near[a + 65]))


# ------------------------------------------------------------------ A4. the level sets against the inflation
A4_GRID = (300, 20, 10)  # ten words a row: two inflate tiles of words, three of rows, three of slices; five field tiles along x
A4_R = 16
A4_LEVELS = (1, 5, 16)


@functools.lru_cache(maxsize=None)
def a4_case():
    """(bools [nz, ny, nx], the packed set, the checker's field at R = 16)"""
    vox = np.random.default_rng(300).random(A4_GRID[::-1]) < 0.02
    bits = gc.pack(vox)
    exp = fc.host_field(bits, A4_GRID[0], A4_R)
    for a in exp.values():
        a.setflags(write=False)
    return _frozen(vox), _frozen(bits), exp


@functools.lru_cache(maxsize=None)
def a4_inflated(r):
    return _frozen(gc.host_inflate(a4_case()[1], A4_GRID[0], r))


# ------------------------------------------------------------------ B1. the carve past one trip
B1_GRID = (33, 260, 260)   # one wave unit a row: 67 600 units against the 65 536 of one trip
B1_TRIP = 16384 * 4        # k_carve's blocks times the waves of a block
B1_VOXEL = 0.02            # 0.66 x 5.2 x 5.2 m about (0, 0, 1.6): z from -1.0 to 4.2
B1_FLAGS = (0, sc.REPLACE, sc.TRUST_INFINITE)


def b1_grid(flags=0):
    origin = tuple(np.float32(c - n * B1_VOXEL / 2) for c, n in zip((0.0, 0.0, 1.6), B1_GRID))
    return sc.make(B1_GRID, sc.CAM_70, origin=origin, flags=flags, voxel=B1_VOXEL)


@functools.lru_cache(maxsize=None)
def b1_frames():
    """two frames: a camera at the origin that sees the low slices, and one at z = 2.6 m whose wall lies behind the grid's far face, so
    that it sees through the last slices -- the rows of the second trip"""
    cam = sc.CAM_70
    return [(sc.pose_at((0.0, 0.0, 0.0)), None, _frozen(sc.depth_plane(cam, 260))),
            (sc.pose_at((0.05, -0.1, 2.6), yaw=0.05, pitch=-0.03), None, _frozen(sc.depth_plane(cam, 261)))]


@functools.lru_cache(maxsize=None)
def b1_old():
    rng = np.random.default_rng(33)
    old = sc.dirty_pads(gc.pack(rng.random(B1_GRID[::-1]) < 0.03), B1_GRID[0], rng)
    return _frozen(old)


@functools.lru_cache(maxsize=None)
def b1_expected(flags):
    """the checker's (bits, count) of the frames carved into the old set under `flags`"""
    bits, n = sc.host_carve(b1_grid(flags), b1_frames(), b1_old())
    return _frozen(bits), n


def b1_second_trip():
    """bools [nz, ny, nx]: the voxels whose row (one wave unit) has z * ny + y >= 65 536"""
    nx, ny, nz = B1_GRID
    rows = np.arange(ny * nz).reshape(nz, ny) >= B1_TRIP
    return np.broadcast_to(rows[:, :, None], (nz, ny, nx))


def b1_conditions():
    """{trip: {condition: count}}: voxels freed by the frames, not freed, and free only because the old set held them"""
    nx = B1_GRID[0]
    by_frames = gc.unpack(sc.host_carve(b1_grid(), b1_frames())[0], nx)
    after = gc.unpack(b1_expected(0)[0], nx)
    second = b1_second_trip()
    out = {}
    for name, trip in (("first trip", ~second), ("second trip", second)):
        out[name] = {"freed by the frames": int((by_frames & trip).sum()), "not freed": int((~after & trip).sum()),
                     "free by the old set alone": int((after & ~by_frames & trip).sum())}
    return out


# ------------------------------------------------------------------ B2. the classification past every cap
B2_GRID = (2, 1500, 1500)       # one word a row: 2 250 000 words, 4 500 000 voxels, 8790 tiles of the cell list
B2_WORD_TRIP = 8192 * 256       # k_space_words, k_grid_cell_count and k_grid_cell_scatter
B2_VOXEL_TRIP = 16384 * 256     # k_space_state
B2_SCAN_TRIP = 1024             # tiles per trip of k_cloud_scan


@functools.lru_cache(maxsize=None)
def b2_sets():
    """(occupied, free) bools [nz, ny, nx], and the same packed with garbage in the 30 pad bits of every word"""
    rng = np.random.default_rng(1500)
    n = B2_GRID[::-1]
    occ, fre = rng.random(n) < 0.1, rng.random(n) < 0.5
    ob, fb = sc.dirty_pads(gc.pack(occ), B2_GRID[0], rng), sc.dirty_pads(gc.pack(fre), B2_GRID[0], rng)
    return _frozen(occ), _frozen(fre), _frozen(ob), _frozen(fb)


@functools.lru_cache(maxsize=None)
def b2_expected():
    _, _, ob, fb = b2_sets()
    out = sc.host_classify(ob, fb, B2_GRID[0])
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def b2_conditions():
    """{condition: count} of the checker's planes"""
    nx, ny, nz = B2_GRID
    exp = b2_expected()
    cells = exp["cells"].astype(np.int64)
    word = cells // nx  # (one word a row)
    tail = exp["state"].ravel()[B2_VOXEL_TRIP:]
    out = {"words": ny * nz, "voxels": nx * ny * nz, "cell tiles": (ny * nz + 255) // 256,
           "cells at or behind the word trip": int((word >= B2_WORD_TRIP).sum()), "cells below the word trip": int((word < B2_WORD_TRIP).sum()),
           "cells not ascending": int((np.diff(cells) <= 0).sum())}
    for name, v in (("unknown", sc.UNKNOWN), ("free", sc.FREE), ("occupied", sc.OCCUPIED)):
        out[name + " behind the voxel trip"] = int((tail == v).sum())
    return out


# ------------------------------------------------------------------ B3. two planes for the public upload paths
B3_GRIDS = ((37, 21, 13), (65, 4, 3))
B3_U16 = ((1000.0, "divide"), (0.001, "multiply"))  # integer millimetres, as the sensor-native suite converts them
B3_POSE = sc.pose_at((0.1, 0.05, 0.0), yaw=-0.15, pitch=0.1)


@functools.lru_cache(maxsize=None)
def b3_planes():
    """(P float32 [h, w], Q uint16 [h, w] in millimetres): a wall about 2.7 m away with holes, behind both grids, and one about 1.4 m
    away, in front of the smaller grid, with the pixels that hold no finite positive depth at 0"""
    cam = sc.CAM_70
    p = sc.depth_plane(cam, 370)[:, :cam.w] * np.float32(1.4)
    q = sc.depth_plane(cam, 371)[:, :cam.w].astype(np.float64) * 750.0
    q = np.where(np.isfinite(q) & (q > 0), np.round(q), 0.0).astype(np.uint16)
    return _frozen(p), _frozen(q)


def b3_pitched(tight, pad=0.0):
    cam = sc.CAM_70
    plane = np.full((cam.h, cam.pitch), pad, np.float32)
    plane[:, :cam.w] = tight
    return plane


def b3_conditions(g, depth_from_u16):
    """the voxels in which the checker's free sets of P and of Q (under either conversion) differ"""
    p, q = b3_planes()
    s = sc.make(g, sc.CAM_70)
    free_p = sc.host_carve(s, [(B3_POSE, None, b3_pitched(p))])[0]
    out = {}
    for scale, op in B3_U16:
        free_q = sc.host_carve(s, [(B3_POSE, None, b3_pitched(depth_from_u16(q, scale, op)))])[0]
        out[op] = int(gc.unpack(free_p ^ free_q, g[0]).sum())
    return out


# ------------------------------------------------------------------ C. one handle, everything interleaved
C_SMALL = (33, 9, 5)


@functools.lru_cache(maxsize=None)
def c_small_sets():
    """(occupied, free) packed, with garbage in the pad bits"""
    rng = np.random.default_rng(3395)
    occ, fre = rng.random(C_SMALL[::-1]) < 0.3, rng.random(C_SMALL[::-1]) < 0.9
    return _frozen(sc.dirty_pads(gc.pack(occ), C_SMALL[0], rng)), _frozen(sc.dirty_pads(gc.pack(fre), C_SMALL[0], rng))
