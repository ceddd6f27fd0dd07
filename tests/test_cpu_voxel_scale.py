"""The inputs of tests/test_gpu_voxel_scale.py without a GPU: tests/voxel_scale_cases.py builds them, and every condition that makes
them worth running on the device -- nearest voxels in another tile along every axis at once, the first and the last halo row met
at exactly R, every bit alignment of the x pass, freed and kept voxels behind the carve's first trip, frontier cells and all three
states behind the classification's launch caps, two depth planes whose free sets differ -- is asserted here on the host checkers
alone, so the device tests cannot pass on nothing and a builder that drifts fails on a machine without a GPU.  The checkers
themselves are pinned on the new shapes: the field's two brute-force forms against each other and against the numpy restatement,
the carve and the classification against theirs on the full grids.  Every comparison is bit for bit."""
import numpy as np

import field_cases as fc
import grid_cases as gc
import space_cases as sc
import voxel_scale_cases as vc


# ------------------------------------------------------------------ A1. more than one tile on every axis
def test_a1_conditions():
    nx, ny, nz = vc.A1_GRID
    tiles = lambda n: (n + vc.TILE - 1) // vc.TILE
    assert nx * ny * nz == 609700 and (tiles(nx), tiles(ny), nz) == (3, 2, 67) and (tiles(nx), ny, tiles(nz)) == (3, 70, 2) and nx % 32 == 2
    for name in vc.A1_SETS:
        n_set = int(vc.a1_set(name).sum())
        assert n_set <= vc.A1_MAX_SET and n_set * nx * ny * nz <= 6.1e8, (name, n_set)
        bits, dirty = vc.a1_bits(name)
        assert not (bits[..., -1] & gc.pad_mask(nx)).any() and (dirty[..., -1] & gc.pad_mask(nx)).any()
        c = vc.a1_conditions(name, 64)
        print("A1 %s: %d set voxels; at R 64 %s" % (name, n_set, c))
        for axis in "xyz":
            assert c["nearest in another %s tile" % axis] >= 1000, (name, axis, c)
        for r in (3, 16):
            c = vc.a1_conditions(name, r)
            print("A1 %s at R %d: %s" % (name, r, c))
            assert c["none in reach"] >= 1000, (name, r, c)
            # nine voxels, eight of them in one cube of two, reach no thousand voxels within 3: there the count is the cube's and the
            # corner's own (every voxel within 3 of a set voxel, counted from the set itself)
            if name == "about the seams' corner" and r == 3:
                z, y, x = np.indices(vc.A1_GRID[::-1])
                within = np.zeros(vc.A1_GRID[::-1], bool)
                for oz, oy, ox in np.argwhere(vc.a1_set(name)):
                    within |= (x - ox) ** 2 + (y - oy) ** 2 + (z - oz) ** 2 <= r * r
                assert c["one in reach"] == int(within.sum()) >= 250, (name, r, c, int(within.sum()))
            else:
                assert c["one in reach"] >= 1000, (name, r, c)


def test_a1_checker_forms_agree():
    for name in vc.A1_SETS:
        bits = vc.a1_bits(name)[0]
        a, b = fc.host_field(bits, vc.A1_GRID[0], 3, form=1), fc.host_field(bits, vc.A1_GRID[0], 3, form=2)
        fc.same_fields(a, b, (name, "list vs window"))
        fc.same_fields(vc.a1_expected(name, 3), a, (name, "the form the checker picks"))
        fc.same_fields(fc.host_field(vc.a1_bits(name)[1], vc.A1_GRID[0], 3), a, (name, "pad bits"))


# ------------------------------------------------------------------ A2. the first and the last halo row
def test_a2_conditions_and_numpy():
    cases = vc.a2_cases()
    assert len(cases) == 2 * 5 * 2 and {c[1] for c in cases} == set(fc.RADII)
    for axis, r, variant in cases:
        g = vc.a2_grid(axis)
        assert g[0] * g[1] * g[2] <= fc.NUMPY_MAX_VOXELS and g["xyz".index(axis)] == 3 * vc.TILE
        vox = vc.a2_set(axis, r, variant)
        assert int(vox.sum()) == (2 if variant == "column" else 5), (axis, r, variant, int(vox.sum()))
        exp = vc.a2_expected(axis, r, variant)
        vc.a2_conditions(axis, r, variant, exp)
        d2, near = fc.np_field(vox, r)
        assert np.array_equal(exp["dist2"], d2) and np.array_equal(exp["nearest"], near), (axis, r, variant)
    # the halo rows the two set voxels of column x0 lie in, as csrc/dsm_k_field.h numbers them: j = y - (tile * 64 - R)
    for r in vc.A2_RADII:
        rows = vc.TILE + 2 * r
        assert (vc.TILE - r) - (vc.TILE - r) == 0 and (2 * vc.TILE - 1 + r) - (vc.TILE - r) == rows - 1


# ------------------------------------------------------------------ A3. the x pass at every bit alignment
def test_a3_conditions_and_numpy():
    calls = 0
    for nx in vc.A3_NX:
        assert nx % 32 and nx <= fc.NUMPY_MAX_VOXELS
        sets = vc.a3_sets(nx)
        assert len(sets) == 66 and {xs[0] % 32 for name, xs in sets if name.startswith("a=")} == set(range(32))
        for name, xs in sets:
            vox = vc.a3_vox(nx, xs)
            assert int(vox.sum()) == len(xs)
            for r in vc.A3_RADII:
                exp = fc.host_field(gc.pack(vox), nx, r)
                d2, near = fc.np_field(vox, r)
                assert np.array_equal(exp["dist2"], d2) and np.array_equal(exp["nearest"], near), (nx, name, r)
                calls += 1
                if r == 64 and name.endswith("pair"):
                    vc.a3_conditions(xs[0], exp)
        # the row's last voxel is met from 64 below it through the last bit of the window above, and not from 65 below
        for below in (64, 65):
            lo = nx - 1 - below
            e64, e63 = (fc.host_field(gc.pack(vc.a3_vox(nx, (nx - 1, lo))), nx, r) for r in (64, 63))
            at = lambda e, x: (int(e["dist2"][0, 0, x]), int(e["nearest"][0, 0, x]))
            assert at(e64, lo - 1) == (1, lo) and at(e64, lo - 64) == (4096, lo) and at(e63, lo - 64) == (fc.FAR, -1), (nx, below)
            assert at(e64, lo + 1) == (1, lo) and at(e64, nx - 2) == (1, nx - 1), (nx, below)
            mid = lo + below // 2  # 32 from both ends, or 32 and 33: the lower voxel either way
            assert at(e64, mid) == (1024, lo), (nx, below, at(e64, mid))
    assert calls == 660


# ------------------------------------------------------------------ A4. the level sets against the inflation
def test_a4_level_sets():
    nx, ny, nz = vc.A4_GRID
    vox, bits, exp = vc.a4_case()
    assert (nx + 31) // 32 == 10 and (nx + 63) // 64 == 5 and 0.015 < vox.mean() < 0.025
    for r in vc.A4_LEVELS:
        level = exp["dist2"] <= r * r
        assert np.array_equal(gc.pack(level), vc.a4_inflated(r)), r
        assert vox.sum() < level.sum() and (level.sum() < vox.size or r == 16), (r, int(level.sum()))  # (at 16 the set reaches everything)
        if r <= 5:
            assert np.array_equal(level, gc.np_inflate(vox, r)), r
    # the set crosses every seam of the field's x tiles and of the inflation's word tiles
    x = np.argwhere(vox)[:, 2]
    assert all(((x >= s - 3) & (x < s)).any() and ((x >= s) & (x < s + 3)).any() for s in (64, 128, 192, 256))


# ------------------------------------------------------------------ B1. the carve past one trip
def test_b1_conditions_and_numpy():
    nx, ny, nz = vc.B1_GRID
    assert (nx + 63) // 64 == 1 and ny * nz == 67600 > vc.B1_TRIP and nx % 32 == 1
    second = vc.b1_second_trip()
    assert not second[:252].any() and not second[252, :16].any() and second[252, 16:].all() and second[253:].all()
    old = vc.b1_old()
    assert (old[..., -1] & gc.pad_mask(nx)).any() and 0.025 < gc.unpack(old, nx).mean() < 0.035
    counts = vc.b1_conditions()
    print("B1:", counts)
    for trip, c in counts.items():
        assert c["freed by the frames"] > 500, (trip, c)
        assert c["not freed"] > 500, (trip, c)
        assert c["free by the old set alone"] > 100, (trip, c)
    # the checker against the numpy restatement on the full grid, under every flag the device test runs
    frames = vc.b1_frames()
    for flags in vc.B1_FLAGS:
        bits, n = vc.b1_expected(flags)
        want, _ = sc.np_carve(vc.b1_grid(flags), frames, old)
        assert np.array_equal(bits, gc.pack(want)) and n == int(want.sum()), (flags, n, int(want.sum()))
    assert vc.b1_expected(sc.TRUST_INFINITE)[1] > vc.b1_expected(0)[1] > vc.b1_expected(sc.REPLACE)[1]
    # each frame frees voxels the other does not, and the second frame is the one that reaches the second trip
    a, b = (gc.unpack(sc.host_carve(vc.b1_grid(), [f])[0], nx) for f in frames)
    assert (a & ~b).sum() > 500 and (b & ~a).sum() > 500 and (b & second).sum() > 500, ((a & ~b).sum(), (b & ~a).sum(), (b & second).sum())


# ------------------------------------------------------------------ B2. the classification past every cap
def test_b2_conditions_and_numpy():
    nx, ny, nz = vc.B2_GRID
    c = vc.b2_conditions()
    print("B2:", c)
    assert c["words"] == 2250000 > vc.B2_WORD_TRIP and c["voxels"] == 4500000 > vc.B2_VOXEL_TRIP
    assert c["cell tiles"] == 8790 > 8192 and c["cell tiles"] > vc.B2_SCAN_TRIP
    assert c["cells at or behind the word trip"] > 1000 and c["cells below the word trip"] > 1000, c
    assert c["cells not ascending"] == 0, c
    assert min(c[k + " behind the voxel trip"] for k in ("unknown", "free", "occupied")) > 0, c
    occ, fre, ob, fb = vc.b2_sets()
    assert (ob[..., -1] & gc.pad_mask(nx)).any() and (fb[..., -1] & gc.pad_mask(nx)).any()
    assert 0.09 < occ.mean() < 0.11 and 0.49 < fre.mean() < 0.51
    exp = vc.b2_expected()
    state, kf, fr = sc.np_classify(occ, fre)
    assert np.array_equal(exp["state"], state)
    assert np.array_equal(exp["known_free"], gc.pack(kf)) and np.array_equal(exp["frontier"], gc.pack(fr))
    assert np.array_equal(exp["cells"], np.flatnonzero(fr.ravel())) and exp["n_frontier"] == int(fr.sum()) > 2 * vc.B2_WORD_TRIP // 4
    cut = sc.host_classify(ob, fb, nx, cap=exp["n_frontier"] // 2, planes=("cells",))
    assert cut["n_frontier"] == exp["n_frontier"] and np.array_equal(cut["cells"], exp["cells"][:exp["n_frontier"] // 2])


# ------------------------------------------------------------------ B3. two planes for the upload paths
def test_b3_conditions():
    from densesurfelmapping_amd import api
    p, q = vc.b3_planes()
    cam = sc.CAM_70
    assert p.shape == q.shape == (cam.h, cam.w) and p.dtype == np.float32 and q.dtype == np.uint16 and cam.pitch > cam.w
    assert (q == 0).any() and (q > 1000).any() and not np.isfinite(p).all()
    for g in vc.B3_GRIDS:
        differ = vc.b3_conditions(g, api.depth_from_u16)
        print("B3 %s: the free sets of P and Q differ in %s voxels" % (sc.grid_id(g), differ))
        assert all(n > 100 for n in differ.values()), (g, differ)
