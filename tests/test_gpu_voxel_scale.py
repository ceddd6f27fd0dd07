"""The voxel kernels on the GPU at their tile seams and past their launch caps (dsm_grid_distance, dsm_grid_inflate, dsm_grid_carve,
dsm_grid_classify, dsm_grid_compose, dsm_field_compose): the cases of tests/voxel_scale_cases.py, whose conditions
tests/test_cpu_voxel_scale.py asserts without a GPU, every result bit for bit against the host checkers of field_cases,
space_cases and grid_cases.
  A1  the field with more than one tile on every axis at once      A2  its first and last halo row
  A3  its x pass at every bit alignment                            A4  its level sets against the inflation
  B1  the carve past one trip                                      B2  the classification past every cap
  B3  the carve right behind the asynchronous upload paths         C   one handle, everything interleaved"""
import numpy as np
import pytest

import field_cases as fc
import grid_cases as gc
import space_cases as sc
import voxel_scale_cases as vc
import test_gpu_field as tf
import test_gpu_space as ts

pytestmark = pytest.mark.gpu

GUARD, N_GUARD = ts.GUARD, ts.N_GUARD


@pytest.fixture(scope="module")
def api():
    import torch
    torch.cuda.init()  # (before the library's first HIP call, as in the other GPU suites)
    from densesurfelmapping_amd import api as api_mod
    return api_mod


def _upload(bits):
    return tf._upload(np.array(bits, np.uint32))  # (a copy: the cases' arrays are read-only, which torch does not take)


def _two_plane_subset(k):
    return tf.SUBSETS[3 + k % 3]  # the three pairs of planes, in rotation


# ------------------------------------------------------------------ A1. more than one tile on every axis
@pytest.mark.parametrize("name", vc.A1_SETS)
def test_a1_every_axis_tiled(api, name):
    g = vc.A1_GRID
    ff = tf._engine(api)
    bits, dirty = vc.a1_bits(name)
    src = _upload(dirty)
    for k, r in enumerate(vc.A1_RADII):
        exp = vc.a1_expected(name, r)
        fc.same_fields(tf._distance(ff, g, r, src, what=(name, r)), exp, (name, r, "garbage in the pad bits"))
        sub = _two_plane_subset(k + vc.A1_SETS.index(name))
        assert len(sub) == 2
        fc.same_fields(tf._distance(ff, g, r, src, sub, what=(name, r, sub)), {p: exp[p] for p in sub}, (name, r, sub))
    assert np.array_equal(src.cpu().numpy().view(np.uint32), dirty), "the source is read only"
    ff.close()


# ------------------------------------------------------------------ A2. the first and the last halo row
@pytest.mark.parametrize("axis", vc.A2_AXES)
def test_a2_halo_extremes(api, axis):
    g = vc.a2_grid(axis)
    ff = tf._engine(api)
    for _, r, variant in (c for c in vc.a2_cases() if c[0] == axis):
        exp = vc.a2_expected(axis, r, variant)
        vc.a2_conditions(axis, r, variant, exp)
        got = tf._distance(ff, g, r, _upload(gc.pack(vc.a2_set(axis, r, variant))), what=(axis, r, variant))
        fc.same_fields(got, exp, (axis, r, variant))
    ff.close()


# ------------------------------------------------------------------ A3. the x pass at every bit alignment
@pytest.mark.parametrize("nx", vc.A3_NX)
def test_a3_every_bit_alignment(api, nx):
    rng = np.random.default_rng(nx)
    g = (nx, 1, 1)
    ff = tf._engine(api)
    calls = 0
    for name, xs in vc.a3_sets(nx):
        bits = gc.pack(vc.a3_vox(nx, xs))
        dirty = fc.dirty_pads(bits, nx, rng)
        src = _upload(dirty)
        for r in vc.A3_RADII:
            fc.same_fields(tf._distance(ff, g, r, src, what=(nx, name, r)), fc.host_field(bits, nx, r), (nx, name, r))
            calls += 1
    assert calls == 330
    ff.close()


# ------------------------------------------------------------------ A4. the level sets against the inflation
def test_a4_level_sets_against_inflation(api):
    g = vc.A4_GRID
    vox, bits, exp = vc.a4_case()
    ff = tf._engine(api)
    src = _upload(bits)
    got = tf._distance(ff, g, vc.A4_R, src, what="A4")
    fc.same_fields(got, exp, "A4 field")
    for r in vc.A4_LEVELS:
        dst = ts._words(bits.size)
        ff.grid_inflate(g, r, src.data_ptr(), dst.data_ptr())
        inflated = ts._read(dst, bits.shape, what=("inflate", r))
        assert np.array_equal(inflated, vc.a4_inflated(r)), ("dsm_grid_inflate against the checker", r)
        assert np.array_equal(gc.pack(got["dist2"] <= r * r), inflated), ("the field's level set against dsm_grid_inflate", r)
        assert np.array_equal(gc.pack(exp["dist2"] <= r * r), inflated), ("the checker's level set against dsm_grid_inflate", r)
    assert np.array_equal(src.cpu().numpy().view(np.uint32), bits)
    ff.close()


# ------------------------------------------------------------------ B1. the carve past one trip
def test_b1_carve_past_one_trip(api):
    ff = ts._engine(api, sc.CAM_70)
    frames = vc.b1_frames()
    for k, f in enumerate(frames):
        ts._load(ff, k, f[2])
    old = np.array(vc.b1_old())
    second = vc.b1_second_trip()
    for flags in vc.B1_FLAGS:
        exp, n_exp = vc.b1_expected(flags)
        bits, n = ts._carve(api, ff, vc.b1_grid(flags), frames, [0, 1], old=old, flags=flags, what=("B1", flags))
        bad = gc.unpack(bits ^ exp, vc.B1_GRID[0])
        assert not bad.any(), ("B1", flags, "voxels that differ in the first trip %d, in the second %d" % ((bad & ~second).sum(), (bad & second).sum()))
        assert n == n_exp, ("B1", flags, n, n_exp)
    ff.close()


# ------------------------------------------------------------------ B2. the classification past every cap
def test_b2_classify_past_every_cap(api):
    g = vc.B2_GRID
    ob, fb = (np.array(a) for a in vc.b2_sets()[2:])
    exp = vc.b2_expected()
    ff = ts._engine(api, sc.CAM_64)
    for planes in (("state", "known_free", "frontier", "cells"), ("cells",), ("state",)):
        got, n, err = ts._classify(api, ff, g, ob, fb, planes=planes, what=("B2", planes))
        assert err is None and n == exp["n_frontier"], ("B2", planes, n, exp["n_frontier"])
        ts._same_space(got, exp, ("B2", planes))
    cap = exp["n_frontier"] // 2
    got, n, err = ts._classify(api, ff, g, ob, fb, cap=cap, what=("B2", "cap"))
    assert err is not None and n == exp["n_frontier"], ("B2", "cap", n)
    ts._same_space(got, dict(exp, cells=exp["cells"][:cap]), ("B2", "cap"))
    ff.close()


# ------------------------------------------------------------------ B3. the carve behind the public upload paths
@pytest.mark.parametrize("g", vc.B3_GRIDS, ids=[sc.grid_id(g) for g in vc.B3_GRIDS])
def test_b3_carve_behind_async_uploads(api, g):
    """A missing wait shows only when the race is lost: this test can miss a real bug, it cannot fail on correct code."""
    cam = sc.CAM_70
    ff = ts._engine(api, cam, slots=2)
    s = sc.make(g, cam)
    p, q = vc.b3_planes()
    img = np.random.default_rng(70).integers(0, 256, (cam.h, cam.w), dtype=np.uint8)
    pin = api.PinnedFrames(ff, 1)
    pin.set(0, img, p)
    pins16 = []
    for scale, op in vc.B3_U16:
        pins16.append(api.PinnedFrames(ff, 1, depth_u16=(scale, op)))
        pins16[-1].set(0, img, q)
    slot, shape = 1, sc.words(s)
    seen = []
    for rnd in range(4):  # P, Q by division, P, Q by multiplication: all in the same slot
        buf = ts._words(int(np.prod(shape)))  # (poisoned: the call replaces it)
        if rnd % 2 == 0:
            ff.frame_upload_async(slot, pin.image(0), pin.depth(0))
            want = p
        else:
            scale, op = vc.B3_U16[rnd // 2]
            ff.frame_upload_async_u16(slot, pins16[rnd // 2].image(0), pins16[rnd // 2].depth(0), scale, op)
            want = api.depth_from_u16(q, scale, op)
        n = ff.grid_carve(ts._spec(api, s), [slot], [vc.B3_POSE], buf.data_ptr(), ts._params(api, s), sc.REPLACE)  # no wait in between
        bits = ts._read(buf, shape, what=(g, rnd))
        back = ff.frame_planes(slot)[1]
        assert back[:, :cam.w].tobytes() == np.ascontiguousarray(want, np.float32).tobytes(), (g, rnd, "the slot holds the frame just uploaded")
        exp, n_exp = sc.host_carve(s, [(vc.B3_POSE, None, back)])
        assert np.array_equal(bits, exp) and n == n_exp, (g, rnd, int(gc.unpack(bits ^ exp, g[0]).sum()))
        seen.append(bits)
        ff.frame_uploads_wait()
    assert np.array_equal(seen[0], seen[2]) and int(gc.unpack(seen[0] ^ seen[1], g[0]).sum()) > 100 and int(gc.unpack(seen[2] ^ seen[3], g[0]).sum()) > 100
    for pf in [pin] + pins16:
        pf.close()
    ff.close()


# ------------------------------------------------------------------ C. one handle, everything interleaved
def _spec(api, s, inflate=0):
    return api.grid_spec(s.origin[:], s.voxel, gc.dims(s), inflate)


def _classify_small(api, ff, ctx):
    ob, fb = (np.array(a) for a in vc.c_small_sets())
    got, n, err = ts._classify(api, ff, vc.C_SMALL, ob, fb, planes=("state", "known_free", "cells"), what="C small")
    assert err is None
    exp = sc.host_classify(ob, fb, vc.C_SMALL[0], planes=("state", "known_free", "cells"))
    assert n == exp["n_frontier"] > 0
    ts._same_space(got, exp, "C small")
    return dict(got, n=n)


def _field_37(api, ff, ctx):
    s = gc.GRID_37
    got = ff.field(2, [ctx["run"]], _spec(api, s), 64)
    b, c = ctx["run"]
    seq = np.concatenate([ctx["store"][b:b + c], gc.keep_select(ctx["live"], 2)])
    assert got["n_surfels"] == len(seq)
    fc.same_fields(got, fc.host_field(gc.host_grid(seq, s)["occupied"], s.nx, 64, voxel=s.voxel), "C field 37x21x13")
    return got


def _classify_big(api, ff, ctx):
    ob, fb = (np.array(a) for a in vc.b2_sets()[2:])
    exp = vc.b2_expected()
    got, n, err = ts._classify(api, ff, vc.B2_GRID, ob, fb, planes=("cells",), what="C big")
    assert err is None and n == exp["n_frontier"]
    ts._same_space(got, exp, "C big")
    return dict(got, n=n)


def _grid_32(api, ff, ctx):
    s = gc.with_inflate(gc.GRID_32, 1)
    got = ff.grid(1, (), _spec(api, s, 1), planes=("occupied", "inflated", "index", "cells"))
    seq = gc.keep_select(ctx["live"], 1)
    exp = gc.host_all(seq, s)
    assert got["n_surfels"] == len(seq) and got["n_cells"] == len(exp["cells"]) > 0
    gc.same_grids(got, exp, "C grid 32x8x4")
    return got


def _distance_a1(api, ff, ctx):
    name = vc.A1_SETS[0]
    got = tf._distance(ff, vc.A1_GRID, 16, _upload(vc.a1_bits(name)[1]), what="C distance")
    fc.same_fields(got, vc.a1_expected(name, 16), "C distance")
    return got


def _inflate_a4(api, ff, ctx):
    bits = vc.a4_case()[1]
    src, dst = _upload(bits), ts._words(bits.size)
    ff.grid_inflate(vc.A4_GRID, 5, src.data_ptr(), dst.data_ptr())
    got = ts._read(dst, bits.shape, what="C inflate")
    assert np.array_equal(got, vc.a4_inflated(5)), "C inflate"
    return {"inflated": got}


def _carve_65(api, ff, ctx):
    s, frames = sc.case((65, 4, 3), "70x44", "oblique")
    ts._load(ff, 0, frames[0][2])
    bits, n = ts._carve(api, ff, s, frames, [0], what="C carve")
    exp, n_exp = sc.expected((65, 4, 3), "70x44", "oblique")
    assert np.array_equal(bits, exp) and n == n_exp > 0, "C carve"
    return {"free": bits, "n": n}


def _field_1(api, ff, ctx):
    s = gc.GRID_1
    got = ff.field(1, (), _spec(api, s), 3)
    seq = gc.keep_select(ctx["live"], 1)
    assert got["n_surfels"] == len(seq)
    fc.same_fields(got, fc.host_field(gc.host_grid(seq, s)["occupied"], 1, 3, voxel=s.voxel), "C field 1x1x1")
    return got


C_STEPS = (_classify_small, _field_37, _classify_big, _grid_32, _distance_a1, _inflate_a4, _carve_65, _field_1, _classify_small)


def _handle_with_map(api):
    ff = ts._engine(api, sc.CAM_70, slots=2)
    run, store, live = tf._map_with_store(api, ff, gc.GRID_37, np.random.default_rng(23))
    return ff, {"run": run, "store": store, "live": live}


def _same_outputs(a, b, what):
    assert set(a) == set(b), what
    for k in a:
        if isinstance(a[k], np.ndarray):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)
        else:
            assert a[k] == b[k], (what, k)


def test_c_one_handle_everything_interleaved(api):
    ff, ctx = _handle_with_map(api)
    before = (ff.store_download(0, ff.store_size())[0].tobytes(), ff.map_download().tobytes())
    results = [step(api, ff, ctx) for step in C_STEPS]  # (every step compares with the checker)
    _same_outputs(results[0], results[-1], "the small classification before and after everything else")
    assert (ff.store_download(0, ff.store_size())[0].tobytes(), ff.map_download().tobytes()) == before
    ff.close()
    for k, step in enumerate(C_STEPS[:-1]):  # the same call on a handle that has done nothing else
        fresh, fresh_ctx = _handle_with_map(api)
        assert fresh_ctx["run"] == ctx["run"]
        _same_outputs(results[k], step(api, fresh, fresh_ctx), ("step %d against a fresh handle" % (k + 1), step.__name__))
        fresh.close()
