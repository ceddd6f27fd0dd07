"""The map products in turn on ONE handle, and the checks they share.

1. The scratch of the synchronous calls (dsm_handle's DevScratch members, grown by scratch_grow) is shared: `pub` and `pub_out` by
   eight entry points with different layouts, `grid_planes` by grid and classify, `field` by both field calls, `store_tmp` by erase
   and the warps.  Small sizes, larger ones, small again, the products interleaved: every output bit for bit what the suites' own
   expectation builders say (render_cases, grid_cases, field_cases, space_cases, mesh_cases, align_cases, the cloud suite's numpy
   restatement) -- never another run of the library.
2. The sequence check (check_sequence, pose_finite) in front of cloud, mesh, render, grid, field and align: one table of faults,
   the code each call returns, the text of dsm_last_error, and the order in which two faults are seen."""
import ctypes as C

import numpy as np
import pytest

import align_cases as ac
import field_cases as fc
import grid_cases as gc
import mesh_cases as mc
import render_cases as rc
import space_cases as sc
import test_gpu_clouds as clouds

pytestmark = pytest.mark.gpu

GUARD = 0x4d
N_GUARD = 256
CAM = sc.Cam(64, 32, 57.25, 55.5, 31.3, 15.7)  # the handle's camera: pitch == w
CAM_16 = rc.Camera(16, 8, 14.5, 13.25, 7.7, 3.9, 0.3, 30.0)
CAM_96 = rc.Camera(96, 48, 83.0, 80.5, 47.6, 23.2, 0.3, 30.0)
GRID_8 = gc.spec((-1.0, -1.0, 0.5), 0.25, (8, 8, 4), 1)
GRID_40 = gc.spec((-2.5, -1.5, 0.75), 0.125, (40, 24, 8), 2)


@pytest.fixture(scope="module")
def api():
    import torch
    torch.cuda.init()  # (before the library's first HIP call, as in the other GPU suites)
    from densesurfelmapping_amd import api as api_mod
    return api_mod


def _engine(api):
    ff = api.FusionFunctions()
    ff.initialize(CAM.w, CAM.h, CAM.fx, CAM.fy, CAM.cx, CAM.cy, 30.0, 0.3, surfel_capacity=1 << 15, frame_slots=2)
    return ff


def _device(a):
    """a device copy of the array's bytes with guard bytes behind it"""
    import torch
    a = np.ascontiguousarray(a)
    t = torch.full((a.nbytes + N_GUARD,), GUARD, dtype=torch.uint8, device="cuda")
    t[:a.nbytes] = torch.from_numpy(a.view(np.uint8).ravel()).cuda()
    return t


def _back(t, like):
    a = t.cpu().numpy()
    assert (a[like.nbytes:] == GUARD).all(), "guard bytes written"
    return a[:like.nbytes].view(like.dtype).reshape(like.shape).copy()


class Handle:
    """one handle and what the test knows of its state: the store and the map as numpy records"""

    def __init__(self, api):
        self.api, self.ff = api, _engine(api)
        self.rng = np.random.default_rng(61)
        self.store = np.zeros(0, api.SURFEL_DTYPE)
        self.live = self.store

    def load(self, n, keys):
        """a map of n records, none with update_times 0; those with last_update in `keys` go to the store, a run per key: the runs"""
        m = rc.render_records(self.rng, n, self.api.SURFEL_DTYPE, ut=self.rng.integers(1, 12, n))
        m["last_update"] = np.arange(n) % 3
        self.ff.map_upload(m)
        runs = [self.ff.store_deactivate(k) for k in keys]
        self.store, self.live = self.ff.store_download(0, self.ff.store_size())[0], self.ff.map_download()
        for (b, c), k in zip(runs, keys):
            assert c == (m["last_update"] == k).sum() and (self.store[b:b + c]["last_update"] == k).all()
        return runs

    def seq(self, select, segs):
        """the store's runs first, then the map part"""
        return np.concatenate([self.store[b:b + c] for b, c in segs] + [rc.keep_select(self.live, select)])

    # ---- the products, each against its suite's expectation
    def cloud(self, select, segs, what):
        exp = np.concatenate([clouds._expect(self.live, select)] + [clouds._xyzi(self.store[b:b + c]) for b, c in segs])  # the map part FIRST here
        clouds._same(self.ff.cloud_compose(select, segs), exp, (what, "cloud"))
        return len(exp)

    def mesh(self, select, segs, layout, what):
        exp = mc.host_vertices(self.seq(select, segs), layout)
        mc.same_vertices(self.ff.mesh_compose(select, segs, layout), exp, layout, (what, "mesh"))
        return len(exp)

    def indices(self, n, what):
        got = self.ff.mesh_indices(n)
        assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), mc.expect_faces(n)), (what, "indices")

    def render(self, select, segs, cam, pose, what):
        seq = self.seq(select, segs)
        got = self.ff.render(select, segs, cam, pose)
        assert got["n_surfels"] == len(seq), what
        exp = rc.host_render(seq, cam, pose)
        rc.same_planes(got, exp, (what, "render"))
        return exp

    def grid(self, select, segs, s, flags, what):
        seq = self.seq(select, segs)
        got = self.ff.grid(select, segs, self.api.grid_spec(s.origin[:], s.voxel, gc.dims(s), s.inflate), flags, planes=("occupied", "inflated", "index", "cells"))
        exp = gc.host_all(seq, s, flags)
        assert got["n_surfels"] == len(seq) and got["n_cells"] == len(exp["cells"]), what
        gc.same_grids(got, exp, (what, "grid"))
        return exp

    def field(self, select, segs, s, r, occupied, what):
        got = self.ff.field(select, segs, self.api.grid_spec(s.origin[:], s.voxel, gc.dims(s), 0), r)
        fc.same_fields(got, fc.host_field(occupied, s.nx, r, voxel=s.voxel), (what, "field"))

    def distance(self, s, r, bits, what):
        """dsm_grid_distance of a caller's bit set, all three planes on the device"""
        exp = fc.host_field(bits, s.nx, r, voxel=s.voxel)
        src = _device(bits)
        bufs = {k: _device(np.zeros_like(exp[k])) for k in fc.PLANES}
        self.ff.grid_distance(gc.dims(s), r, s.voxel, src.data_ptr(), {k: t.data_ptr() for k, t in bufs.items()})
        fc.same_fields({k: _back(bufs[k], exp[k]) for k in fc.PLANES}, exp, (what, "distance"))

    def carve(self, s, seed, what):
        """the depth plane of `seed` into slot 0, carved into an empty set: the free bits"""
        g = sc.make(gc.dims(s), CAM, origin=tuple(s.origin[:]), voxel=s.voxel)
        plane = sc.depth_plane(CAM, seed)
        self.ff.frame_planes(0, depth=plane)
        frames = [(rc.IDENTITY.copy(), None, plane)]
        exp, n_exp = sc.host_carve(g, frames)
        buf = _device(np.zeros_like(exp))
        n = self.ff.grid_carve(self.api.grid_spec(g.origin[:], g.voxel, gc.dims(s), 0), [0], [rc.IDENTITY], buf.data_ptr(),
                               self.api.carve_params(near_dist=g.near_d, far_dist=g.far_d, margin=g.margin))
        assert n == n_exp and np.array_equal(_back(buf, exp), exp), (what, "carve")
        return exp

    def classify(self, s, occupied, free, what):
        exp = sc.host_classify(occupied, free, s.nx)
        occ, fre = _device(occupied), _device(free)
        cells = np.zeros(max(exp["n_frontier"], 1), np.int32)
        bufs = {k: _device(np.zeros_like(exp[k])) for k in ("state", "known_free", "frontier")}
        bufs["cells"] = _device(cells)
        n = self.ff.grid_classify(gc.dims(s), occ.data_ptr(), fre.data_ptr(), {k: t.data_ptr() for k, t in bufs.items()}, cells_cap=exp["n_frontier"])
        assert n == exp["n_frontier"], (what, "classify")
        for k in ("state", "known_free", "frontier"):
            assert np.array_equal(_back(bufs[k], exp[k]), exp[k]), (what, "classify", k)
        assert np.array_equal(_back(bufs["cells"], cells)[:n], exp["cells"]), (what, "classify cells")

    def frame_cloud(self, what):
        image, depth = clouds._adversarial_frame(self.rng, CAM.w, CAM.h)
        self.ff.frame_upload(1, image, depth)
        pose7 = np.concatenate([self.rng.normal(size=3) * 10, self.rng.normal(size=4)])
        clouds._same(self.ff.frame_cloud(1, pose7), clouds._raw_expect(image, depth, pose7, CAM.fx, CAM.fy, CAM.cx, CAM.cy), (what, "frame cloud"))

    def align(self, select, segs, model_cam, what):
        """a frame that saw the sequence from the origin, into slot 0, against the sequence from a pose a little off: the checker's
        loop over the checker's render"""
        own = rc.Camera(CAM.w, CAM.h, CAM.fx, CAM.fy, CAM.cx, CAM.cy, 0.3, 30.0)
        cam = own if model_cam is None else model_cam
        seq = self.seq(select, segs)
        plane = rc.host_render(seq, own, rc.IDENTITY)["depth"]  # (pitch == w)
        self.ff.frame_planes(0, depth=plane)
        guess = ac.rigid((0.004, -0.006, 0.005), (0.01, -0.005, 0.015)).astype(np.float32)
        model = rc.host_render(seq, cam, guess)
        p = ac.params(max_iterations=4, stride=1, min_pixels=20)
        want = ac.host_frame(ac.frame_desc(ac.FRAME_64, CAM.pitch), plane, cam, model["depth"], model["normal"], guess, p)
        got = self.ff.align_frame(0, select, segs, guess, model_cam=model_cam, params=self.api.align_params(self.api._AlignParams.from_buffer_copy(bytes(p))))
        want = self.api.align_result(self.api._AlignResult.from_buffer_copy(bytes(want)))
        for k in ("pose", "T", "sums"):
            assert got[k].tobytes() == want[k].tobytes(), (what, "align", k)
        for k in ("status", "iterations", "n_pixels", "scale_log2"):
            assert got[k] == want[k], (what, "align", k, got[k], want[k])
        assert np.float64(got["rms"]).tobytes() == np.float64(want["rms"]).tobytes(), (what, "align rms")
        print("align, %s: status %d after %d iterations, %d pixels" % (what, got["status"], got["iterations"], got["n_pixels"]))
        return got

    def erase(self, begin, n, what):
        """dsm_store_erase with a tail behind the range: it moves down through store_tmp"""
        assert n > 0 and begin + n < len(self.store)
        self.ff.store_erase(begin, n)
        self.store = np.delete(self.store, np.s_[begin:begin + n])
        got, xyzi = self.ff.store_download(0, self.ff.store_size())
        assert got.tobytes() == self.store.tobytes(), (what, "erase")
        clouds._same(xyzi, clouds._xyzi(self.store), (what, "erase, the XYZI shadow"))


def test_products_in_turn_on_one_handle(api):
    h = Handle(api)
    pose = rc.IDENTITY

    def round_of(what, segs, cam, s, r, seed, align_cam, layout):
        h.cloud(2, segs, what)
        n = h.mesh(2, segs, layout, what)
        h.render(1, segs, cam, pose, what)
        h.cloud(1, segs[:1], what + ", again")
        occupied = h.grid(2, segs, s, gc.CELLS_OF_INFLATED, what)["occupied"]
        h.field(2, segs, s, r, occupied, what)
        free = h.carve(s, seed, what)          # (classify needs carve's set: carve, then classify)
        h.classify(s, occupied, free, what)
        h.distance(s, r, free, what)
        h.frame_cloud(what)
        h.render(2, segs, CAM_16, rc.oblique_pose(), what + ", small image")
        got = h.align(1, segs, align_cam, what)
        h.indices(n, what)
        return got

    # small: every buffer's first allocation; mesh needs more of `pub_out` than cloud did, carve more words of `pub` than the
    # sequences did, align's 64 x 32 model more keys than the 16 x 8 render
    run = h.load(300, (1,))
    assert run[0][1] == 100
    round_of("small", run, CAM_16, GRID_8, 3, 5, None, mc.XYZ_RGBA8)
    h.erase(10, 20, "small")
    # larger: two store runs and ~2000 map records.  Mesh outgrows frame_cloud's `pub_out`, the render cloud's and mesh's; the grid
    # outgrows classify's `grid_planes`; every other buffer outgrows what the small round left
    runs = h.load(6000, (1, 2))
    assert [c for _, c in runs] == [2000, 2000] and runs[0][0] == 80
    got = round_of("larger", [runs[1], runs[0]], CAM_96, GRID_40, 8, 7, CAM_96, mc.REF6)
    assert got["iterations"] >= 1 and got["n_pixels"] >= 20, "the larger align has pixels to sum"
    h.erase(100, 1500, "larger")
    # small again, inside the buffers the larger round left: the runs are what the erases left of the first two
    h.load(300, ())
    left = [(0, 80), (80, 500)]
    round_of("small again", left, CAM_16, GRID_8, 3, 5, None, mc.REF6)
    round_of("small again, no runs", [], CAM_16, gc.with_inflate(GRID_8, 0), 1, 6, None, mc.XYZ_RGBA8)
    h.ff.close()


# ------------------------------------------------------------------ 2. the order of the sequence check
CALLS = ("cloud", "mesh", "render", "grid", "field", "align")


def _call(api, ff, name, select, n_segments, begin, count, pose=None):
    """the raw C call with otherwise valid arguments; host destinations.  Returns the code."""
    lib, hd = ff._lib, ff._h
    b = None if begin is None else np.ascontiguousarray(begin, np.int32)
    c = None if count is None else np.ascontiguousarray(count, np.int32)
    bp, cp = (None if b is None else b.ctypes.data_as(C.c_void_p)), (None if c is None else c.ctypes.data_as(C.c_void_p))
    n, n2 = C.c_int32(0), C.c_int32(0)
    p16 = np.ascontiguousarray(api.pose_to_colmajor(rc.IDENTITY) if pose is None else pose, np.float32)
    if name == "cloud":
        out = np.zeros((1 << 12, 4), np.float32)
        return lib.dsm_cloud_compose(hd, select, n_segments, bp, cp, out.ctypes.data_as(C.c_void_p), 0, len(out), C.byref(n))
    if name == "mesh":
        out = np.zeros((1 << 12, 36), np.float32)
        return lib.dsm_mesh_compose(hd, select, n_segments, bp, cp, mc.REF6, out.ctypes.data_as(C.c_void_p), 0, len(out), C.byref(n))
    if name == "render":
        cam = api.render_camera(CAM_16)
        st, out = api.render_outputs(cam, api.RENDER_PLANES, None)
        return lib.dsm_render_compose(hd, select, n_segments, bp, cp, C.byref(cam), p16.ctypes.data_as(C.c_void_p), None, 0, C.byref(st), 0, C.byref(n))
    spec = api.grid_spec(GRID_8.origin[:], GRID_8.voxel, gc.dims(GRID_8), 1)
    if name == "grid":
        st, out = api.grid_outputs(spec, ("occupied", "inflated", "index", "cells"), None, 1 << 10)
        return lib.dsm_grid_compose(hd, select, n_segments, bp, cp, C.byref(spec), 0, C.byref(st), 0, C.byref(n), C.byref(n2))
    if name == "field":
        st, out = api.field_outputs(spec, fc.PLANES, None)
        return lib.dsm_field_compose(hd, select, n_segments, bp, cp, C.byref(spec), 3, 0, C.byref(st), 0, C.byref(n))
    assert name == "align"
    p, r = api.align_params(), api._AlignResult()
    return lib.dsm_align_frame(hd, 0, select, n_segments, bp, cp, None, p16.ctypes.data_as(C.c_void_p), C.byref(p), C.byref(r))


STORE_N = 100  # of the handle with a map below
# fault -> (select, n_segments, begins, counts, the code's name, dsm_last_error's text as the code before the shared check had it)
SINGLE = {
    "select 3": (3, 0, [0], [0], "DSM_E_INVALID", "cloud select 3"),
    "n_segments -1": (1, -1, [0], [0], "DSM_E_INVALID", "null/negative run list"),
    "null arrays": (1, 1, None, None, "DSM_E_INVALID", "null/negative run list"),
    "a run past the store": (1, 1, [STORE_N - 1], [2], "DSM_E_INVALID", "store run 0 = [99,+2) outside [0,100)"),
    "a negative count": (1, 2, [0, 7], [5, -1], "DSM_E_INVALID", "store run 1 = [7,+-1) outside [0,100)"),
}


@pytest.fixture(scope="module")
def handles(api):
    """(a handle with 200 map records and 100 in the store, a handle with no map); every call on them must leave them usable"""
    full, empty = _engine(api), _engine(api)
    m = rc.render_records(np.random.default_rng(3), 300, api.SURFEL_DTYPE, ut=np.arange(300) % 9 + 1)
    m["last_update"] = np.arange(300) % 3
    full.map_upload(m)
    assert full.store_deactivate(1) == (0, STORE_N)
    for ff in (full, empty):
        ff.frame_planes(0, depth=sc.depth_plane(CAM, 5))
    yield full, empty
    full.close()
    empty.close()


def _still_serves(api, ff, name, with_map):
    assert _call(api, ff, name, 1 if with_map else 0, 1 if with_map else 0, [0], [STORE_N if with_map else 0]) == api.DSM_OK, (name, ff._lib.dsm_last_error(ff._h))


@pytest.mark.parametrize("name", CALLS)
def test_sequence_check_precedence(api, handles, name):
    full, empty = handles
    err = lambda ff: ff._lib.dsm_last_error(ff._h).decode()
    for fault, (select, n_seg, b, c, code, text) in SINGLE.items():
        assert _call(api, full, name, select, n_seg, b, c) == getattr(api, code), (name, fault, err(full))
        assert err(full) == text, (name, fault)
        _still_serves(api, full, name, True)
    # no resident map: a state, not an argument
    assert _call(api, empty, name, 1, 0, [0], [0]) == api.DSM_E_STATE, (name, err(empty))
    assert err(empty) == "no resident map", name
    assert _call(api, empty, name, 0, 0, [0], [0]) == api.DSM_OK, (name, "select 0, no map, no runs", err(empty))
    # two faults: the state is seen before the runs are held against the store, a pose before the state
    assert _call(api, empty, name, 1, 1, [0], [5]) == api.DSM_E_STATE, (name, "a run past the (empty) store and no map", err(empty))
    if name in ("render", "align"):
        bad = api.pose_to_colmajor(rc.IDENTITY).astype(np.float32)
        bad[7] = np.inf
        assert _call(api, empty, name, 1, 0, [0], [0], pose=bad) == api.DSM_E_INVALID, (name, "a pose entry and no map", err(empty))
        assert err(empty) == "pose entry 7 is not finite"
        assert _call(api, full, name, 1, 0, [0], [0], pose=bad) == api.DSM_E_INVALID and err(full) == "pose entry 7 is not finite"
    _still_serves(api, empty, name, False)
    _still_serves(api, full, name, True)
