"""What the eight voxel-grid calls refuse, in their own words, and which of two faults each reports.

dsm_grid_compose, dsm_grid_inflate, dsm_grid_distance, dsm_field_compose, dsm_grid_carve, dsm_grid_classify, dsm_grid_view and
dsm_grid_components on ONE small handle (a 64 x 32 frame slot, 300 records): one fault per check a call makes, with the code and the
text of dsm_last_error as the source has it; pairs of faults, with the text that wins; the three DSM_E_CAPACITY texts with the count
returned and nothing written past the cap; and after every fault one valid call of the same kind.  An 8 x 8 x 8 grid, and 33 x 3 x 2
(two words a row, 12 words a set) where the size of a bit set decides.  Every refusal comes before anything reaches the device, so
the pointers of a refused call are addresses inside one device buffer and nothing more."""
import ctypes as C

import numpy as np
import pytest

import render_cases as rc
import space_cases as sc

pytestmark = pytest.mark.gpu

CAM = sc.Cam(64, 32, 57.25, 55.5, 31.3, 15.7)
VIEW_CAM = (16, 8, 14.5, 13.25, 7.7, 3.9, 0.3, 30.0)
ORIGIN, VOXEL = (-1.0, -1.0, 0.5), 0.25
D8, D33 = (8, 8, 8), (33, 3, 2)
SET8, SET33 = 256, 48  # bytes of a bit set
GUARD = 0x4d
DIMS_28 = "grid %d x %d x %d: a dimension below 1 or more than 2^28 voxels"
DIMS_26 = "grid %d x %d x %d: a dimension below 1 or more than 2^26 voxels"


@pytest.fixture(scope="module")
def api():
    import torch
    torch.cuda.init()  # (before the library's first HIP call, as in the other GPU suites)
    from densesurfelmapping_amd import api as api_mod
    return api_mod


class Bench:
    """the handle, one device buffer cut into 4 KiB parts (more than any plane of the two grids), and the raw calls with valid
    arguments unless told otherwise"""

    def __init__(self, api):
        import torch
        self.api = api
        self.ff = api.FusionFunctions()
        self.ff.initialize(CAM.w, CAM.h, CAM.fx, CAM.fy, CAM.cx, CAM.cy, 30.0, 0.3, surfel_capacity=1 << 15, frame_slots=2)
        m = rc.render_records(np.random.default_rng(3), 300, api.SURFEL_DTYPE, ut=np.arange(300) % 9 + 1)
        m["last_update"] = np.arange(300) % 3
        self.ff.map_upload(m)
        assert self.ff.store_deactivate(1) == (0, 100)
        for slot in (0, 1):
            self.ff.frame_planes(slot, depth=sc.depth_plane(CAM, 5 + slot))
        self.pool = torch.zeros(16 * 4096, dtype=torch.uint8, device="cuda")
        assert self.pool.data_ptr() % 256 == 0
        self.lib, self.h = self.ff._lib, self.ff._h
        self.keep = []

    def part(self, k):
        return self.pool.data_ptr() + 4096 * k

    def err(self):
        return self.lib.dsm_last_error(self.h).decode()

    def spec(self, dims=D8, inflate=1, **kw):
        g = self.api.grid_spec(ORIGIN, VOXEL, dims, inflate)
        for k, v in kw.items():
            if k == "origin":
                g.origin[:] = v
            else:
                setattr(g, k, v)
        return g

    @staticmethod
    def poses(n=1, **entries):
        """n identity poses, column-major; entries: {"f<frame>_<k>": value}"""
        p = np.tile(np.eye(4, dtype=np.float32).reshape(16), (n, 1))
        for key, v in entries.items():
            f, k = key[1:].split("_")
            p[int(f), int(k)] = v
        return np.ascontiguousarray(p)

    # ---- the eight calls; every keyword replaces one valid argument
    def compose(self, select=1, n_seg=1, spec="valid", flags=0, planes="valid", on_device=0, cells_cap=512, same=False, odd=False):
        api = self.api
        g = self.spec() if spec == "valid" else spec
        b, c = np.array([0], np.int32), np.array([100], np.int32)
        n, nc = C.c_int32(-1), C.c_int32(-1)
        st = None
        if planes == "valid":
            st, self.out = api.grid_outputs(g if spec is not None else self.spec(), ("occupied", "inflated", "index", "cells"), None, cells_cap)
            self.out["cells"][:] = -7
        elif planes == "none":
            st = api._GridPlanes(None, None, None, None, 0)
        elif planes == "device":
            st = api._GridPlanes(self.part(2), self.part(2) if same else self.part(3), self.part(4) + (2 if odd else 0), self.part(5), cells_cap)
        rc_ = self.lib.dsm_grid_compose(self.h, select, n_seg, b.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), None if g is None else C.byref(g), flags,
                                        None if st is None else C.byref(st), on_device, C.byref(n), C.byref(nc))
        self.n, self.n_cells = n.value, nc.value
        return rc_

    def inflate(self, dims=D8, radius=1, src=0, dst=None):
        src = self.part(0) + src if src is not None else None
        dst = self.part(2) if dst is None else (None if dst == "null" else self.part(0) + dst)
        return self.lib.dsm_grid_inflate(self.h, dims[0], dims[1], dims[2], radius, src, dst)

    def distance(self, dims=D8, max_dist=3, voxel=VOXEL, src=0, planes="valid"):
        """planes: (dist2, nearest, distance) as offsets from part(0), None for a plane not asked for"""
        api = self.api
        src = self.part(0) + src if src is not None else None
        if planes == "valid":
            planes = (2 * 4096, 3 * 4096, 4 * 4096)
        st = None if planes is None else api._FieldPlanes(*(None if o is None else self.part(0) + o for o in planes))
        return self.lib.dsm_grid_distance(self.h, dims[0], dims[1], dims[2], max_dist, voxel, src, None if st is None else C.byref(st))

    def field(self, select=1, spec="valid", max_dist=3, flags=0, planes="valid", on_device=0):
        api = self.api
        g = self.spec(inflate=0) if spec == "valid" else spec
        b, c = np.array([0], np.int32), np.array([100], np.int32)
        n = C.c_int32(-1)
        st = None
        if planes == "valid":
            st, self.out = api.field_outputs(g if g is not None else self.spec(), api.FIELD_PLANES, None)
        elif planes is not None:
            st = api._FieldPlanes(*(None if o is None else self.part(0) + o for o in planes))
        return self.lib.dsm_field_compose(self.h, select, 1, b.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), None if g is None else C.byref(g), max_dist,
                                          flags, None if st is None else C.byref(st), on_device, C.byref(n))

    def carve(self, spec="valid", params="valid", flags=0, slots=(0,), poses="valid", inv=None, free=2 * 4096, n_frames=None):
        api = self.api
        g = self.spec(inflate=0) if spec == "valid" else spec
        p = api.carve_params(near_dist=0.3, far_dist=8.0, margin=0.1) if params == "valid" else params
        sl = None if slots is None else np.ascontiguousarray(slots, np.int32)
        ps = self.poses(len(slots) if slots is not None else 1) if isinstance(poses, str) else poses
        n = C.c_int64(-1)
        rc_ = self.lib.dsm_grid_carve(self.h, None if g is None else C.byref(g), None if p is None else C.byref(p), flags,
                                      (len(sl) if sl is not None else 1) if n_frames is None else n_frames, None if sl is None else sl.ctypes.data_as(C.c_void_p),
                                      None if ps is None else ps.ctypes.data_as(C.c_void_p), None if inv is None else inv.ctypes.data_as(C.c_void_p),
                                      None if free is None else self.part(0) + free, C.byref(n))
        self.n = n.value
        return rc_

    def classify(self, dims=D8, occ=0, fre=4096, planes="valid", cells_cap=16):
        """planes: (state, known_free, frontier, cells) as offsets from part(0)"""
        api = self.api
        if planes == "valid":
            planes = (2 * 4096, 3 * 4096, 4 * 4096, 5 * 4096)
        st = None if planes is None else api._SpacePlanes(*(None if o is None else self.part(0) + o for o in planes), cells_cap)
        n = C.c_int32(-1)
        rc_ = self.lib.dsm_grid_classify(self.h, dims[0], dims[1], dims[2], None if occ is None else self.part(0) + occ, None if fre is None else self.part(0) + fre,
                                         None if st is None else C.byref(st), C.byref(n))
        self.n = n.value
        return rc_

    def view(self, spec="valid", camera="valid", flags=0, poses="valid", inv=None, occ=0, fre=4096, target=None, scores=6 * 4096, scores_on_device=1,
             visible=8 * 4096, n_poses=None):
        api = self.api
        g = self.spec(inflate=0) if spec == "valid" else spec
        cam = api.render_camera(VIEW_CAM) if camera == "valid" else camera
        ps = self.poses(2) if isinstance(poses, str) else poses
        at = lambda o: None if o is None else self.part(0) + o
        return self.lib.dsm_grid_view(self.h, None if g is None else C.byref(g), None if cam is None else C.byref(cam), flags,
                                      (len(ps) if ps is not None else 1) if n_poses is None else n_poses, None if ps is None else ps.ctypes.data_as(C.c_void_p),
                                      None if inv is None else inv.ctypes.data_as(C.c_void_p), at(occ), at(fre), at(target), at(scores), scores_on_device, at(visible))

    def components(self, dims=D8, connectivity=26, min_count=1, src=0, tag=None, label=2 * 4096, table=4 * 4096, table_cap=4):
        api = self.api
        at = lambda o: None if o is None else self.part(0) + o
        st = None if label == "null planes" else api._ComponentPlanes(at(label), at(table), table_cap)
        n, n_all = C.c_int32(-1), C.c_int32(-1)
        rc_ = self.lib.dsm_grid_components(self.h, dims[0], dims[1], dims[2], connectivity, min_count, at(src), at(tag), None if st is None else C.byref(st),
                                           C.byref(n), C.byref(n_all))
        self.n, self.n_all = n.value, n_all.value
        return rc_


@pytest.fixture(scope="module")
def bench(api):
    b = Bench(api)
    yield b
    b.ff.close()


def _refused(b, call, text, what, code=None, **kw):
    """the call with `kw` is refused with `text`; then it serves with valid arguments"""
    code = b.api.DSM_E_INVALID if code is None else code
    got = call(**kw)
    assert got == code, (what, got, b.err())
    assert b.err() == text, what
    b.pool.zero_()
    assert call() == b.api.DSM_OK, (what, "the valid call after it", b.err())


P = 4096  # one part of the pool


def test_inflate(bench):
    b = bench
    r = lambda text, what, **kw: _refused(b, b.inflate, text, what, **kw)
    r("grid inflate: null source or destination, or the same", "null source", src=None)
    r("grid inflate: null source or destination, or the same", "null destination", dst="null")
    r("grid inflate: null source or destination, or the same", "the same", dst=0)
    r("grid inflate: a bit set not 4-byte aligned", "source off by 2", src=2)
    r("grid inflate: a bit set not 4-byte aligned", "destination off by 1", dst=P + 1)
    r(DIMS_28 % (0, 8, 8), "nx 0", dims=(0, 8, 8))
    r(DIMS_28 % (8, 8, -1), "nz -1", dims=(8, 8, -1))
    r(DIMS_28 % (1 << 14, 1 << 14, 2), "2^29 voxels", dims=(1 << 14, 1 << 14, 2))
    r(DIMS_28 % ((1 << 28) + 1, 1, 1), "2^28 + 1 voxels", dims=((1 << 28) + 1, 1, 1))
    r(DIMS_28 % (1 << 30, 1 << 30, 1 << 30), "2^90 voxels", dims=(1 << 30, 1 << 30, 1 << 30))
    r("grid inflate: source and destination overlap", "the last word of the source", dst=SET8 - 4)
    r("grid inflate: source and destination overlap", "the source's last word, destination first", src=SET8 - 4, dst=0)
    r("grid inflate: source and destination overlap", "33 x 3 x 2: the second word of the last row", dims=D33, dst=SET33 - 4)
    r("grid inflate 17 outside 0..16", "radius 17", radius=17)
    r("grid inflate -1 outside 0..16", "radius -1", radius=-1)
    # two faults
    r("grid inflate: null source or destination, or the same", "first and last", dst=0, radius=17)
    r(DIMS_28 % (0, 8, 8), "bad dims with an overlap", dims=(0, 8, 8), dst=4)
    r("grid inflate: a bit set not 4-byte aligned", "alignment before dims", src=2, dims=(8, 0, 8))
    r("grid inflate: source and destination overlap", "overlap before radius", dst=SET8 - 4, radius=17)
    # sets that touch are no overlap: 12 words a set at 33 x 3 x 2
    assert b.inflate(dims=D33, dst=SET33) == b.api.DSM_OK, b.err()
    assert b.inflate(dims=D33, src=SET33, dst=0) == b.api.DSM_OK, b.err()


def test_distance(bench):
    b = bench
    r = lambda text, what, **kw: _refused(b, b.distance, text, what, **kw)
    r("grid distance: null source or planes", "null source", src=None)
    r("grid distance: null source or planes", "null planes", planes=None)
    r("grid distance: the bit set is not 4-byte aligned", "source off by 2", src=2)
    r(DIMS_26 % (8, 0, 8), "ny 0", dims=(8, 0, 8))
    r(DIMS_26 % (1 << 13, 1 << 13, 2), "2^27 voxels", dims=(1 << 13, 1 << 13, 2))
    r("grid distance: max_dist outside 1..64", "max_dist 0", max_dist=0)
    r("grid distance: max_dist outside 1..64", "max_dist 65", max_dist=65)
    r("grid distance: no output plane", "no plane", planes=(None, None, None))
    r("grid distance: voxel not finite or not positive", "voxel 0 with a distance plane", voxel=0.0)
    r("grid distance: voxel not finite or not positive", "voxel inf with a distance plane", voxel=float("inf"))
    assert b.distance(voxel=0.0, planes=(2 * P, 3 * P, None)) == b.api.DSM_OK, "the voxel edge matters to the distance plane alone"
    r("grid distance: two output planes are the same memory", "dist2 is nearest", planes=(2 * P, 2 * P, None))
    r("grid distance: a device plane is not aligned to its element", "dist2 off by 1", planes=(2 * P + 1, None, None))
    r("grid distance: a device plane is not aligned to its element", "nearest off by 2", planes=(None, 3 * P + 2, None))
    assert b.distance(planes=(2 * P + 2, None, None)) == b.api.DSM_OK, "dist2 is aligned to 2 bytes"
    r("grid distance: a plane overlaps the source", "dist2 ends in the source", src=P, planes=(P - 1024 + 2, None, None))  # 512 x 2 bytes
    r("grid distance: a plane overlaps the source", "nearest begins in the source's last word", planes=(None, SET8 - 4, None))
    r("grid distance: a plane overlaps the source", "33 x 3 x 2: distance in the last word", dims=D33, planes=(None, None, SET33 - 4))
    assert b.distance(dims=D33, planes=(None, None, SET33)) == b.api.DSM_OK, b.err()
    assert b.distance(dims=D33, src=2 * 198, planes=(0, None, None)) == b.api.DSM_OK, "198 voxels of dist2, then the source"
    # two faults
    r("grid distance: null source or planes", "first and last", src=None, planes=(None, 16, None))
    r(DIMS_26 % (0, 8, 8), "bad dims with an overlap", dims=(0, 8, 8), planes=(None, 4, None))
    r("grid distance: max_dist outside 1..64", "max_dist before the planes", max_dist=0, planes=(None, None, None))
    r("grid distance: two output planes are the same memory", "same memory before overlap", planes=(8, 8, None))


def test_classify(bench):
    b = bench
    r = lambda text, what, **kw: _refused(b, b.classify, text, what, **kw)
    r("grid classify: null source or planes", "null occupied", occ=None)
    r("grid classify: null source or planes", "null free", fre=None)
    r("grid classify: null source or planes", "null planes", planes=None)
    r("grid classify: a bit set is not 4-byte aligned", "free off by 2", fre=P + 2)
    r(DIMS_28 % (8, 8, 0), "nz 0", dims=(8, 8, 0))
    r(DIMS_28 % (1 << 14, 1 << 14, 2), "2^29 voxels", dims=(1 << 14, 1 << 14, 2))
    r("grid classify: no output plane", "no plane", planes=(None, None, None, None))
    r("cells_cap -1", "cells_cap -1", cells_cap=-1)
    r("grid classify: a device plane is not 4-byte aligned", "frontier off by 2", planes=(None, None, 4 * P + 2, None))
    assert b.classify(planes=(2 * P + 1, None, None, None)) == b.api.DSM_OK, "the state plane is bytes"
    r("grid classify: two output planes are the same memory", "known_free is frontier", planes=(None, 3 * P, 3 * P, None))
    r("grid classify: a plane overlaps a source", "state ends in free", planes=(P - 511, None, None, None))
    r("grid classify: a plane overlaps a source", "known_free in occupied's last word", planes=(None, SET8 - 4, None, None))
    r("grid classify: a plane overlaps a source", "cells of no room, inside occupied", planes=(None, None, 4 * P, 8), cells_cap=0)
    r("grid classify: a plane overlaps a source", "cells capped at the voxels reach free", planes=(None, None, 4 * P, P - 2048 + 4), cells_cap=1 << 20)
    r("grid classify: a plane overlaps a source", "33 x 3 x 2: frontier in free's last word", dims=D33, planes=(None, None, P + SET33 - 4, None))
    assert b.classify(dims=D33, planes=(None, None, P + SET33, None)) == b.api.DSM_OK, b.err()
    assert b.classify(planes=(None, None, 4 * P, P - 2048), cells_cap=1 << 20) == b.api.DSM_OK, "no more cells than voxels: they end where free begins"
    # two faults
    r("grid classify: null source or planes", "first and last", occ=None, planes=(None, 8, None, None))
    r(DIMS_28 % (0, 8, 8), "bad dims with an overlap", dims=(0, 8, 8), planes=(None, 4, None, None))
    r("cells_cap -1", "cells_cap before alignment", cells_cap=-1, planes=(None, 3 * P + 2, None, 5 * P))
    r("grid classify: two output planes are the same memory", "same memory before overlap", planes=(None, 8, 8, None))


def test_components(bench):
    b = bench
    r = lambda text, what, **kw: _refused(b, b.components, text, what, **kw)
    rec = b.api.COMPONENT_DTYPE.itemsize
    r("grid components: null source or planes", "null source", src=None)
    r("grid components: null source or planes", "null planes", label="null planes")
    r("grid components: the bit set or the tag plane is not 4-byte aligned", "source off by 2", src=2)
    r("grid components: the bit set or the tag plane is not 4-byte aligned", "tag off by 1", tag=6 * P + 1)
    r(DIMS_26 % (-3, 8, 8), "nx -3", dims=(-3, 8, 8))
    r(DIMS_26 % (1 << 13, 1 << 13, 2), "2^27 voxels", dims=(1 << 13, 1 << 13, 2))
    r("grid components: connectivity 18, neither 6 nor 26", "connectivity 18", connectivity=18)
    r("grid components: min_count 0", "min_count 0", min_count=0)
    r("grid components: no output plane", "no plane", label=None, table=None)
    r("table_cap -2", "table_cap -2", table_cap=-2)
    r("grid components: a device plane is not aligned to its element", "label off by 2", label=2 * P + 2)
    r("grid components: a device plane is not aligned to its element", "table off by 4", table=4 * P + 4)
    r("grid components: two output planes are the same memory", "label is table", label=2 * P, table=2 * P)
    r("grid components: two output planes are the same memory", "table begins in the label's last voxel", label=2 * P, table=2 * P + 2048 - 8)
    r("grid components: two output planes are the same memory", "a table of no room inside the label", label=2 * P, table=2 * P + 8, table_cap=0)
    r("grid components: a plane overlaps the source", "label in the source's last word", label=SET8 - 4, table=None)
    r("grid components: a plane overlaps the source", "the table's last record reaches the source", src=P, table=P - 4 * rec + 8, label=None)
    r("grid components: a plane overlaps the source", "33 x 3 x 2: label in the last word", dims=D33, label=SET33 - 4, table=None)
    assert b.components(dims=D33, label=SET33, table=None) == b.api.DSM_OK, b.err()
    r("grid components: a plane overlaps the tag plane", "label in the tag plane's last voxel", tag=6 * P, label=6 * P + 2048 - 4, table=None)
    r("grid components: a plane overlaps the tag plane", "33 x 3 x 2: 198 tags", dims=D33, tag=6 * P, label=6 * P + 4 * 198 - 4, table=None)
    assert b.components(dims=D33, tag=6 * P, label=6 * P + 4 * 198, table=None) == b.api.DSM_OK, b.err()
    # two faults
    r("grid components: null source or planes", "first and last", src=None, tag=6 * P, label=6 * P + 4)
    r(DIMS_26 % (0, 8, 8), "bad dims with an overlap", dims=(0, 8, 8), label=4, table=None)
    r("grid components: connectivity 7, neither 6 nor 26", "connectivity before min_count", connectivity=7, min_count=0)
    r("grid components: a plane overlaps the source", "the source before the tag plane", tag=P, label=8, table=P + 8)


def test_compose(bench):
    b, api = bench, bench.api
    r = lambda text, what, **kw: _refused(b, b.compose, text, what, **kw)
    size = C.sizeof(api._GridSpec)
    r("null grid spec or planes", "null spec", spec=None)
    r("null grid spec or planes", "null planes", planes=None)
    r("grid flags 0x2", "flags 2", flags=2)
    r("dsm_grid_spec struct_size %d, not %d" % (size - 4, size), "struct_size", spec=b.spec(struct_size=size - 4))
    r("grid origin 1 is not finite", "origin", spec=b.spec(origin=(0.0, float("inf"), 0.0)))
    r("grid voxel -1", "voxel -1", spec=b.spec(voxel=-1.0))
    r("grid voxel inf", "voxel inf", spec=b.spec(voxel=float("inf")))
    r(DIMS_28 % (8, 0, 8), "ny 0", spec=b.spec(dims=(8, 0, 8)))
    r(DIMS_28 % (1 << 14, 1 << 14, 2), "2^29 voxels", spec=b.spec(dims=(1 << 14, 1 << 14, 2)), planes="device", on_device=1)
    r("grid inflate 17 outside 0..16", "inflate 17", spec=b.spec(inflate=17))
    r("no output plane", "no plane", planes="none")
    r("cells_cap -1", "cells_cap -1", cells_cap=-1, planes="device", on_device=1)
    r("device output not 4-byte aligned", "index off by 2", planes="device", on_device=1, odd=True)
    r("two output planes are the same memory", "occupied is inflated", planes="device", on_device=1, same=True)
    r("cloud select 3", "select 3", select=3)
    r("null/negative run list", "n_segments -1", n_seg=-1)
    # two faults
    r("null grid spec or planes", "first and last", planes=None, select=3)
    r(DIMS_28 % (0, 8, 8), "bad dims with planes of the same memory", spec=b.spec(dims=(0, 8, 8)), planes="device", on_device=1, same=True)
    r("grid flags 0x4", "flags before the spec", flags=4, spec=b.spec(voxel=0.0))
    r("dsm_grid_spec struct_size 0, not %d" % size, "struct_size before the rest of the spec", spec=b.spec(struct_size=0, dims=(0, 0, 0)))
    r("two output planes are the same memory", "planes before the sequence", planes="device", on_device=1, same=True, select=3)


def test_field(bench):
    b, api = bench, bench.api
    r = lambda text, what, **kw: _refused(b, b.field, text, what, **kw)
    size = C.sizeof(api._GridSpec)
    r("null grid spec or field planes", "null spec", spec=None)
    r("null grid spec or field planes", "null planes", planes=None)
    r("field flags 0x1", "flags 1", flags=1)
    r("dsm_grid_spec struct_size %d, not %d" % (size + 4, size), "struct_size", spec=b.spec(struct_size=size + 4))
    r("grid voxel 0", "voxel 0", spec=b.spec(voxel=0.0))
    r(DIMS_28 % (8, 8, 0), "nz 0", spec=b.spec(dims=(8, 8, 0)))
    r("grid inflate -1 outside 0..16", "inflate -1", spec=b.spec(inflate=-1))
    r("field of %d x %d x %d: more than 2^26 voxels" % (1 << 13, 1 << 13, 2), "2^27 voxels", spec=b.spec(dims=(1 << 13, 1 << 13, 2)), planes=(2 * P, None, None),
      on_device=1)
    r("field: max_dist outside 1..64", "max_dist 65", max_dist=65)
    r("field: no output plane", "no plane", planes=(None, None, None))
    r("field: two output planes are the same memory", "nearest is distance", planes=(None, 2 * P, 2 * P), on_device=1)
    r("field: a device plane is not aligned to its element", "distance off by 2", planes=(None, None, 2 * P + 2), on_device=1)
    r("cloud select 3", "select 3", select=3)
    # two faults
    r("null grid spec or field planes", "first and last", planes=None, select=3)
    r(DIMS_28 % (0, 8, 8), "bad dims with planes of the same memory", spec=b.spec(dims=(0, 8, 8)), planes=(2 * P, 2 * P, None), on_device=1)
    r("grid %d x %d x %d: a dimension below 1 or more than 2^28 voxels" % (1 << 14, 1 << 14, 2), "the grid's limit before the field's",
      spec=b.spec(dims=(1 << 14, 1 << 14, 2)), planes=(2 * P, None, None), on_device=1)
    r("field: max_dist outside 1..64", "max_dist before the sequence", max_dist=0, select=3)


def test_field_refuses_the_sequence_before_its_scratch_grows(bench):
    """2^26 voxels ask for more than 400 MB of `field` scratch; a bad sequence with that valid spec is refused with the device's free
    memory as it was (within 128 MiB: other work on the device is not ours to hold still)"""
    import torch
    b = bench
    big = b.spec(dims=(1 << 10, 1 << 10, 1 << 6), inflate=0)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    assert b.field(spec=big, planes=(2 * P, None, None), on_device=1, select=3) == b.api.DSM_E_INVALID
    assert b.err() == "cloud select 3"
    after = torch.cuda.mem_get_info()[0]
    print("free device memory: %d before, %d after" % (before, after))
    assert before - after < (128 << 20), "the field scratch grew before the sequence was checked"
    assert b.field() == b.api.DSM_OK, b.err()


def test_carve(bench):
    b, api = bench, bench.api
    r = lambda text, what, **kw: _refused(b, b.carve, text, what, **kw)
    size, psize = C.sizeof(api._GridSpec), C.sizeof(api._CarveParams)
    cp = lambda **kw: api.carve_params(dict(dict(near_dist=0.3, far_dist=8.0, margin=0.1), **kw))
    bad_size = cp()
    bad_size.struct_size = psize - 4
    nan = float("nan")
    r("grid carve: null spec, params, slots or poses", "null spec", spec=None)
    r("grid carve: null spec, params, slots or poses", "null params", params=None)
    r("grid carve: null spec, params, slots or poses", "null slots", slots=None)
    r("grid carve: null spec, params, slots or poses", "null poses", poses=None)
    r("grid carve: the free set is null or not 4-byte aligned", "null set", free=None)
    r("grid carve: the free set is null or not 4-byte aligned", "set off by 2", free=2 * P + 2)
    r("carve flags 0x4", "flags 4", flags=4)
    r("dsm_grid_spec struct_size %d, not %d" % (size - 4, size), "spec struct_size", spec=b.spec(struct_size=size - 4))
    r("grid origin 2 is not finite", "origin", spec=b.spec(origin=(0.0, 0.0, float("-inf"))))
    r(DIMS_28 % (8, 8, 0), "nz 0", spec=b.spec(dims=(8, 8, 0)))
    r("dsm_carve_params struct_size %d, not %d" % (psize - 4, psize), "params struct_size", params=bad_size)
    r("carve depth range (0, 8)", "near 0", params=cp(near_dist=0.0))
    r("carve depth range (2, 1.5)", "far below near", params=cp(near_dist=2.0, far_dist=1.5))
    r("carve depth range (0.5, inf)", "far inf", params=cp(near_dist=0.5, far_dist=float("inf")))
    r("carve margin -0.5", "margin -0.5", params=cp(margin=-0.5))
    r("carve margin inf", "margin inf", params=cp(margin=float("inf")))
    r("carve of 0 frames, outside 1..32", "no frames", n_frames=0)
    r("carve of 33 frames, outside 1..32", "33 frames", n_frames=33)
    r("frame slot 2 out of range [0,2)", "slot 2", slots=(2,))
    r("frame slot -1 out of range [0,2)", "slot -1 at frame 1", slots=(1, -1))
    r("carve frame 0: pose entry 5 is not finite", "a NaN pose entry", poses=b.poses(1, f0_5=nan))
    r("carve frame 1: pose entry 14 is not finite", "an infinite pose entry at frame 1", slots=(0, 1), poses=b.poses(2, f1_14=float("inf")))
    r("carve frame 1: pose entry 3 is not finite", "a NaN entry of a given inverse", slots=(0, 1), inv=b.poses(2, f1_3=nan))
    r("carve frame 0: pose entry 2 is not finite", "the lower entry of pose and inverse", poses=b.poses(1, f0_9=nan), inv=b.poses(1, f0_2=nan))
    # two faults
    r("grid carve: null spec, params, slots or poses", "first and last", params=None, poses=b.poses(1, f0_0=nan))
    r(DIMS_28 % (0, 8, 8), "bad dims with a bad frame count", spec=b.spec(dims=(0, 8, 8)), n_frames=0)
    r("carve frame 0: pose entry 0 is not finite", "a NaN pose at frame 0, a bad slot at frame 1", slots=(0, 7), poses=b.poses(2, f0_0=nan))
    r("frame slot 7 out of range [0,2)", "a bad slot and a NaN pose both at frame 0", slots=(7,), poses=b.poses(1, f0_0=nan))
    r("frame slot 7 out of range [0,2)", "a bad slot at frame 0, a NaN pose at frame 1", slots=(7, 0), poses=b.poses(2, f1_0=nan))
    r("dsm_grid_spec struct_size 0, not %d" % size, "the spec before the params", spec=b.spec(struct_size=0), params=bad_size)
    r("carve margin -1", "the params before the frames", params=cp(margin=-1.0), n_frames=0)
    assert b.carve(slots=(0, 1), inv=b.poses(2)) == api.DSM_OK and b.n >= 0, b.err()


def test_view(bench):
    b, api = bench, bench.api
    r = lambda text, what, **kw: _refused(b, b.view, text, what, **kw)
    size = C.sizeof(api._GridSpec)
    nan = float("nan")

    def cam(**kw):
        c = api.render_camera(VIEW_CAM)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    reach = "view pose %d: the camera's voxel is more than 4096 voxels outside the grid along axis %d"
    r("grid view: null spec, camera or poses", "null spec", spec=None)
    r("grid view: null spec, camera or poses", "null camera", camera=None)
    r("grid view: null spec, camera or poses", "null poses", poses=None)
    r("grid view: null source", "null occupied", occ=None)
    r("grid view: null source", "null free", fre=None)
    r("grid view: no output", "no output", scores=None, visible=None)
    r("view flags 0x2", "flags 2", flags=2)
    r("grid view: a device pointer is not 4-byte aligned", "target off by 2", target=2 * P + 2)
    r("grid view: a device pointer is not 4-byte aligned", "device scores off by 2", scores=6 * P + 2)
    r("dsm_grid_spec struct_size %d, not %d" % (size - 4, size), "struct_size", spec=b.spec(struct_size=size - 4))
    r(DIMS_28 % (8, -8, 8), "ny -8", spec=b.spec(dims=(8, -8, 8)))
    r("render image 0 x 8 outside 1..8192", "width 0", camera=cam(width=0))
    r("render camera fx 0 fy 13.25 cx 7.7 cy 3.9", "fx 0", camera=cam(fx=0.0))
    r("render depth range (0.3, 0.25)", "far below near", camera=cam(far_dist=0.25))
    r("view of 0 poses, outside 1..4096", "no poses", n_poses=0)
    r("view of 4097 poses, outside 1..4096", "4097 poses", n_poses=4097)
    r("view pose 1: pose entry 6 is not finite", "a NaN entry at pose 1", poses=b.poses(2, f1_6=nan))
    r("view pose 0: pose entry 15 is not finite", "an infinite entry of a given inverse", inv=b.poses(2, f0_15=float("inf")))
    r(reach % (0, 0), "pose 0 far along x", poses=b.poses(2, f0_12=1.0e6))
    r(reach % (1, 2), "pose 1 far below along z", poses=b.poses(2, f1_14=-1.0e6))
    r("grid view: an output overlaps a source", "visible's second pose reaches free", fre=P, visible=P - 2 * SET8 + 4)
    r("grid view: an output overlaps a source", "device scores in the target's last word", target=2 * P, scores=2 * P + SET8 - 4)
    r("grid view: an output overlaps a source", "33 x 3 x 2: visible in occupied's last word", spec=b.spec(dims=D33, inflate=0), visible=SET33 - 4)
    assert b.view(spec=b.spec(dims=D33, inflate=0), visible=SET33) == api.DSM_OK, b.err()
    assert b.view(fre=P, visible=P - 2 * SET8) == api.DSM_OK, "two poses of visible end where free begins"
    r("grid view: the two outputs overlap", "the scores' last bytes in visible", scores=8 * P - 4)
    r("grid view: the two outputs overlap", "visible's last word in the scores", scores=8 * P + 2 * SET8 - 4)
    assert b.view(scores=8 * P + 2 * SET8) == api.DSM_OK, b.err()
    # two faults
    r("grid view: null spec, camera or poses", "first and last", camera=None, scores=8 * P)
    r(DIMS_28 % (0, 8, 8), "bad dims with an overlap", spec=b.spec(dims=(0, 8, 8)), visible=4)
    r(reach % (0, 1), "pose 0 out of reach, pose 1 NaN", poses=b.poses(2, f0_13=1.0e6, f1_0=nan))
    r("view pose 0: pose entry 4 is not finite", "pose 0 NaN and out of reach", poses=b.poses(2, f0_4=nan, f0_12=1.0e6))
    r("grid view: a device pointer is not 4-byte aligned", "alignment before the spec", visible=8 * P + 2, spec=b.spec(voxel=0.0))
    r("render image 16 x 9000 outside 1..8192", "the camera before the poses", camera=cam(height=9000), n_poses=0)
    r("grid view: an output overlaps a source", "a source before the other output", visible=4, scores=8)
    # host scores serve as well
    out = np.zeros(2, api.VIEW_SCORE_DTYPE)
    assert b.lib.dsm_grid_view(b.h, C.byref(b.spec(inflate=0)), C.byref(cam()), 0, 2, b.poses(2).ctypes.data_as(C.c_void_p), None, b.part(0), b.part(1), None,
                               out.ctypes.data_as(C.c_void_p), 0, None) == api.DSM_OK, b.err()


# ------------------------------------------------------------------ the three DSM_E_CAPACITY texts
def test_capacity_of_compose(bench):
    b, api = bench, bench.api
    assert b.compose(cells_cap=512) == api.DSM_OK, b.err()
    n_surfels, cells = b.n, b.n_cells
    full = b.out["cells"][:cells].copy()
    assert cells > 2 and (full >= 0).all() and (b.out["cells"][cells:] == -7).all()
    assert b.compose(cells_cap=2) == api.DSM_E_CAPACITY
    assert b.err() == "%d cells, room for 2" % cells
    assert (b.n, b.n_cells) == (n_surfels, cells), "both counts come back with the refusal"
    got = b.out["cells"]
    assert len(got) == 2 and np.array_equal(got, full[:2]), "the first two cells"
    # with a longer array behind the same cap nothing is written past it
    st, out = api.grid_outputs(b.spec(), ("cells",), None, 8)
    st.cells_cap = 2
    out["cells"][:] = -7
    seg = np.array([0, 100], np.int32)
    n, nc = C.c_int32(0), C.c_int32(0)
    assert b.lib.dsm_grid_compose(b.h, 1, 1, seg[:1].ctypes.data_as(C.c_void_p), seg[1:].ctypes.data_as(C.c_void_p), C.byref(b.spec()), 0, C.byref(st), 0, C.byref(n),
                                  C.byref(nc)) == api.DSM_E_CAPACITY
    assert b.err() == "%d cells, room for 2" % cells and nc.value == cells
    assert np.array_equal(out["cells"][:2], full[:2]) and (out["cells"][2:] == -7).all()
    assert b.compose() == api.DSM_OK, b.err()


def _bits8(voxels):
    """a bit set of the 8 x 8 x 8 grid (a word a row) with the voxels (x, y, z) set"""
    a = np.zeros((8, 8, 1), np.uint32)
    for x, y, z in voxels:
        a[z, y, 0] |= np.uint32(1 << x)
    return a


def _put(b, part, a):
    import torch
    raw = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).ravel().copy()).cuda()
    b.pool[4096 * part:4096 * part + raw.numel()] = raw


def _get(b, part, nbytes, dtype):
    return b.pool[4096 * part:4096 * part + nbytes].cpu().numpy().view(dtype).copy()


def test_capacity_of_classify(bench):
    b, api = bench, bench.api
    b.pool.zero_()
    _put(b, 1, _bits8([(1, 1, 1), (5, 2, 6), (3, 3, 3), (3, 4, 3)]))  # free voxels in unknown space: each one a frontier voxel
    b.pool[5 * P:6 * P] = GUARD
    assert b.classify(cells_cap=16) == api.DSM_OK, b.err()
    nf = b.n
    full = _get(b, 5, 64, np.int32)
    assert nf == 4 and (np.diff(full[:nf]) > 0).all() and (_get(b, 5, P, np.uint8)[4 * nf:] == GUARD).all()
    b.pool[5 * P:6 * P] = GUARD
    assert b.classify(cells_cap=1) == api.DSM_E_CAPACITY
    assert b.err() == "4 frontier cells, room for 1" and b.n == 4
    got = _get(b, 5, P, np.uint8)
    assert got[:4].view(np.int32)[0] == full[0] and (got[4:] == GUARD).all(), "nothing written past the cap"
    assert b.classify(cells_cap=0, planes=(None, None, 4 * P, 5 * P)) == api.DSM_E_CAPACITY and b.err() == "4 frontier cells, room for 0"
    assert (_get(b, 5, P, np.uint8)[4:] == GUARD).all()
    assert b.classify() == api.DSM_OK, b.err()


def test_capacity_of_components(bench):
    b, api = bench, bench.api
    rec = api.COMPONENT_DTYPE.itemsize
    b.pool.zero_()
    _put(b, 0, _bits8([(0, 0, 0), (1, 0, 0), (4, 4, 4), (7, 7, 7)]))  # three components
    b.pool[4 * P:5 * P] = GUARD
    assert b.components(table_cap=4) == api.DSM_OK, b.err()
    assert (b.n, b.n_all) == (3, 3)
    full = _get(b, 4, 3 * rec, api.COMPONENT_DTYPE)
    assert list(full["root"]) == [0, 4 * 64 + 4 * 8 + 4, 511] and list(full["count"]) == [2, 1, 1]
    assert (_get(b, 4, P, np.uint8)[3 * rec:] == GUARD).all()
    b.pool[4 * P:5 * P] = GUARD
    assert b.components(table_cap=1) == api.DSM_E_CAPACITY
    assert b.err() == "3 components, room for 1" and (b.n, b.n_all) == (3, 3)
    got = _get(b, 4, P, np.uint8)
    assert got[:rec].tobytes() == full[:1].tobytes() and (got[rec:] == GUARD).all(), "nothing written past the cap"
    # min_count drops the small ones from the count that has to fit
    assert b.components(table_cap=1, min_count=2) == api.DSM_OK and (b.n, b.n_all) == (1, 3), b.err()
    assert b.components(table_cap=0, min_count=1) == api.DSM_E_CAPACITY and b.err() == "3 components, room for 0"
    assert b.components() == api.DSM_OK, b.err()
