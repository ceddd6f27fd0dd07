"""Python mirror of the reference's node class ``SurfelMap`` (surfel_fusion/src/surfel_map.h:48-147) over
the C ABI of include/dsm_surfel_map.h: the three subscriber callbacks, ``save_cloud`` / ``save_mesh`` /
``save_map``, and read-only taps for what the publish_* methods would send.

Messages are plain values instead of ROS types: stamps are ``(sec, nsec)``, poses are 7 doubles
``[px, py, pz, qx, qy, qz, qw]`` (geometry_msgs/Pose).  All state lives in the library: host logic in
csrc/dsm_surfel_map.cpp, surfels in HBM.  No CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import api

ABI_SYMBOLS = (
    "dsm_surfel_map_create", "dsm_surfel_map_destroy", "dsm_surfel_map_last_error",
    "dsm_surfel_map_image_input", "dsm_surfel_map_depth_input", "dsm_surfel_map_orb_results_input",
    "dsm_surfel_map_save_cloud", "dsm_surfel_map_save_mesh", "dsm_surfel_map_save_map",
    "dsm_surfel_map_engine", "dsm_surfel_map_frames_fused", "dsm_surfel_map_dropped_poses", "dsm_surfel_map_pose_count",
    "dsm_surfel_map_get_pose", "dsm_surfel_map_get_links", "dsm_surfel_map_get_attached",
    "dsm_surfel_map_get_inactive_cloud", "dsm_surfel_map_get_cloud", "dsm_surfel_map_get_cloud_device", "dsm_surfel_map_set_publish",
    "dsm_surfel_map_depth_input_u16", "dsm_surfel_map_image_input_color",
    "dsm_surfel_map_get_mesh", "dsm_surfel_map_get_mesh_device", "dsm_surfel_map_save_mesh_binary",
    "dsm_surfel_map_render", "dsm_surfel_map_render_device",
    "dsm_surfel_map_align_last", "dsm_surfel_map_last_pose16",
    "dsm_surfel_map_grid", "dsm_surfel_map_grid_device",
    "dsm_surfel_map_field", "dsm_surfel_map_field_device",
    "dsm_surfel_map_set_free_space", "dsm_surfel_map_free_space_resets", "dsm_surfel_map_free_space", "dsm_surfel_map_free_space_device",
    "dsm_surfel_map_space", "dsm_surfel_map_space_device", "dsm_surfel_map_carve_last",
    "dsm_frontier_query_init", "dsm_surfel_map_frontier_clusters", "dsm_surfel_map_frontier_clusters_device",
    "dsm_view_query_init", "dsm_surfel_map_view_gain", "dsm_surfel_map_view_gain_device",
)

# dsm_cloud_kind of include/dsm_surfel_map.h
CLOUD_ACTIVE, CLOUD_INACTIVE, CLOUD_ALL, CLOUD_NEIGHBOR, CLOUD_RAW = range(5)
CLOUD_KINDS = ("active", "inactive", "all", "neighbor", "raw")

_vp = C.c_void_p


class _FrontierQuery(C.Structure):  # dsm_frontier_query
    _fields_ = [("struct_size", C.c_uint32), ("connectivity", C.c_int32), ("min_count", C.c_int32), ("has_from", C.c_int32), ("from_", C.c_float * 3)]


class _Stamp(C.Structure):
    _fields_ = [("sec", C.c_uint32), ("nsec", C.c_uint32)]


class _PoseMsg(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("px", "py", "pz", "qx", "qy", "qz", "qw")]


class _Publication(C.Structure):
    _fields_ = [("stamp", _Stamp), ("relative_index", C.c_int32), ("fuse_pose", _PoseMsg), ("kinds_mask", C.c_uint32),
                ("points", C.POINTER(C.c_float) * 5), ("n_points", C.c_int32 * 5)]


_PublishFn = C.CFUNCTYPE(None, _vp, C.POINTER(_Publication))


class _MapConfig(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("cam_width", C.c_int32), ("cam_height", C.c_int32),
                ("cam_fx", C.c_float), ("cam_fy", C.c_float), ("cam_cx", C.c_float), ("cam_cy", C.c_float),
                ("fuse_far_distence", C.c_float), ("fuse_near_distence", C.c_float),
                ("drift_free_poses", C.c_int32), ("rgbd", C.c_int32), ("device", C.c_int32),
                ("surfel_capacity", C.c_int32), ("max_buffered_frames", C.c_int32), ("engine_flags", C.c_uint32)]


def _bind(lib):
    if not getattr(lib, "_dsm_surfel_map_bound", False):
        lib.dsm_surfel_map_create.argtypes = [C.POINTER(_MapConfig), C.POINTER(_vp)]
        lib.dsm_surfel_map_destroy.argtypes = [_vp]
        lib.dsm_surfel_map_destroy.restype = None
        lib.dsm_surfel_map_last_error.argtypes = [_vp]
        lib.dsm_surfel_map_last_error.restype = C.c_char_p
        lib.dsm_surfel_map_image_input.argtypes = [_vp, _Stamp, C.c_int32, C.c_int32, C.c_size_t, C.c_char_p, _vp]
        lib.dsm_surfel_map_depth_input.argtypes = [_vp, _Stamp, C.c_int32, C.c_int32, C.c_size_t, C.c_char_p, _vp]
        lib.dsm_surfel_map_image_input_color.argtypes = [_vp, _Stamp, C.c_int32, C.c_int32, C.c_size_t, C.c_char_p, _vp, _vp]
        lib.dsm_surfel_map_depth_input_u16.argtypes = [_vp, _Stamp, C.c_int32, C.c_int32, C.c_size_t, C.c_char_p, _vp, C.c_float, C.c_int32]
        lib.dsm_surfel_map_orb_results_input.argtypes = [_vp, _Stamp, _vp, C.c_int32, _vp, C.c_int32, _Stamp, _vp, _vp]
        for name in ("save_cloud", "save_mesh", "save_map"):
            getattr(lib, "dsm_surfel_map_" + name).argtypes = [_vp, C.c_char_p]
        lib.dsm_surfel_map_engine.argtypes = [_vp]
        lib.dsm_surfel_map_engine.restype = _vp
        lib.dsm_surfel_map_frames_fused.argtypes = [_vp]
        lib.dsm_surfel_map_frames_fused.restype = C.c_int64
        lib.dsm_surfel_map_dropped_poses.argtypes = [_vp]
        lib.dsm_surfel_map_dropped_poses.restype = C.c_int64
        lib.dsm_surfel_map_pose_count.argtypes = [_vp]
        lib.dsm_surfel_map_get_pose.argtypes = [_vp, C.c_int32, _vp, _vp, _vp, _vp, _vp]
        lib.dsm_surfel_map_get_links.argtypes = [_vp, C.c_int32, _vp, C.c_int32]
        lib.dsm_surfel_map_get_attached.argtypes = [_vp, C.c_int32, _vp, C.c_int32, _vp]
        lib.dsm_surfel_map_get_inactive_cloud.argtypes = [_vp, _vp, C.c_int32, _vp]
        lib.dsm_map_size.argtypes = [_vp, _vp]
        lib.dsm_map_download.argtypes = [_vp, _vp, C.c_int32, _vp]
        lib.dsm_last_error.argtypes = [_vp]
        lib.dsm_last_error.restype = C.c_char_p
        if hasattr(lib, "dsm_surfel_map_get_cloud"):  # (the tests' CPU stand-in of the node has no clouds)
            lib.dsm_surfel_map_get_cloud.argtypes = [_vp, C.c_int, _vp, C.c_int32, _vp]
            lib.dsm_surfel_map_get_cloud_device.argtypes = [_vp, C.c_int, _vp, C.c_int32, _vp]
            lib.dsm_surfel_map_set_publish.argtypes = [_vp, C.c_uint32, _PublishFn, _vp]
        if hasattr(lib, "dsm_surfel_map_get_mesh"):  # (nor the device mesh)
            lib.dsm_surfel_map_get_mesh.argtypes = [_vp, C.c_int, _vp, C.c_int32, _vp]
            lib.dsm_surfel_map_get_mesh_device.argtypes = [_vp, C.c_int, _vp, C.c_int32, _vp]
            lib.dsm_surfel_map_save_mesh_binary.argtypes = [_vp, C.c_char_p]
        if hasattr(lib, "dsm_surfel_map_render"):  # (nor the renderer)
            for name in ("dsm_surfel_map_render", "dsm_surfel_map_render_device"):
                getattr(lib, name).argtypes = [_vp, C.c_int, C.POINTER(api._RenderCamera), _vp, C.c_uint32, C.POINTER(api._RenderPlanes), _vp]
        if hasattr(lib, "dsm_surfel_map_align_last"):  # (nor the alignment)
            lib.dsm_surfel_map_align_last.argtypes = [_vp, C.c_int, _vp, C.POINTER(api._AlignParams), C.POINTER(api._AlignResult)]
        if hasattr(lib, "dsm_surfel_map_last_pose16"):
            lib.dsm_surfel_map_last_pose16.argtypes = [_vp, _vp]
        if hasattr(lib, "dsm_surfel_map_grid"):  # (nor the voxel grid)
            for name in ("dsm_surfel_map_grid", "dsm_surfel_map_grid_device"):
                getattr(lib, name).argtypes = [_vp, C.c_int, C.POINTER(api._GridSpec), C.c_uint32, C.POINTER(api._GridPlanes), _vp, _vp]
        if hasattr(lib, "dsm_surfel_map_field"):  # (nor the distance field)
            for name in ("dsm_surfel_map_field", "dsm_surfel_map_field_device"):
                getattr(lib, name).argtypes = [_vp, C.c_int, C.POINTER(api._GridSpec), C.c_int32, C.c_uint32, C.POINTER(api._FieldPlanes), _vp]
        if hasattr(lib, "dsm_surfel_map_set_free_space"):  # (nor free space)
            lib.dsm_surfel_map_set_free_space.argtypes = [_vp, C.POINTER(api._GridSpec), C.POINTER(api._CarveParams), C.c_uint32]
            lib.dsm_surfel_map_free_space_resets.argtypes = [_vp]
            lib.dsm_surfel_map_free_space_resets.restype = C.c_int64
            lib.dsm_surfel_map_free_space.argtypes = [_vp, _vp, _vp]
            lib.dsm_surfel_map_free_space_device.argtypes = [_vp, _vp, _vp]
            for name in ("dsm_surfel_map_space", "dsm_surfel_map_space_device"):
                getattr(lib, name).argtypes = [_vp, C.c_int, C.POINTER(api._SpacePlanes), _vp, _vp]
            lib.dsm_surfel_map_carve_last.argtypes = [_vp, C.POINTER(api._GridSpec), C.POINTER(api._CarveParams), C.c_uint32, _vp]
        if hasattr(lib, "dsm_surfel_map_frontier_clusters"):  # (nor frontier clusters)
            lib.dsm_frontier_query_init.argtypes = [C.POINTER(_FrontierQuery)]
            lib.dsm_frontier_query_init.restype = None
            for name in ("dsm_surfel_map_frontier_clusters", "dsm_surfel_map_frontier_clusters_device"):
                getattr(lib, name).argtypes = [_vp, C.c_int, C.POINTER(_FrontierQuery), _vp, C.c_int32, _vp, _vp, _vp, _vp]
        if hasattr(lib, "dsm_surfel_map_view_gain"):  # (nor viewpoint gain)
            lib.dsm_view_query_init.argtypes = [_vp, C.POINTER(api._ViewQuery)]
            lib.dsm_view_query_init.restype = None
            for name in ("dsm_surfel_map_view_gain", "dsm_surfel_map_view_gain_device"):
                getattr(lib, name).argtypes = [_vp, C.c_int, C.POINTER(api._ViewQuery), C.c_int32, _vp, _vp, _vp]
        lib._dsm_surfel_map_bound = True
    return lib


def _ptr(a):
    return a.ctypes.data_as(_vp)


class SurfelMap:
    """``SurfelMap(nh)`` of the reference with the node's ROS parameters as keyword arguments
    (surfel_map.cpp:13-28; launch defaults of kitti_orb.launch: drift_free_poses = 10)."""

    def __init__(self, cam, drift_free_poses: int = 10, device: int = 0, surfel_capacity: int = 0,
                 max_buffered_frames: int = 0, engine_flags: int = 0, _library=None):
        # engine_flags: 0 or api.DSM_FLAG_EIGEN33_PRODUCTS (a reference built against Eigen >= 3.3, include/dsm_surfel_map.h)
        # _library: tests bind the same class to their CPU stand-in build of the host logic (tests/node_hostemu.cpp)
        self._lib = _bind(_library if _library is not None else api.load_library())
        self.cam = cam
        cfg = _MapConfig(C.sizeof(_MapConfig), cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cam.far, cam.near, drift_free_poses,
                         1 if cam.rgbd else 0, device, surfel_capacity, max_buffered_frames, engine_flags)
        h = _vp()
        rc = self._lib.dsm_surfel_map_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise api.DsmError(rc, "dsm_surfel_map_create failed (no gfx950 device? this package has no CPU fallback)")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._publish_cb = None
            self._lib.dsm_surfel_map_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise api.DsmError(rc, self._lib.dsm_surfel_map_last_error(self._h).decode())

    # ---- subscriber callbacks (ros_node.cpp:24-32)
    def image_input(self, stamp, image, encoding: str = "mono8"):
        img = np.ascontiguousarray(image, dtype=np.uint8)
        self._check(self._lib.dsm_surfel_map_image_input(self._h, _Stamp(*stamp), img.shape[1], img.shape[0], img.strides[0],
                                                         encoding.encode(), _ptr(img)))

    def depth_input(self, stamp, depth, encoding: str = "32FC1"):
        d = np.ascontiguousarray(depth, dtype=np.float32)
        self._check(self._lib.dsm_surfel_map_depth_input(self._h, _Stamp(*stamp), d.shape[1], d.shape[0], d.strides[0],
                                                         encoding.encode(), _ptr(d)))

    def image_input_color(self, stamp, image, encoding: str, weights=None):
        """a colour camera's image, uint8 [H,W,3] ('rgb8' / 'bgr8') or [H,W,4] ('rgba8' / 'bgra8'), converted to grey on the device at
        upload: api.gray_from_color(image, encoding, weights); weights = (wr, wg, wb, shift), None = api.GRAY_OPENCV_14BIT"""
        im = np.ascontiguousarray(image, dtype=np.uint8)
        if im.ndim != 3:
            raise ValueError("image_input_color takes a [H,W,C] image")
        w4 = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32).reshape(4)
        self._check(self._lib.dsm_surfel_map_image_input_color(self._h, _Stamp(*stamp), im.shape[1], im.shape[0], im.strides[0],
                                                               encoding.encode(), _ptr(im), None if w4 is None else _ptr(w4)))

    def depth_input_u16(self, stamp, depth, scale, op="divide", encoding: str = "16UC1"):
        """a sensor's uint16 depth (16UC1), converted to metres on the device at upload: api.depth_from_u16(depth, scale, op)"""
        from .api import depth_op_code
        d = np.ascontiguousarray(depth, dtype=np.uint16)
        self._check(self._lib.dsm_surfel_map_depth_input_u16(self._h, _Stamp(*stamp), d.shape[1], d.shape[0], d.strides[0],
                                                             encoding.encode(), _ptr(d), scale, depth_op_code(op)))

    def orb_results_input(self, stamp, loop_values, loop_path, this_pose, covariance, this_stamp=None):
        lv = np.ascontiguousarray(loop_values, dtype=np.float32)
        lp = np.ascontiguousarray(loop_path, dtype=np.float64).reshape(-1, 7)
        tp = np.ascontiguousarray(this_pose, dtype=np.float64)
        cov = np.ascontiguousarray(covariance, dtype=np.float64)
        assert tp.shape == (7,) and cov.shape == (36,)
        self._check(self._lib.dsm_surfel_map_orb_results_input(
            self._h, _Stamp(*stamp), _ptr(lv), lv.size, _ptr(lp), lp.shape[0], _Stamp(*(this_stamp or stamp)), _ptr(tp), _ptr(cov)))

    def feed(self, event):
        """One event of ``synth.node_messages``."""
        if event[0] == "image":
            self.image_input(event[1], event[2])
        elif event[0] == "depth":
            self.depth_input(event[1], event[2])
        else:
            self.orb_results_input(event[1], event[2], event[3], event[4], event[5])

    def save_cloud(self, path: str):
        self._check(self._lib.dsm_surfel_map_save_cloud(self._h, path.encode()))

    def save_mesh(self, path: str):
        self._check(self._lib.dsm_surfel_map_save_mesh(self._h, path.encode()))

    save_map = save_mesh  # surfel_map.cpp:75-81

    # ---- the mesh as a device product (dsm_mesh_compose)
    def get_mesh(self, layout=api.MESH_VERTEX_REF6, dst_ptr=None, cap=None):
        """save_mesh's hexagons as a vertex buffer built on the GPU: the attached surfels keyframe by keyframe, then the active
        ones with update_times >= 5.  (n, 36) float32 for api.MESH_VERTEX_REF6 (6 x (x y z c c c)), (n, 24) for
        api.MESH_VERTEX_XYZ_RGBA8 (6 x (x y z rgba)) -- or, with dst_ptr (device memory of cap surfels), n.  Triangles:
        FusionFunctions.mesh_indices / dsm_mesh_indices."""
        n = C.c_int32()
        if dst_ptr is not None:
            self._check(self._lib.dsm_surfel_map_get_mesh_device(self._h, layout, _vp(dst_ptr), cap, C.byref(n)))
            return n.value
        rc = self._lib.dsm_surfel_map_get_mesh(self._h, layout, None, 0, C.byref(n))  # the count (DSM_E_CAPACITY unless empty)
        if rc not in (0, api.DSM_E_CAPACITY):
            self._check(rc)
        out = np.zeros((max(n.value, 1), api.MESH_SURFEL_BYTES[layout] // 4), dtype=np.float32)
        self._check(self._lib.dsm_surfel_map_get_mesh(self._h, layout, _ptr(out), n.value, C.byref(n)))
        return out[: n.value]

    def save_mesh_binary(self, path: str):
        """save_mesh's mesh as a binary little-endian PLY (15-byte vertices, 13-byte faces), streamed from the GPU in chunks"""
        self._check(self._lib.dsm_surfel_map_save_mesh_binary(self._h, path.encode()))

    # ---- the map as images (dsm_render_compose)
    def render(self, kind="all", camera=None, pose=None, flags=0, planes=api.RENDER_PLANES, dst_ptrs=None):
        """What `camera` (None: the node's; api.render_camera's forms) at `pose` (4x4 cam -> world or 16 column-major floats; None:
        the pose of the latest fuse) sees of the surfels of cloud `kind` ("active" / "inactive" / "all" / "neighbor" or CLOUD_*):
        a dict of [height, width] arrays "depth" float32, "index" int32 (for "all": the surfel's number in get_mesh), "normal"
        float32 [.., 3], "intensity" uint8, plus "n_surfels" -- or, with dst_ptrs = {plane: device pointer}, n_surfels."""
        k = self._kind(kind)
        cam = None if camera is None else api.render_camera(camera)
        shape_cam = cam if cam is not None else api.render_camera(self.cam)
        p = None
        if pose is not None:
            p = np.asarray(pose, np.float32)
            p = api.pose_to_colmajor(p) if p.shape == (4, 4) else np.ascontiguousarray(p.reshape(16))
        st, out = api.render_outputs(shape_cam, planes, dst_ptrs)
        n = C.c_int32()
        fn = self._lib.dsm_surfel_map_render if dst_ptrs is None else self._lib.dsm_surfel_map_render_device
        self._check(fn(self._h, k, None if cam is None else C.byref(cam), None if p is None else _ptr(p), flags, C.byref(st), C.byref(n)))
        if dst_ptrs is not None:
            return n.value
        out["n_surfels"] = n.value
        return out

    # ---- the map as a voxel grid (dsm_grid_compose)
    def grid(self, kind="all", voxel=0.1, dims=(64, 64, 32), centre=None, inflate=0, spec=None, flags=0, planes=("occupied", "inflated", "cells"),
             dst_ptrs=None, cells_cap=None):
        """The surfels of cloud `kind` ("active" / "inactive" / "all" / "neighbor" or CLOUD_*) as an occupancy grid of `dims` voxels of
        edge `voxel` around `centre` (None: the translation of the latest fuse's pose), on the lattice of multiples of `voxel`
        (api.grid_spec_around) and inflated by `inflate` voxels -- or in the grid `spec` (api.grid_spec).  Returns api.FusionFunctions.grid's
        dict with the spec used as "spec" -- or, with dst_ptrs = {plane: device pointer}, (n_surfels, n_cells).  More cells than
        cells_cap: DsmError with code DSM_E_CAPACITY and .n_cells = the count needed."""
        k = self._kind(kind)
        if spec is None:
            if centre is None:
                centre = self.last_pose()[:3, 3]
            spec = api.grid_spec_around(centre, voxel, dims, inflate)
        n, nc = C.c_int32(0), C.c_int32(0)
        auto = dst_ptrs is None and cells_cap is None and "cells" in planes
        st, out = api.grid_outputs(spec, planes, dst_ptrs, 4096 if auto else cells_cap)
        fn = self._lib.dsm_surfel_map_grid if dst_ptrs is None else self._lib.dsm_surfel_map_grid_device
        rc = fn(self._h, k, C.byref(spec), flags, C.byref(st), C.byref(n), C.byref(nc))
        if rc == api.DSM_E_CAPACITY and auto:
            st, out = api.grid_outputs(spec, planes, None, nc.value)
            rc = fn(self._h, k, C.byref(spec), flags, C.byref(st), C.byref(n), C.byref(nc))
        if rc == api.DSM_E_CAPACITY:  # (as FusionFunctions.grid: the count needed travels with the error)
            e = api.DsmError(rc, self._lib.dsm_surfel_map_last_error(self._h).decode())
            e.n_cells, e.n_surfels, e.planes = nc.value, n.value, out
            raise e
        self._check(rc)
        if dst_ptrs is not None:
            return n.value, nc.value
        if "cells" in out:
            out["cells"] = out["cells"][: nc.value]
        out["n_surfels"], out["n_cells"], out["spec"] = n.value, nc.value, spec
        return out

    # ---- the map as a distance field (dsm_field_compose)
    def field(self, kind="all", voxel=0.1, dims=(64, 64, 32), centre=None, max_dist=16, spec=None, flags=0, planes=api.FIELD_PLANES, dst_ptrs=None):
        """The truncated Euclidean distance field, out to `max_dist` voxels, of the occupied set that grid() gives for the same `kind`
        and grid: `dims` voxels of edge `voxel` around `centre` (None: the translation of the latest fuse's pose), or the grid `spec`.
        Returns api.FusionFunctions.field's dict with the spec used as "spec" -- or, with dst_ptrs = {plane: device pointer},
        n_surfels."""
        k = self._kind(kind)
        if spec is None:
            if centre is None:
                centre = self.last_pose()[:3, 3]
            spec = api.grid_spec_around(centre, voxel, dims)
        st, out = api.field_outputs(spec, planes, dst_ptrs)
        n = C.c_int32(0)
        fn = self._lib.dsm_surfel_map_field if dst_ptrs is None else self._lib.dsm_surfel_map_field_device
        self._check(fn(self._h, k, C.byref(spec), int(max_dist), flags, C.byref(st), C.byref(n)))
        if dst_ptrs is not None:
            return n.value
        out["n_surfels"], out["spec"] = n.value, spec
        return out

    # ---- free and unknown space (dsm_grid_carve, dsm_grid_classify)
    def set_free_space(self, spec=None, params=None, flags=0):
        """From the next fuse on every fused frame is carved into a device bit set the node owns, in the grid `spec` (api.grid_spec /
        grid_spec_around; None: switched off, the default).  params: api.carve_params' forms; flags: 0 or api.CARVE_TRUST_INFINITE.
        A new spec clears the set, and so does every loop-closure warp (free_space_resets counts those)."""
        if spec is None:
            self._space_spec = None
            self._check(self._lib.dsm_surfel_map_set_free_space(self._h, None, None, 0))
            return
        p = api.carve_params(params)
        self._check(self._lib.dsm_surfel_map_set_free_space(self._h, C.byref(spec), C.byref(p), int(flags)))
        self._space_spec = spec

    @property
    def free_space_resets(self) -> int:
        return int(self._lib.dsm_surfel_map_free_space_resets(self._h))

    def free_space(self, dst_ptr=None):
        """The accumulated free set: (uint32 [nz, ny, wx], its population count) -- or, with a device pointer, the count."""
        n = C.c_int64(0)
        if dst_ptr is not None:
            self._check(self._lib.dsm_surfel_map_free_space_device(self._h, _vp(dst_ptr), C.byref(n)))
            return n.value
        spec = getattr(self, "_space_spec", None)
        out = np.zeros(api.grid_shapes(spec)[1] if spec is not None else (1, 1, 1), np.uint32)
        self._check(self._lib.dsm_surfel_map_free_space(self._h, _ptr(out), C.byref(n)))
        return out, n.value

    def space(self, kind="all", planes=api.SPACE_PLANES, dst_ptrs=None, cells_cap=None):
        """The occupied set of grid(kind) in the accumulator's grid classified against the accumulated free set.  Returns a dict of
        the `planes` asked for -- "state" uint8 [nz, ny, nx] (api.SPACE_UNKNOWN / _FREE / _OCCUPIED), "known_free" and "frontier"
        uint32 [nz, ny, wx], "cells" int32 [n_frontier] (the frontier's linear indices, ascending) -- plus "n_surfels", "n_frontier"
        and "spec"; cells_cap None: the list is sized by a second call.  With dst_ptrs = {plane: device pointer}: (n_surfels,
        n_frontier).  More frontier voxels than cells_cap: DsmError with code DSM_E_CAPACITY and .n_frontier = the count needed."""
        k = self._kind(kind)
        spec = getattr(self, "_space_spec", None)
        n, nf = C.c_int32(0), C.c_int32(0)
        auto = dst_ptrs is None and cells_cap is None and "cells" in planes
        fn = self._lib.dsm_surfel_map_space if dst_ptrs is None else self._lib.dsm_surfel_map_space_device
        if spec is None and dst_ptrs is None:  # (the library refuses: nothing to size the arrays by)
            self._check(fn(self._h, k, C.byref(api._SpacePlanes()), C.byref(n), C.byref(nf)))
        st, out = api.space_outputs(spec, planes, dst_ptrs, 4096 if auto else cells_cap)
        rc = fn(self._h, k, C.byref(st), C.byref(n), C.byref(nf))
        if rc == api.DSM_E_CAPACITY and auto:
            st, out = api.space_outputs(spec, planes, None, nf.value)
            rc = fn(self._h, k, C.byref(st), C.byref(n), C.byref(nf))
        if rc == api.DSM_E_CAPACITY:
            e = api.DsmError(rc, self._lib.dsm_surfel_map_last_error(self._h).decode())
            e.n_frontier, e.n_surfels, e.planes = nf.value, n.value, out
            raise e
        self._check(rc)
        if dst_ptrs is not None:
            return n.value, nf.value
        if "cells" in out:
            out["cells"] = out["cells"][: nf.value]
        out["n_surfels"], out["n_frontier"], out["spec"] = n.value, nf.value, spec
        return out

    def view_query(self):
        """dsm_view_query_init: the node's own camera with the accumulator's carve range, flags 0, the frontier as target"""
        q = api._ViewQuery()
        self._lib.dsm_view_query_init(self._h, C.byref(q))
        return q

    def view_gain(self, poses, kind="all", camera=None, target="frontier", flags=0, visible=False, dst_ptrs=None):
        """Candidate poses (4x4 cam -> world, row-major numpy; one or many) scored against space(kind): what a camera there would see
        (dsm_grid_view of include/dsm.h).  camera: anything api.render_camera takes, None = view_query()'s; target "frontier" / "none";
        flags api.VIEW_UNKNOWN_BLOCKS or 0.  Returns the scores as an api.VIEW_SCORE_DTYPE array [n_poses], or, with visible=True,
        (scores, the visible sets uint32 [n_poses, nz, ny, wx]).  With dst_ptrs = {"scores": device pointer, "visible": device pointer}
        (either may be missing) both are written on the device and None is returned."""
        k = self._kind(kind)
        q = self.view_query()
        if camera is not None:
            q.camera = api.render_camera(camera)
        q.flags = int(flags)
        q.target = api._VIEW_TARGETS[target] if (target is None or isinstance(target, str)) else int(target)
        ps = api.view_poses(poses)
        if dst_ptrs is not None:
            s, v = dst_ptrs.get("scores"), dst_ptrs.get("visible")
            self._check(self._lib.dsm_surfel_map_view_gain_device(self._h, k, C.byref(q), len(ps), _ptr(ps) if len(ps) else None, _vp(s) if s else None,
                                                                  _vp(v) if v else None))
            return None
        spec = getattr(self, "_space_spec", None)
        scores = np.zeros(len(ps), api.VIEW_SCORE_DTYPE)
        vis = np.zeros((len(ps),) + api.grid_shapes(spec)[1], np.uint32) if visible and spec is not None else None
        self._check(self._lib.dsm_surfel_map_view_gain(self._h, k, C.byref(q), len(ps), _ptr(ps) if len(ps) else None, _ptr(scores) if len(ps) else None,
                                                       None if vis is None else _ptr(vis)))
        return (scores, vis) if visible else scores

    def frontier_clusters(self, kind="all", connectivity=26, min_count=1, origin=None, labels=False, dst_ptrs=None, table_cap=None):
        """The frontier of space(kind) as connected clusters (connectivity 6 or 26) of at least min_count voxels.  origin: a world
        point (x, y, z), e.g. the translation of the last pose; with it every cluster's "tag" is the root of the known-free region
        (6-connected) that holds the cluster's root voxel, and "from_root" that of the region holding `origin` (-1: outside the grid or
        not known free): a cluster is reachable through known-free space iff tag == from_root.  Returns a dict: "table"
        (api.COMPONENT_DTYPE, ascending by root), "n_all" (the clusters before the filter), "from_root", "spec", and "labels" (int32
        [nz, ny, nx]: the root of each frontier voxel's cluster, -1 elsewhere) when asked for.  table_cap None: the table is sized by a
        second call.  With dst_ptrs = {"table": device pointer, "label": device pointer} (either may be missing) and table_cap:
        (n_clusters, n_all, from_root).  More clusters than table_cap: DsmError with code DSM_E_CAPACITY and .n_clusters."""
        k = self._kind(kind)
        spec = getattr(self, "_space_spec", None)
        q = _FrontierQuery()
        self._lib.dsm_frontier_query_init(C.byref(q))
        q.connectivity, q.min_count = int(connectivity), int(min_count)
        if origin is not None:
            q.has_from = 1
            q.from_[:] = [float(v) for v in np.asarray(origin, np.float32).reshape(3)]
        n, n_all, root = C.c_int32(0), C.c_int32(0), C.c_int32(-1)
        if dst_ptrs is not None:
            t, l = dst_ptrs.get("table"), dst_ptrs.get("label")
            rc = self._lib.dsm_surfel_map_frontier_clusters_device(self._h, k, C.byref(q), _vp(t) if t else None, int(table_cap or 0), _vp(l) if l else None,
                                                                   C.byref(n), C.byref(n_all), C.byref(root))
            if rc == api.DSM_E_CAPACITY:
                e = api.DsmError(rc, self._lib.dsm_surfel_map_last_error(self._h).decode())
                e.n_clusters, e.n_all, e.from_root = n.value, n_all.value, root.value
                raise e
            self._check(rc)
            return n.value, n_all.value, root.value
        auto = table_cap is None
        lab = np.zeros(api.grid_shapes(spec)[2], np.int32) if labels and spec is not None else None
        table = np.zeros(max(1, 1024 if auto else int(table_cap)), api.COMPONENT_DTYPE)
        cap = 1024 if auto else int(table_cap)

        def call():
            return self._lib.dsm_surfel_map_frontier_clusters(self._h, k, C.byref(q), _ptr(table), cap, None if lab is None else _ptr(lab), C.byref(n),
                                                              C.byref(n_all), C.byref(root))
        rc = call()
        if rc == api.DSM_E_CAPACITY and auto:
            cap = n.value
            table = np.zeros(cap, api.COMPONENT_DTYPE)
            rc = call()
        if rc == api.DSM_E_CAPACITY:
            e = api.DsmError(rc, self._lib.dsm_surfel_map_last_error(self._h).decode())
            e.n_clusters, e.n_all, e.from_root, e.table = n.value, n_all.value, root.value, table[:cap]
            raise e
        self._check(rc)
        out = {"table": table[: n.value].copy(), "n_all": n_all.value, "from_root": root.value, "spec": spec}
        if labels:
            out["labels"] = lab
        return out

    def carve_last(self, spec, free_ptr, params=None, flags=0):
        """One carve of the latest fused frame, with the pose it was fused with, into the caller's bit set [nz, ny, wx] of the grid
        `spec` at the device pointer free_ptr (api.FusionFunctions.grid_carve's rules)."""
        p = api.carve_params(params)
        self._check(self._lib.dsm_surfel_map_carve_last(self._h, C.byref(spec), C.byref(p), int(flags), _vp(free_ptr)))

    # ---- the latest frame against the map (dsm_align_frame)
    def align_last(self, kind="active", pose_guess=None, params=None):
        """The depth frame of the latest fuse aligned, point to plane, against the surfels of cloud `kind` ("active" / "inactive" /
        "all" / "neighbor" or CLOUD_*) seen by the node's camera at `pose_guess` (4x4 cam -> world or 16 column-major floats; None:
        the pose of the latest fuse).  params: api.align_params' forms.  Returns api.align_result's dict; nothing is changed."""
        g = None
        if pose_guess is not None:
            g = np.asarray(pose_guess, np.float32)
            g = api.pose_to_colmajor(g) if g.shape == (4, 4) else np.ascontiguousarray(g.reshape(16))
        p = api.align_params(params)
        r = api._AlignResult()
        self._check(self._lib.dsm_surfel_map_align_last(self._h, self._kind(kind), None if g is None else _ptr(g), C.byref(p), C.byref(r)))
        return api.align_result(r)

    def last_pose(self) -> np.ndarray:
        """the pose of the latest fuse as the engine was given it: 4x4 float32, cam -> world (align_last's and render's default)"""
        p = np.zeros(16, np.float32)
        self._check(self._lib.dsm_surfel_map_last_pose16(self._h, _ptr(p)))
        return p.reshape(4, 4).T.copy()

    # ---- taps
    @property
    def frames_fused(self) -> int:
        return int(self._lib.dsm_surfel_map_frames_fused(self._h))

    @property
    def dropped_poses(self) -> int:
        return int(self._lib.dsm_surfel_map_dropped_poses(self._h))

    @property
    def pose_count(self) -> int:
        return int(self._lib.dsm_surfel_map_pose_count(self._h))

    def local_surfels(self) -> np.ndarray:
        eng = self._lib.dsm_surfel_map_engine(self._h)
        n = C.c_int32()
        rc = self._lib.dsm_map_size(eng, C.byref(n))
        if rc:
            raise api.DsmError(rc, self._lib.dsm_last_error(eng).decode())
        out = np.zeros(max(n.value, 1), dtype=api.SURFEL_DTYPE)
        rc = self._lib.dsm_map_download(eng, _ptr(out), n.value, C.byref(n))
        if rc:
            raise api.DsmError(rc, self._lib.dsm_last_error(eng).decode())
        return out[: n.value]

    def pose(self, i: int):
        cam, loop = np.zeros(7), np.zeros(7)
        n_att, begin, is_local = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.dsm_surfel_map_get_pose(self._h, i, _ptr(cam), _ptr(loop), C.byref(n_att), C.byref(begin), C.byref(is_local)))
        return {"cam_pose": cam, "loop_pose": loop, "n_attached": n_att.value, "points_begin_index": begin.value,
                "is_local": bool(is_local.value), "links": self.links(i)}

    def links(self, i: int):
        out = np.zeros(4096, dtype=np.int32)
        n = self._lib.dsm_surfel_map_get_links(self._h, i, _ptr(out), out.size)
        if n < 0:
            raise api.DsmError(n, "get_links")
        return out[:n].tolist()

    def attached_surfels(self, i: int) -> np.ndarray:
        n = C.c_int32()
        self._lib.dsm_surfel_map_get_attached(self._h, i, None, 0, C.byref(n))
        out = np.zeros(max(n.value, 1), dtype=api.SURFEL_DTYPE)
        self._check(self._lib.dsm_surfel_map_get_attached(self._h, i, _ptr(out), n.value, C.byref(n)))
        return out[: n.value]

    def inactive_cloud(self) -> np.ndarray:
        n = C.c_int32()
        self._lib.dsm_surfel_map_get_inactive_cloud(self._h, None, 0, C.byref(n))
        out = np.zeros((max(n.value, 1), 4), dtype=np.float32)
        self._check(self._lib.dsm_surfel_map_get_inactive_cloud(self._h, _ptr(out), n.value, C.byref(n)))
        return out[: n.value]

    # ---- point-cloud topics (publish_*_pointcloud, surfel_map.cpp:1115-1151, 1283-1454)
    @staticmethod
    def _kind(kind) -> int:
        return CLOUD_KINDS.index(kind) if isinstance(kind, str) else int(kind)

    def cloud(self, kind) -> np.ndarray:
        """The cloud of `kind` (CLOUD_* or its name) for the current state, (n, 4) float32 x y z intensity."""
        k = self._kind(kind)
        n = C.c_int32()
        rc = self._lib.dsm_surfel_map_get_cloud(self._h, k, None, 0, C.byref(n))  # the count (DSM_E_CAPACITY unless empty)
        if rc not in (0, api.DSM_E_CAPACITY):
            self._check(rc)
        out = np.zeros((max(n.value, 1), 4), dtype=np.float32)
        self._check(self._lib.dsm_surfel_map_get_cloud(self._h, k, _ptr(out), n.value, C.byref(n)))
        return out[: n.value]

    def cloud_to_device(self, kind, dst_ptr: int, cap: int) -> int:
        """The cloud of `kind` into device memory (cap points of 16 bytes); returns the count (map_copy_to_device's convention)."""
        n = C.c_int32()
        self._check(self._lib.dsm_surfel_map_get_cloud_device(self._h, self._kind(kind), _vp(dst_ptr), cap, C.byref(n)))
        return n.value

    def set_publish(self, kinds, fn):
        """After every fuse call fn(publication) with publication = {"stamp", "relative_index", "fuse_pose" (7 doubles),
        "clouds": {name: (n, 4) float32 copy}} for the kinds asked for (names or CLOUD_*); kinds empty or fn None: off."""
        mask = 0
        for k in kinds or ():
            mask |= 1 << self._kind(k)
        if not mask or fn is None:
            self._check(self._lib.dsm_surfel_map_set_publish(self._h, 0, _PublishFn(), None))
            self._publish_cb = None
            return

        def trampoline(_user, pub_p):
            pub = pub_p.contents
            p = pub.fuse_pose
            clouds = {}
            for k in range(5):
                if pub.kinds_mask & (1 << k):
                    n = pub.n_points[k]
                    clouds[CLOUD_KINDS[k]] = (np.ctypeslib.as_array(pub.points[k], shape=(n, 4)).copy() if n
                                              else np.zeros((0, 4), np.float32))
            fn({"stamp": (pub.stamp.sec, pub.stamp.nsec), "relative_index": pub.relative_index,
                "fuse_pose": np.array([p.px, p.py, p.pz, p.qx, p.qy, p.qz, p.qw]), "clouds": clouds})

        cb = _PublishFn(trampoline)
        self._check(self._lib.dsm_surfel_map_set_publish(self._h, mask, cb, None))
        self._publish_cb = cb  # kept alive as long as the library may call it
