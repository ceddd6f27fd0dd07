"""Host-side mirror of the reference's per-frame fusion interface, over the C ABI of include/dsm.h.

Reference (C++) interface mirrored here, same names and argument meaning:

  * ``FusionFunctions::initialize(w, h, fx, fy, cx, cy, far, near)``
    -- surfel_fusion/src/fusion_functions.h:84-87
  * ``FusionFunctions::fuse_initialize_map(reference_frame_index, image, depth, pose,
    local_surfels, new_surfels)`` -- fusion_functions.h:88-94, fusion_functions.cpp:30-83
  * ``SurfelMap::fuse_map(image, depth, pose, reference_index)`` -- surfel_map.cpp:1060-1113

``SurfelElement`` / ``Superpixel_seed`` arrays are numpy structured arrays with the reference's
byte layout (elements.h:5-31).  All compute happens in the HIP library; if it cannot be loaded, or
no gfx950 device is present, construction raises -- there is no CPU path in this package.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSM_LIB_PATH") or os.path.join(HERE, "libdsm_hip.so")  # override: experiments only

SURFEL_DTYPE = np.dtype(
    [("px", "<f4"), ("py", "<f4"), ("pz", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
     ("size", "<f4"), ("color", "<f4"), ("weight", "<f4"), ("update_times", "<i4"), ("last_update", "<i4")]
)  # elements.h:22-31
SEED_DTYPE = np.dtype(
    {"names": ["x", "y", "size", "norm_x", "norm_y", "norm_z", "posi_x", "posi_y", "posi_z", "view_cos",
               "mean_depth", "mean_intensity", "fused", "stable", "min_eigen_value", "max_eigen_value"],
     "formats": ["<f4"] * 12 + ["u1", "u1", "<f4", "<f4"],
     "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 49, 52, 56],
     "itemsize": 60}
)  # elements.h:5-20
assert SURFEL_DTYPE.itemsize == 44 and SEED_DTYPE.itemsize == 60

DSM_FLAG_NO_GRAPH = 1
DSM_FLAG_UPLOAD_STREAM = 2
DSM_FLAG_WAVE_STAMPS = 4
DSM_FLAG_EIGEN33_PRODUCTS = 8  # the reference's 3x3 products in Eigen >= 3.3's order (include/dsm.h)
DSM_MAX_STAGES = 32
# dsm_status
DSM_OK, DSM_E_INVALID, DSM_E_NO_DEVICE, DSM_E_HIP, DSM_E_CAPACITY, DSM_E_STATE = 0, -1, -2, -3, -4, -5

# every symbol include/dsm.h declares
ABI_SYMBOLS = (
    "dsm_abi_version", "dsm_config_init", "dsm_create", "dsm_destroy", "dsm_last_error",
    "dsm_host_alloc", "dsm_host_free", "dsm_host_pack_frames",
    "dsm_fuse_initialize_map", "dsm_fuse_map", "dsm_fuse_initialize_map_inv", "dsm_fuse_map_inv",
    "dsm_fuse_frame_resident_inv", "dsm_replay_enqueue_inv", "dsm_batch_replay_enqueue_inv",
    "dsm_map_upload", "dsm_map_size", "dsm_map_capacity", "dsm_map_download", "dsm_map_copy_to_device",
    "dsm_map_warp", "dsm_warp_grouped_device", "dsm_map_extract", "dsm_map_append",
    "dsm_store_deactivate", "dsm_store_activate", "dsm_store_erase", "dsm_store_warp", "dsm_store_size",
    "dsm_store_download", "dsm_cloud_compose", "dsm_frame_cloud",
    "dsm_frame_upload", "dsm_frame_upload_device", "dsm_frame_pitch", "dsm_frame_upload_async", "dsm_frames_upload_async", "dsm_frame_uploads_wait", "dsm_fuse_frame_resident", "dsm_replay_enqueue", "dsm_replay_enqueue_host", "dsm_replay_wait",
    "dsm_synchronize", "dsm_last_new_count", "dsm_stream",
    "dsm_batch_create", "dsm_batch_destroy", "dsm_batch_last_error", "dsm_batch_replay_enqueue", "dsm_batch_synchronize",
    "dsm_batch_replay_timed",
    "dsm_get_labels", "dsm_get_seeds", "dsm_seed_count", "dsm_replay_timed", "dsm_debug_wave_stamps", "dsm_debug_set_fit_small_cap", "dsm_debug_tier_counts", "dsm_debug_dropin_stats",
    "dsm_debug_run_stages", "dsm_debug_get_label_buffer", "dsm_debug_set_label_buffer", "dsm_debug_get_seed_state",
    "dsm_debug_set_seed_state",
    # sensor-native uint16 depth, converted on the device
    "dsm_frame_upload_u16", "dsm_frame_upload_device_u16", "dsm_frame_upload_async_u16", "dsm_frames_upload_async_u16",
    "dsm_replay_enqueue_host_u16", "dsm_host_pack_frames_u16", "dsm_debug_get_frame",
    # colour camera images converted to grey on the device, and the format descriptor for both halves of a frame
    "dsm_frame_format_init", "dsm_frame_upload_fmt", "dsm_frame_upload_device_fmt", "dsm_frame_upload_async_fmt",
    "dsm_frames_upload_async_fmt", "dsm_replay_enqueue_host_fmt", "dsm_host_pack_frames_fmt", "dsm_debug_frame_planes",
    # the hexagon mesh as vertex and index buffers
    "dsm_mesh_compose", "dsm_mesh_indices",
    # the map as depth / index / normal / intensity images from any pose
    "dsm_render_compose",
    # a depth frame against the rendered map: one evaluation of the normal equations, and the point-to-plane loop
    "dsm_align_params_init", "dsm_align_equations", "dsm_align_frame",
    # the map as an occupancy voxel grid with inflation and a cell list
    "dsm_grid_spec_init", "dsm_grid_spec_around", "dsm_grid_compose", "dsm_grid_inflate",
    # the truncated Euclidean distance field of the grid
    "dsm_grid_distance", "dsm_field_compose",
    # free space carved by depth frames, the three-state map and its frontier
    "dsm_carve_params_init", "dsm_grid_carve", "dsm_grid_classify",
    # connected components of a bit set of the grid: frontier clusters, obstacles as objects
    "dsm_grid_components",
    # viewpoint gain: candidate camera poses scored against the grid
    "dsm_grid_view",
)

# dsm_frame_upload_u16 & co.: how a uint16 depth value becomes metres (include/dsm.h)
DEPTH_U16_DIVIDE, DEPTH_U16_MULTIPLY = 0, 1
_DEPTH_OPS = {"divide": DEPTH_U16_DIVIDE, "multiply": DEPTH_U16_MULTIPLY}


def depth_op_code(op) -> int:
    """'divide' / 'multiply' (or the DEPTH_U16_* code itself) -> the code; anything else is passed on for the library to refuse"""
    return _DEPTH_OPS[op] if isinstance(op, str) else int(op)


def depth_from_u16(u, scale, op="divide") -> np.ndarray:
    """Host reference of the device conversion: 'divide' = u16.astype(float32) / float32(scale) (TUM PNGs: 5000, KITTI-style: 256),
    'multiply' = u16.astype(float32) * float32(scale) (ROS depth_image_proc's depth * 0.001f); 0 stays 0."""
    u = np.asarray(u, np.uint16).astype(np.float32)
    s = np.float32(scale)
    with np.errstate(over="ignore"):
        return (u / s if depth_op_code(op) == DEPTH_U16_DIVIDE else u * s).astype(np.float32)


# dsm_frame_format (include/dsm.h): image formats, and the grey weights (wr, wg, wb, shift) of
# grey = (R * wr + G * wg + B * wb + (1 << (shift - 1))) >> shift
IMAGE_MONO8, IMAGE_RGB8, IMAGE_BGR8, IMAGE_RGBA8, IMAGE_BGRA8 = 0, 1, 2, 3, 4
IMAGE_FORMATS = {"mono8": IMAGE_MONO8, "rgb8": IMAGE_RGB8, "bgr8": IMAGE_BGR8, "rgba8": IMAGE_RGBA8, "bgra8": IMAGE_BGRA8}
IMAGE_CHANNELS = {IMAGE_MONO8: 1, IMAGE_RGB8: 3, IMAGE_BGR8: 3, IMAGE_RGBA8: 4, IMAGE_BGRA8: 4}
DEPTH_F32, DEPTH_U16 = 0, 1
GRAY_OPENCV_14BIT = (4899, 9617, 1868, 14)   # OpenCV 2.4 / 3.x RGB2Gray<uchar> (as remembered from its source: not checked against a build); the default
GRAY_OPENCV_15BIT = (9798, 19235, 3735, 15)  # OpenCV 4.x 8-bit path (likewise)
GRAY_PIL_L = (19595, 38470, 7471, 16)        # Pillow's convert("L") (checked against Pillow by tests/test_cpu_color.py)


def image_format_code(fmt) -> int:
    """'rgb8' & co. (or the IMAGE_* code itself) -> the code; an unknown code is passed on for the library to refuse"""
    return IMAGE_FORMATS[fmt] if isinstance(fmt, str) else int(fmt)


def image_channels(fmt) -> int:
    return IMAGE_CHANNELS[image_format_code(fmt)]


class _FrameFormat(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("image_format", C.c_int32), ("gray_wr", C.c_int32), ("gray_wg", C.c_int32),
                ("gray_wb", C.c_int32), ("gray_shift", C.c_int32), ("depth_format", C.c_int32), ("depth_scale", C.c_float),
                ("depth_op", C.c_int32)]


def frame_format(image_format="mono8", weights=None, depth_u16=None) -> _FrameFormat:
    """a dsm_frame_format: image_format 'mono8' / 'rgb8' / 'bgr8' / 'rgba8' / 'bgra8' (or an IMAGE_* code), weights = (wr, wg, wb,
    shift) or None = GRAY_OPENCV_14BIT, depth_u16 = (scale, op) or None = float depth.  Nothing is checked here: the library does."""
    wr, wg, wb, shift = GRAY_OPENCV_14BIT if weights is None else weights
    f = _FrameFormat(C.sizeof(_FrameFormat), image_format_code(image_format), int(wr), int(wg), int(wb), int(shift), DEPTH_F32, 1.0, DEPTH_U16_DIVIDE)
    if depth_u16 is not None:
        f.depth_format, f.depth_scale, f.depth_op = DEPTH_U16, float(depth_u16[0]), depth_op_code(depth_u16[1])
    return f


def gray_from_color(image, encoding, weights=None) -> np.ndarray:
    """Host reference of the device conversion: image uint8 [..., 3 or 4] in `encoding` ('rgb8', 'bgr8', 'rgba8', 'bgra8') ->
    uint8 [...] grey = (R * wr + G * wg + B * wb + (1 << (shift - 1))) >> shift in exact integer arithmetic; alpha is ignored."""
    code = image_format_code(encoding)
    ch = IMAGE_CHANNELS[code]
    image = np.asarray(image)
    if ch == 1 or image.dtype != np.uint8 or image.shape[-1] != ch:
        raise ValueError("gray_from_color: a uint8 [..., %d] image in a colour encoding" % ch)
    wr, wg, wb, shift = (int(v) for v in (GRAY_OPENCV_14BIT if weights is None else weights))
    if min(wr, wg, wb) < 0 or not 1 <= shift <= 22 or wr + wg + wb > (1 << shift):
        raise ValueError("gray_from_color: weights >= 0, 1 <= shift <= 22, sum <= 1 << shift")
    first, second, third = (image[..., k].astype(np.int64) for k in range(3))
    r, b = (third, first) if code in (IMAGE_BGR8, IMAGE_BGRA8) else (first, third)
    return ((r * wr + second * wg + b * wb + (1 << (shift - 1))) >> shift).astype(np.uint8)


# dsm_cloud_compose's map part (include/dsm.h dsm_cloud_select)
CLOUD_SELECT_NONE, CLOUD_SELECT_MATURE, CLOUD_SELECT_NONZERO = 0, 1, 2
CLOUD_TILE = 1024  # records per workgroup of the map compaction (dsm_device.h kCloudTile)
# dsm_mesh_compose's vertex layouts (include/dsm.h dsm_mesh_vertex_layout) and their bytes per surfel (six vertices)
MESH_VERTEX_REF6, MESH_VERTEX_XYZ_RGBA8 = 0, 1
MESH_SURFEL_BYTES = {MESH_VERTEX_REF6: 144, MESH_VERTEX_XYZ_RGBA8: 96}
# dsm_render_compose (include/dsm.h): its flag, its planes in the order of dsm_render_planes, and their element types / trailing shape
RENDER_CULL_BACKFACES = 1
RENDER_PLANES = ("depth", "index", "normal", "intensity")
RENDER_PLANE_TYPES = {"depth": (np.float32, ()), "index": (np.int32, ()), "normal": (np.float32, (3,)), "intensity": (np.uint8, ())}
# dsm_grid_compose (include/dsm.h): its flag, its planes in the order of dsm_grid_planes, the largest grid and inflation radius
GRID_CELLS_OF_INFLATED = 1
GRID_PLANES = ("occupied", "inflated", "index", "cells")
GRID_MAX_VOXELS = 1 << 28
GRID_MAX_INFLATE = 16
# dsm_grid_distance / dsm_field_compose (include/dsm.h): dist2 where no set voxel lies within max_dist, the largest max_dist and grid,
# the planes in the order of dsm_field_planes and their element types
FIELD_FAR = 65535
FIELD_MAX_DIST = 64
FIELD_MAX_VOXELS = 1 << 26
FIELD_PLANES = ("dist2", "nearest", "distance")
FIELD_PLANE_TYPES = {"dist2": np.uint16, "nearest": np.int32, "distance": np.float32}
# dsm_grid_carve / dsm_grid_classify (include/dsm.h): the most frames of one carve, its flags, the states of a voxel, the planes in the
# order of dsm_space_planes
CARVE_MAX_FRAMES = 32
CARVE_REPLACE = 1
CARVE_TRUST_INFINITE = 2
SPACE_UNKNOWN, SPACE_FREE, SPACE_OCCUPIED = 0, 1, 2
SPACE_PLANES = ("state", "known_free", "frontier", "cells")


# dsm_align_status, and the layout of the 29 sums (include/dsm.h)
ALIGN_CONVERGED, ALIGN_MAX_ITERATIONS, ALIGN_TOO_FEW, ALIGN_SINGULAR = range(4)
ALIGN_STATUS = ("converged", "max_iterations", "too_few", "singular")
ALIGN_SUMS = 29


class DsmError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"dsm error {code}: {msg}")
        self.code = code


class _Config(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("far_dist", C.c_float), ("near_dist", C.c_float),
                ("huber_range", C.c_double), ("baseline", C.c_double),
                ("disparity_error", C.c_double), ("min_tolerate_diff", C.c_double),
                ("device", C.c_int32), ("surfel_capacity", C.c_int32), ("frame_slots", C.c_int32),
                ("flags", C.c_uint32), ("pipeline_depth", C.c_int32)]


class _RenderCamera(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("near_dist", C.c_float), ("far_dist", C.c_float)]


class _RenderPlanes(C.Structure):
    _fields_ = [("depth", C.c_void_p), ("index", C.c_void_p), ("normal", C.c_void_p), ("intensity", C.c_void_p)]


class _GridSpec(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("origin", C.c_float * 3), ("voxel", C.c_float), ("nx", C.c_int32), ("ny", C.c_int32), ("nz", C.c_int32),
                ("inflate", C.c_int32)]


class _GridPlanes(C.Structure):
    _fields_ = [("occupied", C.c_void_p), ("inflated", C.c_void_p), ("index", C.c_void_p), ("cells", C.c_void_p), ("cells_cap", C.c_int32)]


class _FieldPlanes(C.Structure):
    _fields_ = [("dist2", C.c_void_p), ("nearest", C.c_void_p), ("distance", C.c_void_p)]


class _CarveParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("near_dist", C.c_float), ("far_dist", C.c_float), ("margin", C.c_float)]


class _SpacePlanes(C.Structure):
    _fields_ = [("state", C.c_void_p), ("known_free", C.c_void_p), ("frontier", C.c_void_p), ("cells", C.c_void_p), ("cells_cap", C.c_int32)]


class _ComponentPlanes(C.Structure):
    _fields_ = [("label", C.c_void_p), ("table", C.c_void_p), ("table_cap", C.c_int32)]


# dsm_component (include/dsm.h): 64 bytes
COMPONENT_DTYPE = np.dtype([("root", np.int32), ("count", np.int32), ("sum", np.int64, (3,)), ("lo", np.int32, (3,)), ("hi", np.int32, (3,)),
                            ("tag", np.int32), ("reserved", np.int32)])
assert COMPONENT_DTYPE.itemsize == 64
CONNECT_FACES, CONNECT_ALL = 6, 26

# dsm_view_score (include/dsm.h): 32 bytes, one per pose of dsm_grid_view
VIEW_SCORE_DTYPE = np.dtype([("in_view", np.int32), ("visible", np.int32), ("unknown", np.int32), ("free", np.int32), ("occupied", np.int32),
                             ("target", np.int32), ("reserved", np.int32, (2,))])
assert VIEW_SCORE_DTYPE.itemsize == 32
VIEW_MAX_REACH, VIEW_MAX_POSES, VIEW_UNKNOWN_BLOCKS = 4096, 4096, 1
VIEW_TARGET_NONE, VIEW_TARGET_FRONTIER = 0, 1
_VIEW_TARGETS = {None: VIEW_TARGET_NONE, "none": VIEW_TARGET_NONE, "frontier": VIEW_TARGET_FRONTIER}


class _ViewQuery(C.Structure):  # dsm_view_query of include/dsm_surfel_map.h
    _fields_ = [("struct_size", C.c_uint32), ("camera", _RenderCamera), ("flags", C.c_uint32), ("target", C.c_int32)]


def view_query(camera, target="frontier", flags=0) -> _ViewQuery:
    """a dsm_view_query: the view camera (anything render_camera takes), target "frontier" / "none" / None (or a VIEW_TARGET_* code,
    passed on for the library to judge), flags VIEW_UNKNOWN_BLOCKS or 0"""
    q = _ViewQuery()
    q.struct_size = C.sizeof(_ViewQuery)
    q.camera = render_camera(camera)
    q.flags = int(flags)
    q.target = _VIEW_TARGETS[target] if (target is None or isinstance(target, str)) else int(target)
    return q


def view_poses(poses) -> np.ndarray:
    """4x4 cam -> world matrices (row-major numpy, as everywhere here; one or many) as [n, 16] column-major floats"""
    return np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1, 16)


class _AlignParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_iterations", C.c_int32), ("stride", C.c_int32), ("dist_max", C.c_float),
                ("min_view_cos", C.c_float), ("huber", C.c_float), ("min_pixels", C.c_int32), ("stop_translation", C.c_float),
                ("stop_rotation", C.c_float)]


class _AlignResult(C.Structure):
    _fields_ = [("pose16", C.c_float * 16), ("T16", C.c_float * 16), ("status", C.c_int32), ("iterations", C.c_int32), ("n_pixels", C.c_int32),
                ("scale_log2", C.c_int32), ("rms", C.c_double), ("sums", C.c_int64 * ALIGN_SUMS)]


def align_params(params=None, **kw) -> _AlignParams:
    """a dsm_align_params: one passed through, or the library's defaults (dsm_align_params_init: 10 iterations, stride 2, dist_max
    0.25 m, min_view_cos 0.2, huber 0.05 m, min_pixels 200, stop at 1e-4 m and 1e-4 rad) with the fields named in kw replaced"""
    if isinstance(params, _AlignParams):
        return params
    p = _AlignParams()
    load_library().dsm_align_params_init(C.byref(p))
    for k, v in dict(params or {}, **kw).items():
        if k not in dict(_AlignParams._fields_):
            raise ValueError("no such align parameter: %s" % k)
        setattr(p, k, v)
    return p


def align_result(r: _AlignResult) -> dict:
    """a dsm_align_result as a dict: "pose" and "T" 4x4 float32 (row-major numpy), "status" (ALIGN_*), "iterations", "n_pixels",
    "rms", "scale_log2", "sums" int64 [29]"""
    return {"pose": np.array(r.pose16, np.float32).reshape(4, 4).T.copy(), "T": np.array(r.T16, np.float32).reshape(4, 4).T.copy(),
            "status": r.status, "iterations": r.iterations, "n_pixels": r.n_pixels, "rms": r.rms, "scale_log2": r.scale_log2,
            "sums": np.array(r.sums, np.int64)}


def carve_params(params=None, **kw) -> _CarveParams:
    """a dsm_carve_params: one passed through, or the library's defaults (dsm_carve_params_init: near_dist 0.1 m, far_dist 10 m, margin
    0.1732051 m = one voxel diagonal of a 0.1 m grid) with the fields named in kw replaced"""
    if isinstance(params, _CarveParams):
        return params
    p = _CarveParams()
    load_library().dsm_carve_params_init(C.byref(p))
    for k, v in dict(params or {}, **kw).items():
        if k not in dict(_CarveParams._fields_):
            raise ValueError("no such carve parameter: %s" % k)
        setattr(p, k, v)
    return p


def space_outputs(spec, planes, dst_ptrs, cells_cap):
    """(the dsm_space_planes struct, the numpy arrays behind it or None for device pointers)"""
    unknown = set(planes) - set(SPACE_PLANES) if dst_ptrs is None else set(dst_ptrs) - set(SPACE_PLANES)
    if unknown:
        raise ValueError("no such space plane: %s" % sorted(unknown))
    st = _SpacePlanes()
    st.cells_cap = 0 if cells_cap is None else int(cells_cap)
    if dst_ptrs is not None:
        for k, p in dst_ptrs.items():
            setattr(st, k, p)
        return st, None
    wx, words, voxels = grid_shapes(spec)
    out = {}
    for k in SPACE_PLANES:
        if k in planes:
            out[k] = np.zeros(max(st.cells_cap, 1), np.int32) if k == "cells" else np.zeros(voxels, np.uint8) if k == "state" else np.zeros(words, np.uint32)
            setattr(st, k, out[k].ctypes.data)
    return st, out


def grid_spec(origin=(0.0, 0.0, 0.0), voxel=0.1, dims=(1, 1, 1), inflate=0) -> _GridSpec:
    """a dsm_grid_spec: the low corner of voxel (0, 0, 0), the edge in metres, (nx, ny, nz), the inflation radius in voxels.
    Nothing is checked here: the library does."""
    g = _GridSpec()
    load_library().dsm_grid_spec_init(C.byref(g))
    g.origin[:] = [float(v) for v in origin]
    g.voxel = float(voxel)
    g.nx, g.ny, g.nz = (int(v) for v in dims)
    g.inflate = int(inflate)
    return g


def grid_spec_around(centre, voxel=0.1, dims=(64, 64, 32), inflate=0) -> _GridSpec:
    """dsm_grid_spec_around: a grid of `dims` voxels around `centre` on the lattice of multiples of `voxel`, so that grids taken
    around successive poses share one lattice"""
    g = grid_spec(voxel=voxel, dims=dims, inflate=inflate)
    c = (C.c_float * 3)(*(float(v) for v in centre))
    load_library().dsm_grid_spec_around(C.byref(g), c, float(voxel), *(int(v) for v in dims))
    return g


def grid_shapes(spec):
    """(words per row, the shape of a bit set, the shape of the index plane) of a dsm_grid_spec"""
    wx = (spec.nx + 31) // 32
    return wx, (spec.nz, spec.ny, wx), (spec.nz, spec.ny, spec.nx)


def grid_unpack(bits, nx) -> np.ndarray:
    """a bit set [nz, ny, wx] uint32 as a bool array [nz, ny, nx]"""
    b = np.ascontiguousarray(bits, np.uint32)
    x = np.arange(nx)
    return ((b[..., x >> 5] >> (x & 31).astype(np.uint32)) & 1).astype(bool)


def grid_cell_centres(spec, cells) -> np.ndarray:
    """the voxel centres (n, 3) float32 of the linear indices `cells`: the voxel-down-sampled cloud, with the definition's arithmetic"""
    c = np.asarray(cells, np.int64)
    ijk = np.stack([c % spec.nx, c // spec.nx % spec.ny, c // (spec.nx * spec.ny)], 1)
    o, v = np.array(spec.origin[:], np.float32), np.float32(spec.voxel)
    return (o[None, :] + (ijk.astype(np.float32) + np.float32(0.5)) * v).astype(np.float32)


def grid_outputs(spec, planes, dst_ptrs, cells_cap):
    """(the dsm_grid_planes struct, the numpy arrays behind it or None for device pointers)"""
    unknown = set(planes) - set(GRID_PLANES) if dst_ptrs is None else set(dst_ptrs) - set(GRID_PLANES)
    if unknown:
        raise ValueError("no such grid plane: %s" % sorted(unknown))
    st = _GridPlanes()
    st.cells_cap = 0 if cells_cap is None else int(cells_cap)
    if dst_ptrs is not None:
        for k, p in dst_ptrs.items():
            setattr(st, k, p)
        return st, None
    # (a size the library will refuse still gets arrays to point at: the refusal is the library's to make)
    nx, ny, nz = (min(max(int(v), 1), 1 << 10) for v in (spec.nx, spec.ny, spec.nz))
    ok = 1 <= spec.nx and 1 <= spec.ny and 1 <= spec.nz and spec.nx * spec.ny * spec.nz <= GRID_MAX_VOXELS
    if ok:
        nx, ny, nz = spec.nx, spec.ny, spec.nz
    out = {}
    for k in GRID_PLANES:
        if k in planes:
            if k == "cells":
                out[k] = np.zeros(max(st.cells_cap, 1), np.int32)
            else:
                out[k] = np.zeros((nz, ny, nx) if k == "index" else (nz, ny, (nx + 31) // 32), np.int32 if k == "index" else np.uint32)
            setattr(st, k, out[k].ctypes.data)
    return st, out


def field_distance_table(voxel, max_dist) -> np.ndarray:
    """the metres of the `distance` plane by squared distance in voxels, float32 [max_dist^2 + 1], as the library builds it on the
    host: table[k] = (float)((double)(float)voxel * sqrt((double)k)); a voxel with no set voxel within max_dist holds table[-1]"""
    k = np.arange(int(max_dist) ** 2 + 1, dtype=np.float64)
    return (np.float64(np.float32(voxel)) * np.sqrt(k)).astype(np.float32)


def field_outputs(spec, planes, dst_ptrs):
    """(the dsm_field_planes struct, the numpy arrays behind it or None for device pointers)"""
    unknown = set(planes) - set(FIELD_PLANES) if dst_ptrs is None else set(dst_ptrs) - set(FIELD_PLANES)
    if unknown:
        raise ValueError("no such field plane: %s" % sorted(unknown))
    st = _FieldPlanes()
    if dst_ptrs is not None:
        for k, p in dst_ptrs.items():
            setattr(st, k, p)
        return st, None
    # (a size the library will refuse still gets arrays to point at: the refusal is the library's to make)
    ok = 1 <= spec.nx and 1 <= spec.ny and 1 <= spec.nz and spec.nx * spec.ny * spec.nz <= FIELD_MAX_VOXELS
    shape = (spec.nz, spec.ny, spec.nx) if ok else (1, 1, 1)
    out = {k: np.zeros(shape, FIELD_PLANE_TYPES[k]) for k in FIELD_PLANES if k in planes}
    for k, a in out.items():
        setattr(st, k, a.ctypes.data)
    return st, out


def render_camera(cam) -> _RenderCamera:
    """a dsm_render_camera from one (passed through), from (width, height, fx, fy, cx, cy, near_dist, far_dist), or from an object
    with those attributes (near / far also do: synth's cameras)"""
    if isinstance(cam, _RenderCamera):
        return cam
    if isinstance(cam, C.Structure):  # the same fields declared elsewhere
        return _RenderCamera(*(getattr(cam, f[0]) for f in _RenderCamera._fields_))
    if isinstance(cam, (tuple, list)):
        return _RenderCamera(*cam)
    near = cam.near_dist if hasattr(cam, "near_dist") else cam.near
    far = cam.far_dist if hasattr(cam, "far_dist") else cam.far
    return _RenderCamera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, near, far)


def render_outputs(cam, planes, dst_ptrs):
    """(the dsm_render_planes struct, the numpy arrays behind it or None for device pointers)"""
    unknown = set(planes) - set(RENDER_PLANES) if dst_ptrs is None else set(dst_ptrs) - set(RENDER_PLANES)
    if unknown:
        raise ValueError("no such render plane: %s" % sorted(unknown))
    st = _RenderPlanes()
    if dst_ptrs is not None:
        for k, p in dst_ptrs.items():
            setattr(st, k, p)
        return st, None
    out = {}
    for k in RENDER_PLANES:
        if k in planes:
            dt, tail = RENDER_PLANE_TYPES[k]
            # (a size the library will refuse still gets an array to point at: the refusal is the library's to make)
            out[k] = np.zeros((min(max(cam.height, 0), 8192), min(max(cam.width, 0), 8192)) + tail, dt)
            setattr(st, k, out[k].ctypes.data)
    return st, out


class _StageTimes(C.Structure):
    _fields_ = [("n_stages", C.c_int32), ("name", C.c_char_p * DSM_MAX_STAGES),
                ("ms", C.c_double * DSM_MAX_STAGES), ("launches", C.c_int64 * DSM_MAX_STAGES),
                ("frames", C.c_int64), ("event_overhead_ms", C.c_double), ("sum_new", C.c_int64), ("sum_local", C.c_int64)]


_vp = C.c_void_p
_lib = None


def load_library():
    """dlopen the in-tree HIP library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m densesurfelmapping_amd.build` "
            "(hipcc, gfx950). This package has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    lib.dsm_last_error.restype = C.c_char_p
    lib.dsm_last_error.argtypes = [_vp]
    lib.dsm_config_init.argtypes = [C.POINTER(_Config), C.c_int, C.c_int] + [C.c_float] * 6 + [C.c_int]
    lib.dsm_create.argtypes = [C.POINTER(_Config), C.POINTER(_vp)]
    lib.dsm_destroy.argtypes = [_vp]
    lib.dsm_destroy.restype = None
    lib.dsm_host_alloc.argtypes = [C.POINTER(_vp), C.c_size_t]
    lib.dsm_host_free.argtypes = [_vp]
    lib.dsm_host_free.restype = None
    lib.dsm_host_pack_frames.argtypes = [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t]
    lib.dsm_fuse_initialize_map.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, C.c_int32,
                                            _vp, C.c_int32, _vp]
    lib.dsm_fuse_map.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, C.c_int32, _vp]
    lib.dsm_fuse_initialize_map_inv.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, C.c_int32,
                                                _vp, C.c_int32, _vp]
    lib.dsm_fuse_map_inv.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _vp, _vp, _vp, _vp, C.c_int32, _vp]
    lib.dsm_fuse_frame_resident_inv.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp]
    lib.dsm_replay_enqueue_inv.argtypes = [_vp, C.c_int32, _vp, _vp, _vp, _vp]
    lib.dsm_replay_enqueue_host.argtypes = [_vp, C.c_int32, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp]
    lib.dsm_replay_wait.argtypes = [_vp, C.c_int32]
    lib.dsm_batch_replay_enqueue_inv.argtypes = [_vp, C.c_int32, _vp, _vp, _vp, _vp]
    lib.dsm_map_upload.argtypes = [_vp, _vp, C.c_int32]
    lib.dsm_map_size.argtypes = [_vp, _vp]
    lib.dsm_map_capacity.argtypes = [_vp, _vp]
    lib.dsm_map_download.argtypes = [_vp, _vp, C.c_int32, _vp]
    lib.dsm_map_copy_to_device.argtypes = [_vp, _vp, C.c_int32, _vp]
    lib.dsm_map_warp.argtypes = [_vp, _vp]
    lib.dsm_warp_grouped_device.argtypes = [_vp, _vp, C.c_int32, _vp, _vp]
    lib.dsm_map_extract.argtypes = [_vp, C.c_int32, _vp, C.c_int32, _vp]
    lib.dsm_map_append.argtypes = [_vp, _vp, C.c_int32]
    lib.dsm_store_deactivate.argtypes = [_vp, C.c_int32, _vp, _vp]
    lib.dsm_store_activate.argtypes = [_vp, C.c_int32, C.c_int32]
    lib.dsm_store_erase.argtypes = [_vp, C.c_int32, C.c_int32]
    lib.dsm_store_warp.argtypes = [_vp, C.c_int32, _vp, _vp, _vp]
    lib.dsm_store_size.argtypes = [_vp, _vp]
    lib.dsm_store_download.argtypes = [_vp, C.c_int32, C.c_int32, _vp, _vp]
    lib.dsm_cloud_compose.argtypes = [_vp, C.c_int, C.c_int32, _vp, _vp, _vp, C.c_int, C.c_int32, _vp]
    lib.dsm_frame_cloud.argtypes = [_vp, C.c_int, _vp, _vp, C.c_int, C.c_int32, _vp]
    lib.dsm_mesh_compose.argtypes = [_vp, C.c_int, C.c_int32, _vp, _vp, C.c_int, _vp, C.c_int, C.c_int32, _vp]
    lib.dsm_mesh_indices.argtypes = [_vp, C.c_int32, _vp, C.c_int]
    lib.dsm_render_compose.argtypes = [_vp, C.c_int, C.c_int32, _vp, _vp, C.POINTER(_RenderCamera), _vp, _vp, C.c_uint32, C.POINTER(_RenderPlanes),
                                       C.c_int, _vp]
    lib.dsm_grid_spec_init.argtypes = [C.POINTER(_GridSpec)]
    lib.dsm_grid_spec_init.restype = None
    lib.dsm_grid_spec_around.argtypes = [C.POINTER(_GridSpec), _vp, C.c_float, C.c_int32, C.c_int32, C.c_int32]
    lib.dsm_grid_spec_around.restype = None
    lib.dsm_grid_compose.argtypes = [_vp, C.c_int, C.c_int32, _vp, _vp, C.POINTER(_GridSpec), C.c_uint32, C.POINTER(_GridPlanes), C.c_int, _vp, _vp]
    lib.dsm_grid_inflate.argtypes = [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp]
    lib.dsm_grid_distance.argtypes = [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_float, _vp, C.POINTER(_FieldPlanes)]
    lib.dsm_field_compose.argtypes = [_vp, C.c_int, C.c_int32, _vp, _vp, C.POINTER(_GridSpec), C.c_int32, C.c_uint32, C.POINTER(_FieldPlanes), C.c_int, _vp]
    lib.dsm_carve_params_init.argtypes = [C.POINTER(_CarveParams)]
    lib.dsm_carve_params_init.restype = None
    lib.dsm_grid_carve.argtypes = [_vp, C.POINTER(_GridSpec), C.POINTER(_CarveParams), C.c_uint32, C.c_int32, _vp, _vp, _vp, _vp, _vp]
    lib.dsm_grid_classify.argtypes = [_vp, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.POINTER(_SpacePlanes), _vp]
    lib.dsm_grid_components.argtypes = [_vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.POINTER(_ComponentPlanes), _vp, _vp]
    lib.dsm_grid_view.argtypes = [_vp, C.POINTER(_GridSpec), C.POINTER(_RenderCamera), C.c_uint32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_int, _vp]
    lib.dsm_align_params_init.argtypes = [C.POINTER(_AlignParams)]
    lib.dsm_align_params_init.restype = None
    lib.dsm_align_equations.argtypes = [_vp, C.c_int, C.POINTER(_RenderCamera), _vp, _vp, _vp, C.POINTER(_AlignParams), _vp, _vp]
    lib.dsm_align_frame.argtypes = [_vp, C.c_int, C.c_int, C.c_int32, _vp, _vp, C.POINTER(_RenderCamera), _vp, C.POINTER(_AlignParams),
                                    C.POINTER(_AlignResult)]
    lib.dsm_frame_upload.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t]
    lib.dsm_frame_upload_device.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t]
    lib.dsm_frame_pitch.argtypes = [_vp, _vp]
    lib.dsm_frame_upload_async.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t]
    lib.dsm_frames_upload_async.argtypes = [_vp, C.c_int, C.c_int, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t]
    lib.dsm_frame_uploads_wait.argtypes = [_vp]
    lib.dsm_fuse_frame_resident.argtypes = [_vp, C.c_int, C.c_int, _vp]
    lib.dsm_replay_enqueue.argtypes = [_vp, C.c_int32, _vp, _vp, _vp]
    lib.dsm_synchronize.argtypes = [_vp]
    lib.dsm_last_new_count.argtypes = [_vp, _vp]
    lib.dsm_stream.argtypes = [_vp, C.POINTER(_vp)]
    lib.dsm_get_labels.argtypes = [_vp, _vp]
    lib.dsm_get_seeds.argtypes = [_vp, _vp]
    lib.dsm_seed_count.argtypes = [_vp]
    lib.dsm_debug_wave_stamps.argtypes = [_vp, _vp]
    lib.dsm_debug_set_fit_small_cap.argtypes = [_vp, C.c_int32]
    lib.dsm_debug_tier_counts.argtypes = [_vp, _vp]
    lib.dsm_debug_dropin_stats.argtypes = [_vp, _vp]
    lib.dsm_debug_run_stages.argtypes = [_vp, C.c_int, C.c_int, _vp, C.c_int, C.c_int]
    lib.dsm_debug_get_label_buffer.argtypes = [_vp, C.c_int, _vp]
    lib.dsm_debug_set_label_buffer.argtypes = [_vp, C.c_int, _vp]
    lib.dsm_debug_get_seed_state.argtypes = [_vp, _vp, _vp]
    lib.dsm_debug_set_seed_state.argtypes = [_vp, _vp, _vp]
    lib.dsm_replay_timed.argtypes = [_vp, C.c_int32, _vp, _vp, _vp, C.POINTER(_StageTimes)]
    lib.dsm_batch_create.argtypes = [C.POINTER(_vp), C.c_int32, C.POINTER(_vp)]
    lib.dsm_batch_destroy.argtypes = [_vp]
    lib.dsm_batch_destroy.restype = None
    lib.dsm_batch_last_error.argtypes = [_vp]
    lib.dsm_batch_last_error.restype = C.c_char_p
    lib.dsm_batch_replay_enqueue.argtypes = [_vp, C.c_int32, _vp, _vp, _vp]
    lib.dsm_batch_synchronize.argtypes = [_vp]
    lib.dsm_batch_replay_timed.argtypes = [_vp, C.c_int32, _vp, _vp, _vp, C.POINTER(_StageTimes)]
    lib.dsm_frame_upload_u16.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, C.c_float, C.c_int32]
    lib.dsm_frame_upload_device_u16.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, C.c_float, C.c_int32]
    lib.dsm_frame_upload_async_u16.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, C.c_float, C.c_int32]
    lib.dsm_frames_upload_async_u16.argtypes = [_vp, C.c_int, C.c_int, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_float, C.c_int32]
    lib.dsm_replay_enqueue_host_u16.argtypes = [_vp, C.c_int32, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp,
                                                C.c_float, C.c_int32]
    lib.dsm_host_pack_frames_u16.argtypes = [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t]
    lib.dsm_debug_get_frame.argtypes = [_vp, C.c_int, _vp, _vp]
    lib.dsm_debug_frame_planes.argtypes = [_vp, C.c_int, C.c_int, _vp, _vp]
    _ff = C.POINTER(_FrameFormat)
    lib.dsm_frame_format_init.argtypes = [_ff]
    lib.dsm_frame_format_init.restype = None
    lib.dsm_frame_upload_fmt.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _ff]
    lib.dsm_frame_upload_device_fmt.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _ff]
    lib.dsm_frame_upload_async_fmt.argtypes = [_vp, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, _ff]
    lib.dsm_frames_upload_async_fmt.argtypes = [_vp, C.c_int, C.c_int, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _ff]
    lib.dsm_replay_enqueue_host_fmt.argtypes = [_vp, C.c_int32, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t, _vp, _vp, _vp, _ff]
    lib.dsm_host_pack_frames_fmt.argtypes = [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t,
                                             C.c_size_t, _ff]
    _lib = lib
    return lib


def _ptr(a):
    return a.ctypes.data_as(_vp)


def _inv_ptr(inv_pose):
    """the caller's own world->cam matrix (4x4 row-major numpy, or 16 column-major floats) as a pointer, or NULL"""
    if inv_pose is None:
        return None, None
    a = np.asarray(inv_pose, np.float32)
    a = pose_to_colmajor(a) if a.shape == (4, 4) else np.ascontiguousarray(a.reshape(16))
    return a, _ptr(a)


def pose_to_colmajor(pose) -> np.ndarray:
    """4x4 cam->world matrix (row-major numpy) -> the 16 floats of an Eigen::Matrix4f."""
    p = np.asarray(pose, np.float32)
    if p.shape != (4, 4):
        raise ValueError("pose must be 4x4")
    return np.ascontiguousarray(p.T).ravel()


class FusionFunctions:
    """Drop-in for the reference's ``FusionFunctions`` (one instance = one handle = one stream)."""

    def __init__(self):
        self._lib = load_library()
        self._h = None

    # fusion_functions.h:84-87; the keyword arguments are what an HBM-resident engine adds
    def initialize(self, width, height, fx, fy, cx, cy, far_dist, near_dist, *, rgbd=False, device=0,
                   surfel_capacity=0, frame_slots=0, flags=0, pipeline_depth=0, constants=None):
        """constants: (huber_range, baseline, disparity_error, min_tolerate_diff) in place of the set `rgbd` selects
        (struct dsm_config, include/dsm.h); None keeps that set."""
        self.close()
        cfg = _Config()
        rc = self._lib.dsm_config_init(C.byref(cfg), width, height, fx, fy, cx, cy, far_dist, near_dist,
                                       1 if rgbd else 0)
        if rc:
            raise DsmError(rc, "dsm_config_init")
        cfg.device, cfg.surfel_capacity, cfg.frame_slots, cfg.flags = device, surfel_capacity, frame_slots, flags
        cfg.pipeline_depth = pipeline_depth
        if constants is not None:
            cfg.huber_range, cfg.baseline, cfg.disparity_error, cfg.min_tolerate_diff = (float(v) for v in constants)
        h = _vp()
        rc = self._lib.dsm_create(C.byref(cfg), C.byref(h))
        if rc:
            raise DsmError(rc, self._lib.dsm_last_error(None).decode())
        self._h = h
        self.width, self.height = width, height
        self.n_seed = self._lib.dsm_seed_count(h)
        return self

    @classmethod
    def from_camera(cls, cam, **kw):
        return cls().initialize(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cam.far, cam.near,
                                rgbd=getattr(cam, "rgbd", False), **kw)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.dsm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise DsmError(rc, self._lib.dsm_last_error(self._h).decode())

    def _frame_args(self, image, depth):
        image = np.asarray(image)
        depth = np.asarray(depth)
        if image.dtype != np.uint8 or depth.dtype != np.float32:
            raise TypeError("image must be uint8 (CV_8UC1) and depth float32 (CV_32FC1)")
        if image.shape != (self.height, self.width) or depth.shape != (self.height, self.width):
            raise ValueError("image/depth shape does not match initialize()")
        # the C side takes a pointer and a positive row step >= one row (a cv::Mat): anything else -- element stride
        # other than the item size, flipped (negative step) or broadcast (step smaller than a row) views -- is copied
        if image.strides[1] != 1 or image.strides[0] < self.width:
            image = np.ascontiguousarray(image)
        if depth.strides[1] != 4 or depth.strides[0] < self.width * 4:
            depth = np.ascontiguousarray(depth)
        return image, depth

    # fusion_functions.h:88-94: returns (local_surfels updated, new_surfels)
    # inv_pose: the caller's own pose.inverse() (FF.cpp:59), see dsm_fuse_map_inv in include/dsm.h; None = the library's closed form
    def fuse_initialize_map(self, reference_frame_index, image, depth, pose, local_surfels, inv_pose=None):
        image, depth = self._frame_args(image, depth)
        pose_cm = pose_to_colmajor(pose)
        _keep, inv = _inv_ptr(inv_pose)
        local = np.ascontiguousarray(local_surfels, SURFEL_DTYPE).copy()
        fresh = np.zeros(self.n_seed, SURFEL_DTYPE)
        n_new = C.c_int32(0)
        self._check(self._lib.dsm_fuse_initialize_map_inv(
            self._h, reference_frame_index, _ptr(image), image.strides[0], _ptr(depth), depth.strides[0],
            _ptr(pose_cm), inv, _ptr(local), len(local), _ptr(fresh), len(fresh), C.byref(n_new)))
        return local, fresh[: n_new.value].copy()

    # SurfelMap::fuse_map (surfel_map.cpp:1060-1113): returns (local_surfels after compaction, n_new)
    def fuse_map(self, reference_frame_index, image, depth, pose, local_surfels, inv_pose=None):
        image, depth = self._frame_args(image, depth)
        pose_cm = pose_to_colmajor(pose)
        _keep, inv = _inv_ptr(inv_pose)
        cap = len(local_surfels) + self.n_seed
        buf = np.zeros(cap, SURFEL_DTYPE)
        buf[: len(local_surfels)] = local_surfels
        n_local = C.c_int32(len(local_surfels))
        n_new = C.c_int32(0)
        self._check(self._lib.dsm_fuse_map_inv(
            self._h, reference_frame_index, _ptr(image), image.strides[0], _ptr(depth), depth.strides[0],
            _ptr(pose_cm), inv, _ptr(buf), C.byref(n_local), cap, C.byref(n_new)))
        return buf[: n_local.value].copy(), n_new.value

    def fuse_map_inplace(self, reference_frame_index, image, depth, pose, buf, n_local, inv_pose=None):
        """dsm_fuse_map on the caller's own array, as the C++ caller uses it (`buf` = std::vector storage with
        capacity len(buf), the first n_local records live): no copies on the Python side.  Returns (n_local, n_new)."""
        image, depth = self._frame_args(image, depth)
        pose_cm = pose_to_colmajor(pose)
        _keep, inv = _inv_ptr(inv_pose)
        assert buf.dtype == SURFEL_DTYPE and buf.flags.c_contiguous
        n = C.c_int32(n_local)
        n_new = C.c_int32(0)
        self._check(self._lib.dsm_fuse_map_inv(
            self._h, reference_frame_index, _ptr(image), image.strides[0], _ptr(depth), depth.strides[0],
            _ptr(pose_cm), inv, _ptr(buf), C.byref(n), len(buf), C.byref(n_new)))
        return n.value, n_new.value

    # ---- resident path -------------------------------------------------------------------
    def map_upload(self, surfels):
        a = np.ascontiguousarray(surfels, SURFEL_DTYPE)
        self._check(self._lib.dsm_map_upload(self._h, _ptr(a), len(a)))

    def map_size(self) -> int:
        n = C.c_int32(0)
        self._check(self._lib.dsm_map_size(self._h, C.byref(n)))
        return n.value

    def map_capacity(self) -> int:
        n = C.c_int32(0)
        self._check(self._lib.dsm_map_capacity(self._h, C.byref(n)))
        return n.value

    def map_download(self) -> np.ndarray:
        n = self.map_size()
        out = np.zeros(max(n, 1), SURFEL_DTYPE)
        m = C.c_int32(0)
        self._check(self._lib.dsm_map_download(self._h, _ptr(out), len(out), C.byref(m)))
        return out[: m.value].copy()

    def map_copy_to_device(self, dst_ptr: int, cap: int) -> int:
        n = C.c_int32(0)
        self._check(self._lib.dsm_map_copy_to_device(self._h, _vp(dst_ptr), cap, C.byref(n)))
        return n.value

    # ---- map maintenance between frames (surfel_map.cpp:681-824, 1456-1595) -----------------
    def map_warp(self, warp):
        """SurfelMap::warp_active_surfels_cpu_kernel: warp = (loop_pose * cam_pose^-1) as 4x4 float."""
        w = pose_to_colmajor(warp)
        self._check(self._lib.dsm_map_warp(self._h, _ptr(w)))

    def warp_grouped_device(self, surfels_ptr, offsets, mats):
        """SurfelMap::warp_inactive_surfels_cpu_kernel on device memory: mats [g,4,4], offsets [g+1]."""
        offsets = np.ascontiguousarray(offsets, np.int32)
        mats_cm = np.ascontiguousarray(np.asarray(mats, np.float32).transpose(0, 2, 1)).reshape(-1, 16)
        self._check(self._lib.dsm_warp_grouped_device(self._h, _vp(surfels_ptr), len(offsets) - 1, _ptr(offsets), _ptr(mats_cm)))

    def map_extract(self, key) -> np.ndarray:
        """move_add_surfels removal: live surfels with last_update == key, in order; their slots are deleted."""
        out = np.zeros(max(self.map_size(), 1), SURFEL_DTYPE)
        n = C.c_int32(0)
        self._check(self._lib.dsm_map_extract(self._h, key, _ptr(out), len(out), C.byref(n)))
        return out[: n.value].copy()

    def map_append(self, surfels):
        a = np.ascontiguousarray(surfels, SURFEL_DTYPE)
        self._check(self._lib.dsm_map_append(self._h, _ptr(a), len(a)))

    # ---- inactive store (device-side attached_surfels + inactive_pointcloud of surfel_map.cpp)
    def store_deactivate(self, key):
        """move_add_surfels removal into the device store; returns the segment (begin, n)."""
        b, n = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.dsm_store_deactivate(self._h, key, C.byref(b), C.byref(n)))
        return b.value, n.value

    def store_activate(self, begin, n):
        self._check(self._lib.dsm_store_activate(self._h, begin, n))

    def store_erase(self, begin, n):
        self._check(self._lib.dsm_store_erase(self._h, begin, n))

    def store_warp(self, offsets, mats, changed):
        """offsets [g+1] tile the store; mats [g,4,4] row-major numpy; changed [g] bool."""
        offsets = np.ascontiguousarray(offsets, np.int32)
        mats_cm = np.ascontiguousarray(np.asarray(mats, np.float32).transpose(0, 2, 1)).reshape(-1, 16)
        ch = np.ascontiguousarray(changed, np.uint8)
        self._check(self._lib.dsm_store_warp(self._h, len(offsets) - 1, _ptr(offsets), _ptr(mats_cm), _ptr(ch)))

    def store_size(self) -> int:
        n = C.c_int32(0)
        self._check(self._lib.dsm_store_size(self._h, C.byref(n)))
        return n.value

    def store_download(self, begin=0, n=None):
        """(surfels, xyzi) of store[begin, begin+n)."""
        if n is None:
            n = self.store_size() - begin
        s = np.zeros(max(n, 1), SURFEL_DTYPE)
        c = np.zeros((max(n, 1), 4), np.float32)
        self._check(self._lib.dsm_store_download(self._h, begin, n, _ptr(s), _ptr(c)))
        return s[:n].copy(), c[:n].copy()

    # ---- point-cloud publications (surfel_map.cpp:1115-1151, 1283-1454) ---------------------------
    def cloud_compose(self, select=CLOUD_SELECT_MATURE, segments=(), dst_ptr=None, cap=None):
        """dsm_cloud_compose: the map records that pass `select` (CLOUD_SELECT_*), then the store's XYZI runs `segments`
        [(begin, count), ...].  Returns an (n, 4) float32 array -- or, with dst_ptr (device memory of cap points), n."""
        seg = np.ascontiguousarray(np.asarray(segments, np.int32).reshape(-1, 2))
        b = np.ascontiguousarray(seg[:, 0]) if len(seg) else np.zeros(1, np.int32)
        c = np.ascontiguousarray(seg[:, 1]) if len(seg) else np.zeros(1, np.int32)
        n = C.c_int32(0)
        if dst_ptr is not None:
            self._check(self._lib.dsm_cloud_compose(self._h, select, len(seg), _ptr(b), _ptr(c), _vp(dst_ptr), 1, cap, C.byref(n)))
            return n.value
        if cap is None:  # size it from the bound: the map records plus the runs
            cap = self.map_size() + int(seg[:, 1].sum() if len(seg) else 0)
        out = np.zeros((max(cap, 1), 4), np.float32)
        self._check(self._lib.dsm_cloud_compose(self._h, select, len(seg), _ptr(b), _ptr(c), _ptr(out), 0, cap, C.byref(n)))
        return out[: n.value].copy()

    # ---- the hexagon mesh (surfel_map.cpp:1176-1280) -----------------------------------------------
    def mesh_compose(self, select=CLOUD_SELECT_MATURE, segments=(), layout=MESH_VERTEX_REF6, dst_ptr=None, cap=None):
        """dsm_mesh_compose: six hexagon vertices per surfel -- the store's record runs `segments` [(begin, count), ...] first,
        then the map records that pass `select` (save_mesh's order).  Returns an (n, 36) float32 array (MESH_VERTEX_REF6:
        6 x (x y z c c c)) or an (n, 24) one (MESH_VERTEX_XYZ_RGBA8: 6 x (x y z rgba), the fourth the bytes r g b 255) -- or,
        with dst_ptr (device memory of cap surfels), n."""
        seg = np.ascontiguousarray(np.asarray(segments, np.int32).reshape(-1, 2))
        b = np.ascontiguousarray(seg[:, 0]) if len(seg) else np.zeros(1, np.int32)
        c = np.ascontiguousarray(seg[:, 1]) if len(seg) else np.zeros(1, np.int32)
        n = C.c_int32(0)
        if dst_ptr is not None:
            self._check(self._lib.dsm_mesh_compose(self._h, select, len(seg), _ptr(b), _ptr(c), layout, _vp(dst_ptr), 1, cap, C.byref(n)))
            return n.value
        if cap is None:  # size it from the bound: the runs plus the map records
            cap = (self.map_size() if select != CLOUD_SELECT_NONE else 0) + int(seg[:, 1].sum() if len(seg) else 0)
        out = np.zeros((max(cap, 1), MESH_SURFEL_BYTES[layout] // 4), np.float32)
        self._check(self._lib.dsm_mesh_compose(self._h, select, len(seg), _ptr(b), _ptr(c), layout, _ptr(out), 0, cap, C.byref(n)))
        return out[: n.value].copy()

    # ---- the map as an image ------------------------------------------------------------------------
    def render(self, select, segs, camera, pose, pose_inv=None, flags=0, planes=RENDER_PLANES, dst_ptrs=None):
        """dsm_render_compose: what `camera` (render_camera's forms) at `pose` (4x4 cam -> world, or 16 column-major floats) sees
        of the surfel sequence of mesh_compose(select, segs): the nearest disc along every pixel's ray.  Returns a dict of
        [height, width] numpy arrays for the `planes` asked for -- "depth" float32 (0 = nothing hit), "index" int32 (-1),
        "normal" float32 [.., 3] (camera frame), "intensity" uint8 -- plus "n_surfels", the length of the sequence.  With
        dst_ptrs = {plane: device pointer} (e.g. torch data_ptr()) the planes named there are written on the device and
        n_surfels is returned.  pose_inv: the caller's own world -> cam matrix, as for the *_inv calls; flags: RENDER_CULL_BACKFACES."""
        seg = np.ascontiguousarray(np.asarray(segs, np.int32).reshape(-1, 2))
        b = np.ascontiguousarray(seg[:, 0]) if len(seg) else np.zeros(1, np.int32)
        c = np.ascontiguousarray(seg[:, 1]) if len(seg) else np.zeros(1, np.int32)
        cam = render_camera(camera)
        p = np.asarray(pose, np.float32)
        p = pose_to_colmajor(p) if p.shape == (4, 4) else np.ascontiguousarray(p.reshape(16))
        _keep, inv_p = _inv_ptr(pose_inv)
        st, out = render_outputs(cam, planes, dst_ptrs)
        n = C.c_int32(0)
        self._check(self._lib.dsm_render_compose(self._h, select, len(seg), _ptr(b), _ptr(c), C.byref(cam), _ptr(p), inv_p, flags, C.byref(st),
                                                 0 if dst_ptrs is None else 1, C.byref(n)))
        if dst_ptrs is not None:
            return n.value
        out["n_surfels"] = n.value
        return out

    # ---- the map as a voxel grid -------------------------------------------------------------------
    def grid(self, select, segs, spec, flags=0, planes=("occupied", "inflated", "cells"), dst_ptrs=None, cells_cap=None):
        """dsm_grid_compose: the surfel sequence of render(select, segs) as an occupancy grid `spec` (grid_spec / grid_spec_around).
        Returns a dict of the `planes` asked for -- "occupied" and "inflated" uint32 [nz, ny, wx] bit sets (bit x & 31 of word
        x >> 5; grid_unpack gives bools), "index" int32 [nz, ny, nx] (the lowest surfel number covering the voxel, -1), "cells"
        int32 [n_cells] (the linear indices of the set voxels, of `inflated` with GRID_CELLS_OF_INFLATED; grid_cell_centres gives
        points) -- plus "n_surfels" and "n_cells".  cells_cap None: the list is sized by a second call when the first reports
        more cells than fit.  With dst_ptrs = {plane: device pointer} the planes named there are written on the device (cells
        needs cells_cap) and (n_surfels, n_cells) is returned.  More cells than cells_cap: DsmError with code DSM_E_CAPACITY and
        .n_cells = the count needed."""
        seg = np.ascontiguousarray(np.asarray(segs, np.int32).reshape(-1, 2))
        b = np.ascontiguousarray(seg[:, 0]) if len(seg) else np.zeros(1, np.int32)
        c = np.ascontiguousarray(seg[:, 1]) if len(seg) else np.zeros(1, np.int32)
        n, nc = C.c_int32(0), C.c_int32(0)
        auto = dst_ptrs is None and cells_cap is None and "cells" in planes
        st, out = grid_outputs(spec, planes, dst_ptrs, 4096 if auto else cells_cap)
        rc = self._lib.dsm_grid_compose(self._h, select, len(seg), _ptr(b), _ptr(c), C.byref(spec), flags, C.byref(st), 0 if dst_ptrs is None else 1,
                                        C.byref(n), C.byref(nc))
        if rc == DSM_E_CAPACITY and auto:
            st, out = grid_outputs(spec, planes, None, nc.value)
            rc = self._lib.dsm_grid_compose(self._h, select, len(seg), _ptr(b), _ptr(c), C.byref(spec), flags, C.byref(st), 0, C.byref(n), C.byref(nc))
        if rc == DSM_E_CAPACITY:
            e = DsmError(rc, self._lib.dsm_last_error(self._h).decode())
            e.n_cells, e.n_surfels, e.planes = nc.value, n.value, out
            raise e
        self._check(rc)
        if dst_ptrs is not None:
            return n.value, nc.value
        if "cells" in out:
            out["cells"] = out["cells"][: nc.value]
        out["n_surfels"], out["n_cells"] = n.value, nc.value
        return out

    def grid_inflate(self, dims, radius, src_ptr, dst_ptr):
        """dsm_grid_inflate: the inflation alone on a bit set [nz, ny, wx] in device memory (pointers, e.g. torch data_ptr()):
        dst = src dilated by the voxels within `radius`; dims = (nx, ny, nz)"""
        self._check(self._lib.dsm_grid_inflate(self._h, int(dims[0]), int(dims[1]), int(dims[2]), int(radius), _vp(src_ptr), _vp(dst_ptr)))

    # ---- the distance field of the voxel grid ------------------------------------------------------
    def grid_distance(self, dims, max_dist, voxel, src_ptr, dst_ptrs):
        """dsm_grid_distance: the truncated Euclidean distance field of a bit set [nz, ny, wx] in device memory (pointers, e.g. torch
        data_ptr()) into the device planes dst_ptrs = {"dist2" uint16 / "nearest" int32 / "distance" float32: pointer}, [nz, ny, nx]
        each; dims = (nx, ny, nz), max_dist in voxels (1 .. FIELD_MAX_DIST), voxel the edge in metres"""
        st, _ = field_outputs(None, (), dict(dst_ptrs))
        self._check(self._lib.dsm_grid_distance(self._h, int(dims[0]), int(dims[1]), int(dims[2]), int(max_dist), float(voxel), _vp(src_ptr), C.byref(st)))

    def field(self, select, segs, spec, max_dist, planes=FIELD_PLANES, dst_ptrs=None, flags=0):
        """dsm_field_compose: the distance field, out to max_dist voxels, of the occupied set that grid(select, segs, spec) gives.
        Returns a dict of the `planes` asked for, [nz, ny, nx] each -- "dist2" uint16 (the squared distance in voxels to the nearest
        occupied voxel, FIELD_FAR where none lies within max_dist), "nearest" int32 (its linear index (z ny + y) nx + x, -1),
        "distance" float32 (metres: field_distance_table(spec.voxel, max_dist)[dist2], its last entry where none) -- plus
        "n_surfels".  With dst_ptrs = {plane: device pointer} the planes named there are written on the device and n_surfels is
        returned."""
        seg = np.ascontiguousarray(np.asarray(segs, np.int32).reshape(-1, 2))
        b = np.ascontiguousarray(seg[:, 0]) if len(seg) else np.zeros(1, np.int32)
        c = np.ascontiguousarray(seg[:, 1]) if len(seg) else np.zeros(1, np.int32)
        st, out = field_outputs(spec, planes, dst_ptrs)
        n = C.c_int32(0)
        self._check(self._lib.dsm_field_compose(self._h, select, len(seg), _ptr(b), _ptr(c), C.byref(spec), int(max_dist), flags, C.byref(st),
                                                0 if dst_ptrs is None else 1, C.byref(n)))
        if dst_ptrs is not None:
            return n.value
        out["n_surfels"] = n.value
        return out

    # ---- free space, the three states, the frontier ------------------------------------------------
    def grid_carve(self, spec, slots, poses, free_ptr, params=None, flags=0, poses_inv=None):
        """dsm_grid_carve: the voxels of the grid `spec` that the depth frames in the frame slots `slots` see through, OR-ed into the bit
        set [nz, ny, wx] at the device pointer free_ptr (CARVE_REPLACE: stored over it).  poses: one 4x4 cam -> world matrix per slot
        (row-major numpy, as everywhere here), poses_inv their inverses or None (the library's closed form); params a carve_params()
        or a dict of its fields.  Returns the population count of the set after the call."""
        sl = np.ascontiguousarray(np.asarray(slots, np.int32).reshape(-1))
        ps = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
        pi = None if poses_inv is None else np.ascontiguousarray(np.asarray(poses_inv, np.float32).reshape(-1, 4, 4).transpose(0, 2, 1))
        if len(ps) != len(sl) or (pi is not None and len(pi) != len(sl)):
            raise ValueError("one pose (and one inverse) per slot")
        p = carve_params(params)
        n = C.c_int64(0)
        self._check(self._lib.dsm_grid_carve(self._h, C.byref(spec), C.byref(p), int(flags), len(sl), _ptr(sl) if len(sl) else None, _ptr(ps) if len(sl) else None,
                                             None if pi is None else _ptr(pi), _vp(free_ptr), C.byref(n)))
        return n.value

    def grid_classify(self, dims, occupied_ptr, free_ptr, dst_ptrs, cells_cap=0):
        """dsm_grid_classify: the three states and the frontier of the bit sets [nz, ny, wx] at the device pointers occupied_ptr and
        free_ptr, into the device planes dst_ptrs = {"state" uint8 [nz, ny, nx] (SPACE_UNKNOWN / _FREE / _OCCUPIED) / "known_free" /
        "frontier" uint32 [nz, ny, wx] / "cells" int32 [cells_cap]: pointer}; dims = (nx, ny, nz).  Returns the number of frontier
        voxels.  More than cells_cap with a cells plane: DsmError with code DSM_E_CAPACITY and .n_frontier = the count needed."""
        st, _ = space_outputs(None, (), dict(dst_ptrs), cells_cap)
        n = C.c_int32(0)
        rc = self._lib.dsm_grid_classify(self._h, int(dims[0]), int(dims[1]), int(dims[2]), _vp(occupied_ptr), _vp(free_ptr), C.byref(st), C.byref(n))
        if rc == DSM_E_CAPACITY:
            e = DsmError(rc, self._lib.dsm_last_error(self._h).decode())
            e.n_frontier = n.value
            raise e
        self._check(rc)
        return n.value

    # ---- connected components of a bit set ------------------------------------------------------------
    def grid_components(self, dims, src_ptr, connectivity=26, min_count=1, tag_ptr=None, label_ptr=None, table_ptr=None, table_cap=0):
        """dsm_grid_components: the connected components (connectivity 6 or 26) of the bit set [nz, ny, wx] at the device pointer
        src_ptr; dims = (nx, ny, nz).  label_ptr: a device plane int32 [nz, ny, nx] (the lowest linear index of the voxel's component,
        -1 outside the set), table_ptr: COMPONENT_DTYPE [table_cap] in device memory for the components of at least min_count voxels,
        ascending by root; either may be None.  tag_ptr: an int32 [nz, ny, nx] device plane whose value at a component's root becomes
        its `tag`.  Returns (n_components, n_all).  More than table_cap: DsmError with code DSM_E_CAPACITY and .n_components = the count
        needed, .n_all."""
        st = _ComponentPlanes(_vp(label_ptr) if label_ptr else None, _vp(table_ptr) if table_ptr else None, int(table_cap))
        n, n_all = C.c_int32(0), C.c_int32(0)
        rc = self._lib.dsm_grid_components(self._h, int(dims[0]), int(dims[1]), int(dims[2]), int(connectivity), int(min_count), _vp(src_ptr),
                                           _vp(tag_ptr) if tag_ptr else None, C.byref(st), C.byref(n), C.byref(n_all))
        if rc == DSM_E_CAPACITY:
            e = DsmError(rc, self._lib.dsm_last_error(self._h).decode())
            e.n_components, e.n_all = n.value, n_all.value
            raise e
        self._check(rc)
        return n.value, n_all.value

    def grid_components_host(self, bits, nx, connectivity=26, min_count=1, tags=None, labels=True):
        """The convenience for host data: the bit set `bits` (uint32 [nz, ny, wx]) and the optional int32 tag plane go to the device
        through torch, the table is sized by a first call.  Returns (table as a COMPONENT_DTYPE array, n_all, labels int32 [nz, ny, nx]
        or None)."""
        import torch
        b = np.ascontiguousarray(bits, np.uint32)
        nz, ny, wx = b.shape
        if wx != (nx + 31) // 32:
            raise ValueError("bits is not [nz, ny, (nx + 31) // 32]")
        dims = (nx, ny, nz)
        d_src = torch.from_numpy(b.view(np.int32)).cuda()
        d_tag = None if tags is None else torch.from_numpy(np.ascontiguousarray(tags, np.int32).reshape(nz, ny, nx)).cuda()
        d_label = torch.empty((nz, ny, nx), dtype=torch.int32, device="cuda")
        tag_ptr = None if d_tag is None else d_tag.data_ptr()
        n, n_all = self.grid_components(dims, d_src.data_ptr(), connectivity, min_count, tag_ptr, label_ptr=d_label.data_ptr())
        table = np.zeros(n, COMPONENT_DTYPE)
        if n:
            d_table = torch.empty((n * 8,), dtype=torch.int64, device="cuda")
            self.grid_components(dims, d_src.data_ptr(), connectivity, min_count, tag_ptr, table_ptr=d_table.data_ptr(), table_cap=n)
            table = d_table.cpu().numpy().view(COMPONENT_DTYPE).copy()
        return table, n_all, (d_label.cpu().numpy() if labels else None)

    # ---- viewpoint gain ---------------------------------------------------------------------------------
    def grid_view(self, spec, camera, poses, occupied_ptr, free_ptr, target_ptr=None, flags=0, poses_inv=None, visible_ptr=None, scores_ptr=None,
                  scores=True):
        """dsm_grid_view: what a camera (anything render_camera takes) at each of `poses` (4x4 cam -> world, row-major numpy; poses_inv
        their inverses or None = the library's closed form) would see of the grid `spec`, given the bit sets [nz, ny, wx] at the device
        pointers occupied_ptr and free_ptr and optionally target_ptr.  flags: VIEW_UNKNOWN_BLOCKS or 0.  visible_ptr: a device plane
        uint32 [n_poses, nz, ny, wx] for the visible set of every pose, or None.  Returns the scores as a VIEW_SCORE_DTYPE array
        [n_poses]; with scores_ptr (device memory, 32 bytes a pose) they are written there and None is returned; scores=False asks
        for the planes alone."""
        cam = render_camera(camera)
        ps = view_poses(poses)
        pi = None if poses_inv is None else view_poses(poses_inv)
        if pi is not None and len(pi) != len(ps):
            raise ValueError("one inverse per pose")
        out = np.zeros(len(ps), VIEW_SCORE_DTYPE) if (scores and not scores_ptr) else None
        dst = _vp(scores_ptr) if scores_ptr else (_ptr(out) if out is not None and len(out) else None)
        self._check(self._lib.dsm_grid_view(self._h, C.byref(spec), C.byref(cam), int(flags), len(ps), _ptr(ps) if len(ps) else None,
                                            None if pi is None else _ptr(pi), _vp(occupied_ptr) if occupied_ptr else None, _vp(free_ptr) if free_ptr else None,
                                            _vp(target_ptr) if target_ptr else None, dst, 1 if scores_ptr else 0, _vp(visible_ptr) if visible_ptr else None))
        return out

    # ---- a depth frame against the rendered map -----------------------------------------------------
    def align_equations(self, slot, model_cam, model_depth_ptr, model_normal_ptr, T, params=None):
        """dsm_align_equations: one evaluation of the frame in `slot` against the model planes in DEVICE memory (pointers, e.g.
        torch data_ptr(): depth [h, w] float32, normal [h, w, 3] float32 as render() writes them for `model_cam`), T the 4x4
        frame camera -> model camera transform (or 16 column-major floats).  Returns (sums int64 [29], scale_log2)."""
        cam = render_camera(model_cam)
        t = np.asarray(T, np.float32)
        t = pose_to_colmajor(t) if t.shape == (4, 4) else np.ascontiguousarray(t.reshape(16))
        p = align_params(params)
        sums = np.zeros(ALIGN_SUMS, np.int64)
        k = C.c_int32(0)
        self._check(self._lib.dsm_align_equations(self._h, slot, C.byref(cam), _vp(model_depth_ptr), _vp(model_normal_ptr), _ptr(t), C.byref(p),
                                                  _ptr(sums), C.byref(k)))
        return sums, k.value

    def align_frame(self, slot, select, segs, pose_guess, model_cam=None, params=None):
        """dsm_align_frame: the frame in `slot` aligned, point to plane, against the surfel sequence of render(select, segs) seen by
        `model_cam` (None: the handle's camera and fuse distances) at `pose_guess`.  Returns align_result's dict."""
        seg = np.ascontiguousarray(np.asarray(segs, np.int32).reshape(-1, 2))
        b = np.ascontiguousarray(seg[:, 0]) if len(seg) else np.zeros(1, np.int32)
        c = np.ascontiguousarray(seg[:, 1]) if len(seg) else np.zeros(1, np.int32)
        cam = None if model_cam is None else render_camera(model_cam)
        g = np.asarray(pose_guess, np.float32)
        g = pose_to_colmajor(g) if g.shape == (4, 4) else np.ascontiguousarray(g.reshape(16))
        p = align_params(params)
        r = _AlignResult()
        self._check(self._lib.dsm_align_frame(self._h, slot, select, len(seg), _ptr(b), _ptr(c), None if cam is None else C.byref(cam), _ptr(g),
                                              C.byref(p), C.byref(r)))
        return align_result(r)

    def mesh_indices(self, n_surfels, dst_ptr=None):
        """dsm_mesh_indices: the (n_surfels * 4, 3) uint32 triangles of n_surfels hexagons -- or, with dst_ptr, into device memory."""
        if dst_ptr is not None:
            self._check(self._lib.dsm_mesh_indices(self._h, n_surfels, _vp(dst_ptr), 1))
            return n_surfels
        out = np.zeros((max(n_surfels, 1) * 4, 3), np.uint32)
        self._check(self._lib.dsm_mesh_indices(self._h, n_surfels, _ptr(out), 0))
        return out[: n_surfels * 4].copy()

    def frame_cloud(self, slot, pose7, dst_ptr=None, cap=None):
        """dsm_frame_cloud: publish_raw_pointcloud of the frame in `slot`; pose7 = px py pz qx qy qz qw (geometry_msgs/Pose).
        Returns a (width * height, 4) float32 array in column-major pixel order -- or, with dst_ptr, n."""
        p = np.ascontiguousarray(pose7, np.float64).reshape(7)
        n = C.c_int32(0)
        if dst_ptr is not None:
            self._check(self._lib.dsm_frame_cloud(self._h, slot, _ptr(p), _vp(dst_ptr), 1, cap, C.byref(n)))
            return n.value
        cap = self.width * self.height if cap is None else cap
        out = np.zeros((max(cap, 1), 4), np.float32)
        self._check(self._lib.dsm_frame_cloud(self._h, slot, _ptr(p), _ptr(out), 0, cap, C.byref(n)))
        return out[: n.value].copy()

    def frame_upload(self, slot, image, depth):
        image, depth = self._frame_args(image, depth)
        self._check(self._lib.dsm_frame_upload(self._h, slot, _ptr(image), image.strides[0], _ptr(depth),
                                               depth.strides[0]))

    def frame_pitch(self) -> int:
        n = C.c_int32(0)
        self._check(self._lib.dsm_frame_pitch(self._h, C.byref(n)))
        return n.value

    def frame_upload_async(self, slot, image, depth):
        """dsm_frame_upload_async: `image` / `depth` are views of PAGE-LOCKED memory (PinnedFrames below) that stay
        untouched until frame_uploads_wait(); rows with the slot pitch go up as one transfer per plane."""
        if image.dtype != np.uint8 or depth.dtype != np.float32 or image.shape != (self.height, self.width) or depth.shape != image.shape:
            raise TypeError("image must be uint8 [H,W], depth float32 [H,W]")
        if image.strides[1] != 1 or depth.strides[1] != 4:
            raise ValueError("rows must be contiguous")
        self._check(self._lib.dsm_frame_upload_async(self._h, slot, _ptr(image), image.strides[0], _ptr(depth), depth.strides[0]))

    def frames_upload_async(self, slot0, pinned, first, n):
        """frames first .. first+n-1 of a PinnedFrames block (slot layout, back to back) into slots slot0 .. slot0+n-1:
        one transfer per plane for all of them -- of a block with tight rows too (PinnedFrames(..., tight=True))"""
        assert 0 <= first and first + n <= pinned.n and (pinned.h, pinned.w) == (self.height, self.width) and pinned.pitch in (self.frame_pitch(), self.width)
        img, dep = pinned.image(first), pinned.depth(first)
        if pinned.fmt is not None:  # colour images (with float or uint16 depth): PinnedFrames(..., image_format=...)
            self._check(self._lib.dsm_frames_upload_async_fmt(self._h, slot0, n, _ptr(img), img.strides[0], pinned._bytes_img,
                                                              _ptr(dep), dep.strides[0], pinned._bytes_dep, C.byref(pinned.fmt)))
            return
        if pinned.depth_u16 is not None:  # uint16 depth: converted on the device (PinnedFrames(..., depth_u16=(scale, op)))
            self._check(self._lib.dsm_frames_upload_async_u16(self._h, slot0, n, _ptr(img), img.strides[0], pinned.pitch * pinned.h,
                                                              _ptr(dep), dep.strides[0], pinned.pitch * pinned.h * 2, *pinned.depth_u16_args))
            return
        self._check(self._lib.dsm_frames_upload_async(self._h, slot0, n, _ptr(img), img.strides[0], pinned.pitch * pinned.h,
                                                      _ptr(dep), dep.strides[0], pinned.pitch * pinned.h * 4))

    def _frame_args_u16(self, image, depth):
        image = np.asarray(image)
        depth = np.asarray(depth)
        if image.dtype != np.uint8 or depth.dtype != np.uint16:
            raise TypeError("image must be uint8 (CV_8UC1) and depth uint16 (CV_16UC1)")
        if image.shape != (self.height, self.width) or depth.shape != (self.height, self.width):
            raise ValueError("image/depth shape does not match initialize()")
        if image.strides[1] != 1 or image.strides[0] < self.width:
            image = np.ascontiguousarray(image)
        if depth.strides[1] != 2 or depth.strides[0] < self.width * 2:
            depth = np.ascontiguousarray(depth)
        return image, depth

    def frame_upload_u16(self, slot, image, depth, scale, op="divide"):
        """dsm_frame_upload_u16: uint16 depth converted to metres on the device (depth_from_u16(depth, scale, op) bit for bit)"""
        image, depth = self._frame_args_u16(image, depth)
        self._check(self._lib.dsm_frame_upload_u16(self._h, slot, _ptr(image), image.strides[0], _ptr(depth), depth.strides[0],
                                                   scale, depth_op_code(op)))

    def frame_upload_device_u16(self, slot, image_ptr, img_step, depth_ptr, depth_step, scale, op="divide"):
        self._check(self._lib.dsm_frame_upload_device_u16(self._h, slot, _vp(image_ptr), img_step, _vp(depth_ptr), depth_step,
                                                          scale, depth_op_code(op)))

    def frame_upload_async_u16(self, slot, image, depth, scale, op="divide"):
        """dsm_frame_upload_async_u16: views of PAGE-LOCKED memory (PinnedFrames(..., depth_u16=...)), untouched until
        frame_uploads_wait()"""
        if image.dtype != np.uint8 or depth.dtype != np.uint16 or image.shape != (self.height, self.width) or depth.shape != image.shape:
            raise TypeError("image must be uint8 [H,W], depth uint16 [H,W]")
        if image.strides[1] != 1 or depth.strides[1] != 2:
            raise ValueError("rows must be contiguous")
        self._check(self._lib.dsm_frame_upload_async_u16(self._h, slot, _ptr(image), image.strides[0], _ptr(depth), depth.strides[0],
                                                         scale, depth_op_code(op)))

    def _frame_args_fmt(self, image, depth, fmt):
        image = np.asarray(image)
        depth = np.asarray(depth)
        ch = IMAGE_CHANNELS.get(fmt.image_format, 1)
        ddt = np.dtype(np.uint16 if fmt.depth_format == DEPTH_U16 else np.float32)
        if image.dtype != np.uint8 or depth.dtype != ddt:
            raise TypeError("image must be uint8 and depth %s" % ddt)
        if image.shape != ((self.height, self.width) if ch == 1 else (self.height, self.width, ch)) or depth.shape != (self.height, self.width):
            raise ValueError("image/depth shape does not match initialize() and the format")
        if image.strides[1] != ch or (ch > 1 and image.strides[2] != 1) or image.strides[0] < self.width * ch:
            image = np.ascontiguousarray(image)
        if depth.strides[1] != ddt.itemsize or depth.strides[0] < self.width * ddt.itemsize:
            depth = np.ascontiguousarray(depth)
        return image, depth

    def frame_upload_fmt(self, slot, image, depth, fmt):
        """dsm_frame_upload_fmt: image uint8 [H,W] (mono8) or [H,W,3|4] (colour: converted to grey on the device, gray_from_color byte
        for byte), depth float32 or uint16 [H,W], as `fmt` (frame_format(...)) says; row strides are passed on as they are"""
        image, depth = self._frame_args_fmt(image, depth, fmt)
        self._check(self._lib.dsm_frame_upload_fmt(self._h, slot, _ptr(image), image.strides[0], _ptr(depth), depth.strides[0], C.byref(fmt)))

    def frame_upload_device_fmt(self, slot, image_ptr, img_step, depth_ptr, depth_step, fmt):
        self._check(self._lib.dsm_frame_upload_device_fmt(self._h, slot, _vp(image_ptr), img_step, _vp(depth_ptr), depth_step, C.byref(fmt)))

    def frame_upload_async_fmt(self, slot, image, depth, fmt):
        """dsm_frame_upload_async_fmt: views of PAGE-LOCKED memory (PinnedFrames(..., image_format=...)), untouched until
        frame_uploads_wait()"""
        ch = IMAGE_CHANNELS.get(fmt.image_format, 1)
        if image.dtype != np.uint8 or image.shape[:2] != (self.height, self.width) or depth.shape != (self.height, self.width):
            raise TypeError("image must be uint8 [H,W] or [H,W,C], depth [H,W]")
        if image.strides[1] != ch or depth.strides[1] != depth.dtype.itemsize:
            raise ValueError("rows must be contiguous")
        self._check(self._lib.dsm_frame_upload_async_fmt(self._h, slot, _ptr(image), image.strides[0], _ptr(depth), depth.strides[0], C.byref(fmt)))

    def frame(self, slot):
        """debug tap (dsm_debug_get_frame): (image uint8 [H,W], depth float32 [H,W]) of a frame slot as the kernels read them"""
        img = np.zeros((self.height, self.width), np.uint8)
        dep = np.zeros((self.height, self.width), np.float32)
        self._check(self._lib.dsm_debug_get_frame(self._h, slot, _ptr(img), _ptr(dep)))
        return img, dep

    def frame_planes(self, slot, image=None, depth=None):
        """debug tap (dsm_debug_frame_planes): the whole pitched planes of a slot, pad columns included.  With no argument: read,
        (image uint8 [H,pitch], depth float32 [H,pitch]); with image and / or depth of those shapes: the planes are overwritten."""
        pitch = self.frame_pitch()
        if image is None and depth is None:
            img = np.zeros((self.height, pitch), np.uint8)
            dep = np.zeros((self.height, pitch), np.float32)
            self._check(self._lib.dsm_debug_frame_planes(self._h, slot, 0, _ptr(img), _ptr(dep)))
            return img, dep
        image = None if image is None else np.ascontiguousarray(image, np.uint8).reshape(self.height, pitch)
        depth = None if depth is None else np.ascontiguousarray(depth, np.float32).reshape(self.height, pitch)
        self._check(self._lib.dsm_debug_frame_planes(self._h, slot, 1, None if image is None else _ptr(image), None if depth is None else _ptr(depth)))
        return None

    def frame_uploads_wait(self):
        self._check(self._lib.dsm_frame_uploads_wait(self._h))

    def frame_upload_device(self, slot, image_ptr, img_step, depth_ptr, depth_step):
        self._check(self._lib.dsm_frame_upload_device(self._h, slot, _vp(image_ptr), img_step, _vp(depth_ptr),
                                                      depth_step))

    def fuse_frame_resident(self, slot, reference_frame_index, pose, inv_pose=None):
        pose_cm = pose_to_colmajor(pose)
        _keep, inv = _inv_ptr(inv_pose)
        self._check(self._lib.dsm_fuse_frame_resident_inv(self._h, slot, reference_frame_index, _ptr(pose_cm), inv))

    @staticmethod
    def pack_replay(slots, ref_idx, poses):
        slots = np.ascontiguousarray(slots, np.int32)
        ref_idx = np.ascontiguousarray(ref_idx, np.int32)
        poses_cm = np.ascontiguousarray(np.asarray(poses, np.float32).transpose(0, 2, 1)).reshape(len(slots), 16)
        return slots, ref_idx, poses_cm

    def replay_enqueue(self, slots, ref_idx, poses_cm, inv_poses_cm=None):
        """slots/ref_idx int32 [n], poses_cm float32 [n,16] column-major (see pack_replay); inv_poses_cm: the caller's own
        inverses in the same layout, or None."""
        inv = None
        if inv_poses_cm is not None:
            inv_poses_cm = np.ascontiguousarray(inv_poses_cm, np.float32).reshape(len(slots), 16)
            inv = _ptr(inv_poses_cm)
        self._check(self._lib.dsm_replay_enqueue_inv(self._h, len(slots), _ptr(slots), _ptr(ref_idx), _ptr(poses_cm), inv))

    def replay_enqueue_host(self, pinned, first, ref_idx, poses_cm, inv_poses_cm=None):
        """frames first .. first+n-1 of a PinnedFrames block (n = len(ref_idx)) fused in order, each group of frames uploaded on
        the stream that runs its superpixel stages, right in front of them (include/dsm.h, dsm_replay_enqueue_host); the block's
        frames may be rewritten once replay_wait says the call is done"""
        n = len(ref_idx)
        assert 0 <= first and first + n <= pinned.n and (pinned.h, pinned.w, pinned.pitch) == (self.height, self.width, self.frame_pitch())
        if n == 0:
            return
        img, dep = pinned.image(first), pinned.depth(first)
        inv = None
        if inv_poses_cm is not None:
            inv_poses_cm = np.ascontiguousarray(inv_poses_cm, np.float32).reshape(n, 16)
            inv = _ptr(inv_poses_cm)
        ref_idx = np.ascontiguousarray(ref_idx, np.int32)
        poses_cm = np.ascontiguousarray(poses_cm, np.float32).reshape(n, 16)
        if pinned.fmt is not None:
            self._check(self._lib.dsm_replay_enqueue_host_fmt(self._h, n, _ptr(img), img.strides[0], pinned._bytes_img, _ptr(dep),
                                                              dep.strides[0], pinned._bytes_dep, _ptr(ref_idx), _ptr(poses_cm), inv,
                                                              C.byref(pinned.fmt)))
            return
        if pinned.depth_u16 is not None:
            self._check(self._lib.dsm_replay_enqueue_host_u16(self._h, n, _ptr(img), img.strides[0], pinned.pitch * pinned.h, _ptr(dep),
                                                              dep.strides[0], pinned.pitch * pinned.h * 2, _ptr(ref_idx), _ptr(poses_cm), inv,
                                                              *pinned.depth_u16_args))
            return
        self._check(self._lib.dsm_replay_enqueue_host(self._h, n, _ptr(img), img.strides[0], pinned.pitch * pinned.h, _ptr(dep), dep.strides[0],
                                                      pinned.pitch * pinned.h * 4, _ptr(ref_idx), _ptr(poses_cm), inv))

    def replay_wait(self, calls_back=0):
        """host wait until the frames of the replay_enqueue_host call `calls_back` calls ago have been fused"""
        self._check(self._lib.dsm_replay_wait(self._h, int(calls_back)))

    def synchronize(self):
        self._check(self._lib.dsm_synchronize(self._h))

    def last_new_count(self) -> int:
        n = C.c_int32(0)
        self._check(self._lib.dsm_last_new_count(self._h, C.byref(n)))
        return n.value

    def stream(self) -> int:
        s = _vp()
        self._check(self._lib.dsm_stream(self._h, C.byref(s)))
        return s.value or 0

    # ---- parity taps -----------------------------------------------------------------------
    def labels(self) -> np.ndarray:  # FusionFunctions::superpixel_index
        out = np.zeros((self.height, self.width), np.int32)
        self._check(self._lib.dsm_get_labels(self._h, _ptr(out)))
        return out

    def seeds(self) -> np.ndarray:  # FusionFunctions::superpixel_seeds
        out = np.zeros(self.n_seed, SEED_DTYPE)
        self._check(self._lib.dsm_get_seeds(self._h, _ptr(out)))
        return out

    # ---- state-level test taps ---------------------------------------------------------------
    STAGES = ("init_seeds", "assign_0", "update_seeds_0", "commit_seeds_0", "assign_1", "resolve_1", "update_seeds_1",
              "commit_seeds_1", "assign_2", "resolve_2", "update_seeds_2", "commit_seeds_2", "seed_points", "seed_fit",
              "fuse_surfels", "frame_tail")

    def debug_run_stages(self, slot, reference_frame_index, pose, first, last):
        pose_cm = pose_to_colmajor(pose)
        self._check(self._lib.dsm_debug_run_stages(self._h, slot, reference_frame_index, _ptr(pose_cm),
                                                   self.STAGES.index(first), self.STAGES.index(last)))

    def debug_get_labels(self, which) -> np.ndarray:
        out = np.zeros((self.height, self.width), np.int32)
        self._check(self._lib.dsm_debug_get_label_buffer(self._h, which, _ptr(out)))
        return out

    def debug_set_labels(self, which, labels):
        a = np.ascontiguousarray(labels, np.int32)
        self._check(self._lib.dsm_debug_set_label_buffer(self._h, which, _ptr(a)))

    def debug_get_seed_state(self):
        core = np.zeros((self.n_seed, 4), np.float32)
        stable = np.zeros(self.n_seed, np.int32)
        self._check(self._lib.dsm_debug_get_seed_state(self._h, _ptr(core), _ptr(stable)))
        return core, stable

    def debug_set_seed_state(self, core, stable):
        core = np.ascontiguousarray(core, np.float32)
        stable = np.ascontiguousarray(stable, np.int32)
        self._check(self._lib.dsm_debug_set_seed_state(self._h, _ptr(core), _ptr(stable)))

    def debug_tier_counts(self):
        """second-tier occupancy of the latest frame's lane-per-seed kernels (include/dsm.h, dsm_debug_tier_counts)"""
        out = np.zeros(8, np.int32)
        self._check(self._lib.dsm_debug_tier_counts(self._h, out.ctypes.data_as(_vp)))
        return {"huber_rest_by_sweep": [int(out[0]), int(out[2]), int(out[4])], "long_list_by_sweep": [int(out[1]), int(out[3]), int(out[5])],
                "fit_long_groups": int(out[6])}

    def debug_dropin_stats(self):
        """the drop-in calls' delta downloads so far (include/dsm.h, dsm_debug_dropin_stats)"""
        out = np.zeros(8, np.int64)
        self._check(self._lib.dsm_debug_dropin_stats(self._h, out.ctypes.data_as(_vp)))
        return {"calls": int(out[0]), "delta_calls": int(out[1]), "delta_groups": int(out[2]), "last_groups": int(out[3]),
                "host_us": {"frame_staging": int(out[4]), "map_compare_or_upload": int(out[5]), "gpu_wait": int(out[6]), "fetch_and_patch": int(out[7])}}

    def debug_set_fit_small_cap(self, cap):
        self._check(self._lib.dsm_debug_set_fit_small_cap(self._h, int(cap)))

    def debug_wave_stamps(self) -> np.ndarray:
        out = np.zeros((5, self.n_seed, 8), np.int64)
        self._check(self._lib.dsm_debug_wave_stamps(self._h, _ptr(out)))
        return out

    def replay_timed(self, slots, ref_idx, poses_cm):
        """Eager replay with a HIP event pair around every kernel; returns {stage: (ms_total, launches)}."""
        st = _StageTimes()
        self._check(self._lib.dsm_replay_timed(self._h, len(slots), _ptr(slots), _ptr(ref_idx), _ptr(poses_cm),
                                               C.byref(st)))
        self.event_overhead_ms = st.event_overhead_ms / max(st.frames, 1)
        self.timed_mean_new = st.sum_new / max(st.frames, 1)      # K: surfels created per frame
        self.timed_mean_local = st.sum_local / max(st.frames, 1)  # M: live surfels after a frame
        return {st.name[i].decode(): (st.ms[i], st.launches[i]) for i in range(st.n_stages)}, st.frames


class PinnedFrames:
    """n frames in page-locked host memory (dsm_host_alloc), rows laid out with a handle's slot pitch, pad columns zero:
    image(i) / depth(i) are [H,W] views that dsm_frame_upload_async moves in one transfer per plane."""

    @staticmethod
    def layout(height, width, tight=False, depth_u16=None, image_format=None):
        """(pitch in pixels, bytes per image pixel, image bytes per frame, depth bytes per frame) of a block: host arithmetic only"""
        pitch = int(width) if tight else (int(width) + 63) // 64 * 64
        ch = 1 if image_format in (None, "mono8", IMAGE_MONO8) else image_channels(image_format)
        return pitch, ch, pitch * int(height) * ch, pitch * int(height) * (4 if depth_u16 is None else 2)

    def __init__(self, ff, n: int, tight: bool = False, depth_u16=None, image_format=None, gray_weights=None):
        """ff: a FusionFunctions (its slot layout), or a (height, width) pair -- the pitch is then the library's rule,
        ceil(width / 64) * 64 elements per row, and frames_upload_async checks it against the handle's.  tight=True: rows
        `width` elements apart, frames back to back (`pitch` = width) -- the asynchronous uploads then move no pad bytes over
        the link and set the rows to the slots' pitch on the device.  depth_u16=(scale, op): the depth planes hold the sensor's
        uint16 (2 bytes a pixel), and frames_upload_async / replay_enqueue_host send them to the *_u16 entry points, which
        convert on the device (depth_from_u16).  image_format='rgb8' / 'bgr8' / 'rgba8' / 'bgra8' (gray_weights = (wr, wg, wb, shift),
        None = GRAY_OPENCV_14BIT): the image planes hold the camera's packed colour pixels, image(i) is a [H,W,3|4] view, rows
        3 or 4 x pitch bytes apart, and the uploads go to the *_fmt entry points, which convert to grey on the device
        (gray_from_color) -- together with float or uint16 depth."""
        self._lib = load_library()
        self.image_format = None if image_format in (None, "mono8", IMAGE_MONO8) else image_format
        self.channels = 1 if self.image_format is None else image_channels(self.image_format)
        self.fmt = None if self.image_format is None else frame_format(self.image_format, gray_weights, depth_u16)
        self.depth_u16 = None if depth_u16 is None else (float(depth_u16[0]), depth_u16[1])
        self.depth_u16_args = None if depth_u16 is None else (self.depth_u16[0], depth_op_code(self.depth_u16[1]))
        de = 4 if depth_u16 is None else 2
        if isinstance(ff, tuple):
            self.n, self.h, self.w = n, int(ff[0]), int(ff[1])
            self.pitch = (self.w + 63) // 64 * 64
        else:
            self.n, self.h, self.w, self.pitch = n, ff.height, ff.width, ff.frame_pitch()
        if tight:
            self.pitch = self.w
        self._bytes_img, self._bytes_dep = self.pitch * self.h * self.channels, self.pitch * self.h * de
        p = _vp()
        rc = self._lib.dsm_host_alloc(C.byref(p), n * (self._bytes_img + self._bytes_dep))
        if rc:
            raise DsmError(rc, "dsm_host_alloc")
        self._p = p
        raw = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n * (self._bytes_img + self._bytes_dep),))
        raw[:] = 0
        self._img = raw[: n * self._bytes_img].reshape((n, self.h, self.pitch) if self.channels == 1 else (n, self.h, self.pitch, self.channels))
        self._dep = raw[n * self._bytes_img:].view(np.float32 if de == 4 else np.uint16).reshape(n, self.h, self.pitch)

    def image(self, i):
        return self._img[i, :, : self.w]

    def depth(self, i):
        return self._dep[i, :, : self.w]

    def set(self, i, image, depth):
        self.image(i)[...] = image
        self.depth(i)[...] = depth

    def set_many(self, first, images, depths):
        """frames first .. first+n-1 from n (image uint8 [H,W], depth float32 [H,W]) pairs, copied by the library's host
        threads (dsm_host_pack_frames; the GIL is released for the call)"""
        n = len(images)
        if n == 0:
            return
        if first < 0 or first + n > self.n or len(depths) != n:
            raise ValueError("frames out of range")
        keep = []
        dt = self._dep.dtype
        ch = self.channels
        for im, dp in zip(images, depths):
            im = im if (im.dtype == np.uint8 and im.strides[1] == ch and (ch == 1 or im.strides[2] == 1)) else np.ascontiguousarray(im, np.uint8)
            dp = dp if (dp.dtype == dt and dp.strides[1] == dt.itemsize) else np.ascontiguousarray(dp, dt)
            if im.shape != ((self.h, self.w) if ch == 1 else (self.h, self.w, ch)) or dp.shape != (self.h, self.w):
                raise ValueError("frame size")
            keep.append((im, dp))
        ip = (C.c_void_p * n)(*[k[0].ctypes.data for k in keep])
        dp_ = (C.c_void_p * n)(*[k[1].ctypes.data for k in keep])
        ist = (C.c_size_t * n)(*[k[0].strides[0] for k in keep])
        dst = (C.c_size_t * n)(*[k[1].strides[0] for k in keep])
        pack = self._lib.dsm_host_pack_frames if dt == np.float32 else self._lib.dsm_host_pack_frames_u16
        more = ()
        if self.fmt is not None:
            pack, more = self._lib.dsm_host_pack_frames_fmt, (C.byref(self.fmt),)
        rc = pack(n, self.w, self.h, ip, ist, dp_, dst,
                  C.c_void_p(self._img[first].ctypes.data), C.c_size_t(self.pitch * ch), C.c_size_t(self._bytes_img),
                  C.c_void_p(self._dep[first].ctypes.data), C.c_size_t(self.pitch * dt.itemsize), C.c_size_t(self._bytes_dep), *more)
        if rc:
            raise DsmError(rc, self._lib.dsm_last_error(None).decode())

    def close(self):
        if getattr(self, "_p", None):
            self._img = self._dep = None
            self._lib.dsm_host_free(self._p)
            self._p = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """Handles of equal image size on one device advancing in lockstep: every kernel of a frame is launched once for all
    of them (include/dsm.h, dsm_batch_*).  The handles keep their own maps and frame slots and stay usable on their own
    (map_download, labels, ...) between batch calls."""

    def __init__(self, handles):
        self._lib = load_library()
        self.handles = list(handles)
        arr = (_vp * len(self.handles))(*[h._h for h in self.handles])
        b = _vp()
        rc = self._lib.dsm_batch_create(arr, len(self.handles), C.byref(b))
        if rc:
            raise DsmError(rc, self._lib.dsm_batch_last_error(None).decode())
        self._b = b

    def close(self):
        if getattr(self, "_b", None):
            self._lib.dsm_batch_destroy(self._b)
            self._b = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc:
            raise DsmError(rc, self._lib.dsm_batch_last_error(self._b).decode())

    @staticmethod
    def pack(plans):
        """[(slots[n], ref_idx[n], poses_cm[n,16]) per handle] (FusionFunctions.pack_replay) -> handle-major arrays."""
        n = len(plans[0][0])
        assert all(len(p[0]) == n for p in plans), "every handle of a batch advances by the same number of frames"
        return (np.ascontiguousarray(np.concatenate([p[0] for p in plans]), np.int32),
                np.ascontiguousarray(np.concatenate([p[1] for p in plans]), np.int32),
                np.ascontiguousarray(np.concatenate([p[2] for p in plans]), np.float32), n)

    def replay_enqueue(self, slots, ref_idx, poses_cm, n_frames, inv_poses_cm=None):
        inv = None
        if inv_poses_cm is not None:
            inv_poses_cm = np.ascontiguousarray(inv_poses_cm, np.float32).reshape(len(slots), 16)
            inv = _ptr(inv_poses_cm)
        self._check(self._lib.dsm_batch_replay_enqueue_inv(self._b, n_frames, _ptr(slots), _ptr(ref_idx), _ptr(poses_cm), inv))

    def synchronize(self):
        self._check(self._lib.dsm_batch_synchronize(self._b))

    def replay_timed(self, slots, ref_idx, poses_cm, n_frames):
        """Eager batched replay with a HIP event pair around every (batched) kernel; returns {stage: (ms_total, launches)}
        and the number of handle-frames."""
        st = _StageTimes()
        self._check(self._lib.dsm_batch_replay_timed(self._b, n_frames, _ptr(slots), _ptr(ref_idx), _ptr(poses_cm), C.byref(st)))
        self.event_overhead_ms = st.event_overhead_ms / max(st.frames, 1)
        self.timed_mean_new = st.sum_new / max(st.frames, 1)
        self.timed_mean_local = st.sum_local / max(st.frames, 1)
        return {st.name[i].decode(): (st.ms[i], st.launches[i]) for i in range(st.n_stages)}, st.frames
