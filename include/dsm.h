/* dsm.h -- C ABI of the MI355X-native surfel-fusion hot path.
 *
 * This is the boundary a maintainer of HKUST-Aerial-Robotics/DenseSurfelMapping binds
 * instead of the in-process CPU engine.  Reference interfaces replaced (paths relative
 * to the reference checkout):
 *
 *   dsm_create / dsm_destroy      <- FusionFunctions::initialize
 *                                    surfel_fusion/src/fusion_functions.h:84-87, .cpp:7-28
 *   dsm_fuse_initialize_map       <- FusionFunctions::fuse_initialize_map
 *                                    surfel_fusion/src/fusion_functions.h:88-94, .cpp:30-83
 *   dsm_fuse_map                  <- SurfelMap::fuse_map (engine call + hole refill /
 *                                    swap-with-last compaction)
 *                                    surfel_fusion/src/surfel_map.cpp:1060-1113
 *   dsm_surfel / dsm_seed         <- SurfelElement / Superpixel_seed, bit-for-bit
 *                                    surfel_fusion/src/elements.h:5-31
 *
 * Everything else (resident map, frame slots, replay queue, taps) is what an HBM-resident
 * engine needs and the CPU reference has no counterpart for.
 *
 * Conventions: plain pointers and sizes, no exceptions; every call returns DSM_OK (0) or a
 * negative dsm_status; dsm_last_error() gives the message.  A handle owns its device buffers and, with
 * pipeline_depth < 4, all of its streams (from 4 on it also launches on the device's shared per-queue streams,
 * see dsm_config.pipeline_depth) and is single-threaded-use (like a FusionFunctions instance,
 * whose scratch buffers are members: fusion_functions.h:34-37); use one handle per
 * concurrent subsequence.  There is no CPU fallback: dsm_create fails with
 * DSM_E_NO_DEVICE when no gfx950 device is visible.
 */
#ifndef DSM_H
#define DSM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSM_ABI_VERSION 4 /* 3: the *_inv entry points (the caller's own pose inverse).  4: a batch no longer touches its handles'
                             streams at every call -- a handle's stream comes behind its batch at the handle's NEXT dsm_* call
                             (dsm_stream's note): a caller that cached the hipStream_t must fetch it again after batch calls;
                             dsm_create refuses DSM_FLAG_WAVE_STAMPS in a library built without stamp code; dsm_debug_tier_counts */

typedef enum {
    DSM_OK = 0,
    DSM_E_INVALID = -1,   /* bad argument (null pointer, dims, steps, slot index) */
    DSM_E_NO_DEVICE = -2, /* no HIP device / not gfx950 */
    DSM_E_HIP = -3,       /* a HIP runtime call failed; see dsm_last_error */
    DSM_E_CAPACITY = -4,  /* surfel capacity exceeded */
    DSM_E_STATE = -5      /* call made in the wrong state (e.g. nothing uploaded) */
} dsm_status;

/* elements.h:22-31 -- 44 bytes.  update_times == 0 marks a deleted slot. */
typedef struct dsm_surfel {
    float px, py, pz;
    float nx, ny, nz;
    float size;
    float color;
    float weight;
    int32_t update_times;
    int32_t last_update;
} dsm_surfel;

/* elements.h:5-20 -- 60 bytes (bool fused @48, bool stable @49, 2 pad bytes). */
typedef struct dsm_seed {
    float x, y;
    float size;
    float norm_x, norm_y, norm_z;
    float posi_x, posi_y, posi_z;
    float view_cos;
    float mean_depth;
    float mean_intensity;
    uint8_t fused;
    uint8_t stable;
    uint8_t pad_[2];
    float min_eigen_value, max_eigen_value;
} dsm_seed;

/* Constructor arguments of FusionFunctions::initialize plus the compile-time constant set of
 * fusion_functions.h:7-21 made run-time (the RGB-D set of lines 17-21 is needed for
 * 640x480 RGB-D input). */
typedef struct dsm_config {
    int32_t width, height;
    float fx, fy, cx, cy;
    float far_dist, near_dist;
    double huber_range;       /* HUBER_RANGE        0.4  (rgbd 0.05) */
    double baseline;          /* BASELINE           0.5  (rgbd 0.08) */
    double disparity_error;   /* DISPARITY_ERROR    4.0  (rgbd 1.0)  */
    double min_tolerate_diff; /* MIN_TOLERATE_DIFF  0.1  (rgbd 0.05) */
    int32_t device;           /* HIP device ordinal */
    int32_t surfel_capacity;  /* max resident surfels; 0 = default (4 Mi) */
    int32_t frame_slots;      /* resident frame slots in HBM; 0 = default (2) */
    uint32_t flags;           /* DSM_FLAG_* */
    int32_t pipeline_depth;   /* frames of one sequence whose superpixel stages may be in flight at once
                                 (1, 2, 4, 8, 12, 16, 24 or 32); 0 = default (4).  Results do not depend on it.  From 4 on,
                                 dsm_replay_enqueue launches the superpixel stages of G consecutive frames as one batch
                                 (every kernel once for all of them) while fuse + compaction of the previous group run
                                 in frame order: G = depth / 2 (two groups in turn) for 4 and 8, depth / 4 (four groups)
                                 for 16 and 32, depth / 3 (three groups) for 12 and 24.  From depth 4 on the streams the
                                 groups are launched on -- and with 12 / 24 the map stream too -- are the device's four
                                 process-wide per-queue streams, shared with batches and other handles: they carry
                                 launches only (graphs are captured on private streams), the handle's buffers stay its
                                 own.  24 is the fastest single-sequence setting on MI355X. */
} dsm_config;

#define DSM_FLAG_NO_GRAPH 1u /* launch kernels eagerly instead of replaying a hipGraph */
#define DSM_FLAG_UPLOAD_STREAM 2u /* dsm_frame_upload (the blocking call) runs on a stream of its own, overlapping the
                                     frames in flight on other slots (live feeds: the node).  Off by default: HIP spreads
                                     streams over 4 hardware queues in creation order, and one more stream per handle
                                     spreads the map streams of many handles unevenly (8-subsequence replay: -22 %).
                                     Handles of a batch cannot have it; replays that stream their frames -- batched or
                                     not -- use dsm_frames_upload_async, which needs no flag and no stream per handle. */

#define DSM_FLAG_WAVE_STAMPS 4u /* debug: allocate the per-wave phase-stamp buffer read by dsm_debug_wave_stamps -- in a library
                                   built with -DDSM_WAVE_STAMPS=1 (tools/wave_stamps.py); the shipped build has no stamp code in
                                   its kernels and dsm_create REFUSES the flag (DSM_E_INVALID): a profiling run on the wrong
                                   library fails at once instead of reading an empty buffer later */

#define DSM_FLAG_EIGEN33_PRODUCTS 8u /* evaluate the reference's 3x3 * 3x1 products -- the camera-frame normal of every surfel
                                        (FF.cpp:228, its delete test at :265-268), the normal of every new and every fused
                                        surfel (:296, :341) and dsm_frame_cloud's rotation_R * cam_point (SM.cpp:1139) -- in
                                        the order Eigen 3.3 / 3.4 give them, a0*b0 + (a1*b1 + a2*b2), instead of Eigen 3.2's
                                        (a0*b0 + a1*b1) + a2*b2.  Set it to match a reference built against Eigen >= 3.3 (what
                                        Ubuntu 18.04 and later ship) byte for byte; leave it clear for Eigen 3.2 (the default).
                                        The other products (the 4x4 ones, and dsm_warp_surfels' dynamic
                                        MatrixXf products of SM.cpp:724, 774) are unchanged: DESIGN.md section 6.  Handles of
                                        one batch must agree on it. */

typedef struct dsm_handle dsm_handle;

/* Fill cfg with the driving constant set (fusion_functions.h:13-16) or, if rgbd != 0, the
 * RGB-D set (fusion_functions.h:17-21). */
int dsm_config_init(dsm_config *cfg, int width, int height, float fx, float fy, float cx, float cy,
                    float far_dist, float near_dist, int rgbd);

/* (width / 8) * (height / 8) <= 65 535 superpixels per frame (DSM_E_INVALID beyond: 4K frames are out of range, 1920x1080
 * has 32 400): superpixel indices are 16 bits in the device's label planes; the taps below speak int32, -1 = no superpixel. */
int dsm_create(const dsm_config *cfg, dsm_handle **out);
void dsm_destroy(dsm_handle *h);
const char *dsm_last_error(const dsm_handle *h); /* h may be NULL: last dsm_create error */
int dsm_abi_version(void);

/* ---- drop-in calls (host buffers in, host buffers out; synchronous) -------------------- */

/* FusionFunctions::fuse_initialize_map: image is 8-bit grey (img_step bytes per row), depth is
 * float metres with 0 = invalid (depth_step bytes per row), pose16 is the cam->world matrix,
 * column-major (Eigen::Matrix4f storage).  local[0..n_local) is updated in place; surfels
 * created by this frame are written to new_out[0..*n_new) in seed order. */
int dsm_fuse_initialize_map(dsm_handle *h, int reference_frame_index, const uint8_t *image, size_t img_step,
                            const float *depth, size_t depth_step, const float *pose16, dsm_surfel *local,
                            int32_t n_local, dsm_surfel *new_out, int32_t new_cap, int32_t *n_new);

/* SurfelMap::fuse_map: the call above followed by the reference's order-exact refill of deleted
 * slots and swap-with-last compaction.  *n_local is updated; cap is the capacity of local[].  More surfels than cap:
 * DSM_E_CAPACITY, *n_local = the count needed, *n_new = the frame's new surfels, local[] is left as it was handed in (its
 * records are the caller's first n); the frame has been fused on the device, so the same call again with room starts
 * from the caller's array once more.  More surfels than the HANDLE holds (dsm_config.surfel_capacity): DSM_E_CAPACITY as
 * well, but *n_local and *n_new are left as they were handed in and local[] is untouched -- no count is known, a larger
 * handle is needed (dsm_last_error names which of the two limits was hit). */
int dsm_fuse_map(dsm_handle *h, int reference_frame_index, const uint8_t *image, size_t img_step,
                 const float *depth, size_t depth_step, const float *pose16, dsm_surfel *local,
                 int32_t *n_local, int32_t cap, int32_t *n_new);

/* The same two calls with the world->cam matrix handed in.  FusionFunctions::fuse_initialize_map inverts the pose with the
 * caller's matrix library (`pose.inverse()`, Eigen::Matrix4f, fusion_functions.cpp:59); Eigen is not part of this library,
 * which uses the adjugate / determinant closed form instead -- equal to Eigen's result up to the last place, and a last
 * place of this matrix can flip a create / delete decision downstream.  A caller that has the
 * reference's matrix type computes inv_pose16 = pose.inverse() itself (include/dsm_fusion_functions.hpp does) and gets the
 * arithmetic of ITS Eigen build bit for bit; NULL = the closed form. */
int dsm_fuse_initialize_map_inv(dsm_handle *h, int reference_frame_index, const uint8_t *image, size_t img_step,
                                const float *depth, size_t depth_step, const float *pose16, const float *inv_pose16,
                                dsm_surfel *local, int32_t n_local, dsm_surfel *new_out, int32_t new_cap, int32_t *n_new);
int dsm_fuse_map_inv(dsm_handle *h, int reference_frame_index, const uint8_t *image, size_t img_step,
                     const float *depth, size_t depth_step, const float *pose16, const float *inv_pose16,
                     dsm_surfel *local, int32_t *n_local, int32_t cap, int32_t *n_new);

/* Page-locked host memory for frames handed to dsm_frame_upload / dsm_fuse_*: uploads from it run at PCIe
 * rate without a staging copy.  Plain malloc'ed buffers work too, slower. */
int dsm_host_alloc(void **out, size_t bytes);
void dsm_host_free(void *p);
/* n of the caller's frames (frame i: images[i] / depths[i] with their row steps in bytes -- n cv::Mat pairs as
 * SurfelMap::image_input / depth_input receive them, surfel_map.cpp:83-101) copied into page-locked memory in the layout the
 * asynchronous uploads read (dsm_frames_upload_async, dsm_replay_enqueue_host: rows dst_*_step bytes apart, frames
 * dst_*_frame_step apart) by the library's host threads, the caller's among them; pad bytes are left as they are.  Synchronous;
 * calls from several threads take turns. */
int dsm_host_pack_frames(int32_t n, int32_t width, int32_t height, const uint8_t *const *images, const size_t *image_steps,
                         const float *const *depths, const size_t *depth_steps, uint8_t *dst_image, size_t dst_img_step,
                         size_t dst_img_frame_step, float *dst_depth, size_t dst_depth_step, size_t dst_depth_frame_step);

/* ---- resident path: map and frames stay in HBM, calls are asynchronous on the handle's stream */

int dsm_map_upload(dsm_handle *h, const dsm_surfel *surfels, int32_t n);
int dsm_map_size(dsm_handle *h, int32_t *n);                       /* synchronises */
int dsm_map_capacity(const dsm_handle *h, int32_t *cap);           /* slots of the resident map (surfel_capacity rounded up) */
int dsm_map_download(dsm_handle *h, dsm_surfel *out, int32_t cap, int32_t *n); /* synchronises */
/* device-to-device copy of the resident map into caller-owned device memory (e.g. a torch
 * tensor's data_ptr) for the multi-GPU merge; synchronises. */
int dsm_map_copy_to_device(dsm_handle *h, void *dst_device, int32_t cap, int32_t *n);

/* ---- map maintenance between frames (the data-parallel parts of surfel_map.cpp:681-824, 1456-1595) ---- */

/* SurfelMap::warp_active_surfels_cpu_kernel (surfel_map.cpp:750-789): p' = M*(p,1), n' = M[0:3,0:3]*n for
 * every resident surfel; warp16 = (loop_pose * cam_pose^-1).cast<float>(), column-major (surfel_map.cpp:808-813).
 * Asynchronous on the handle's stream. */
int dsm_map_warp(dsm_handle *h, const float *warp16);
/* SurfelMap::warp_inactive_surfels_cpu_kernel (surfel_map.cpp:681-748) on caller-owned DEVICE memory: the
 * attached surfels of n_groups keyframes stored back to back, group g = [offsets[g], offsets[g+1]) warped by
 * mats16[16 g ..].  offsets (n_groups+1) and mats16 are host arrays.  Synchronises. */
int dsm_warp_grouped_device(dsm_handle *h, void *surfels_device, int32_t n_groups, const int32_t *offsets,
                            const float *mats16);
/* move_add_surfels, removal half (surfel_map.cpp:1476-1497): copy the live resident surfels whose
 * last_update == key to out[] in index order and mark their slots deleted.  Synchronises. */
int dsm_map_extract(dsm_handle *h, int32_t key, dsm_surfel *out, int32_t cap, int32_t *n);
/* move_add_surfels, insertion half (surfel_map.cpp:1583-1590): append to the resident map. */
int dsm_map_append(dsm_handle *h, const dsm_surfel *surfels, int32_t n);

/* ---- inactive store: the surfels of keyframes that left the local window stay in HBM, back to back in
 * deactivation order, each with the XYZI point the reference keeps in `inactive_pointcloud`
 * (surfel_map.cpp:1476-1497 fills poses_database[i].attached_surfels and inactive_pointcloud; here both are
 * one device arena indexed like inactive_pointcloud).  The segment table (which keyframe owns [begin,
 * begin+n)) is host state of the caller -- include/dsm_surfel_map.h keeps it as the reference does
 * (points_begin_index / points_pose_index / pointcloud_pose_index). ---- */

/* surfel_map.cpp:1476-1497: move the live resident surfels with last_update == key, in index order, to the
 * end of the store (slots marked deleted in the map).  Returns the segment.  Synchronises. */
int dsm_store_deactivate(dsm_handle *h, int32_t key, int32_t *begin, int32_t *n);
/* surfel_map.cpp:1583-1590: append store[begin, begin+n) to the resident map (the store is not changed). */
int dsm_store_activate(dsm_handle *h, int32_t begin, int32_t n);
/* surfel_map.cpp:1551-1553 (`inactive_pointcloud->erase`): remove [begin, begin+n); the tail moves down. */
int dsm_store_erase(dsm_handle *h, int32_t begin, int32_t n);
/* surfel_map.cpp:681-748 for every keyframe at once: offsets[n_groups+1] tile the store, group g is warped
 * by mats16[16 g ..] (column-major float) when changed[g] != 0 and left alone otherwise; the XYZI shadow is
 * refreshed for all points of a warped group except its last (surfel_map.cpp:742).  Synchronises. */
int dsm_store_warp(dsm_handle *h, int32_t n_groups, const int32_t *offsets, const float *mats16,
                   const uint8_t *changed);
int dsm_store_size(dsm_handle *h, int32_t *n);
/* either output may be NULL; xyzi_out receives 4 floats per point (x, y, z, intensity).  Synchronises. */
int dsm_store_download(dsm_handle *h, int32_t begin, int32_t n, dsm_surfel *surfels_out, float *xyzi_out);

/* ---- point-cloud publications (the reference's publish_*_pointcloud, surfel_map.cpp:1115-1151, 1283-1454): XYZI points,
 * 4 floats each (x, y, z, intensity), the layout of dsm_store_download's xyzi_out ---- */
typedef enum {
    DSM_CLOUD_SELECT_NONE = 0,    /* no map part */
    DSM_CLOUD_SELECT_MATURE = 1,  /* resident records with update_times >= 5, map order (publish_active_pointcloud :1398-1417) */
    DSM_CLOUD_SELECT_NONZERO = 2  /* resident records with update_times != 0, map order (publish_neighbor_pointcloud :1292-1303) */
} dsm_cloud_select;
/* The map part chosen by `select`, then the store's XYZI shadow runs [store_begin[s], +store_count[s]) for s < n_segments,
 * in list order (empty runs and an empty list are allowed).  ACTIVE = (MATURE, no runs), INACTIVE = (NONE, [0, store size)),
 * ALL = (MATURE, [0, store size)), NEIGHBOR = (NONZERO, the runs of the drift-free neighbours).  dst is host memory
 * (dst_on_device = 0; pageable or dsm_host_alloc'ed) or device memory.  *n = the number of points; more than cap:
 * DSM_E_CAPACITY, *n = the count needed, nothing written past cap.  A run outside the store: DSM_E_INVALID before any device
 * work.  A device destination is written behind the work enqueued on the null stream so far (as by a hipMemcpy).
 * Synchronises. */
int dsm_cloud_compose(dsm_handle *h, int select, int32_t n_segments, const int32_t *store_begin, const int32_t *store_count,
                      void *dst, int dst_on_device, int32_t cap, int32_t *n);
/* publish_raw_pointcloud (:1115-1151) of the frame in `slot`: width * height points, unfiltered, COLUMN-major (point i * height + j
 * is pixel column i, row j), world = R * ((i - cx) * d / fx, (j - cy) * d / fy, d) + T with R = Quaternionf(qw, qx, qy, qz)
 * (the doubles cast to float, not normalised).toRotationMatrix(), T = (px, py, pz) as float; intensity = the image byte.
 * pose7 = px py pz qx qy qz qw.  The launch reads the slot: a later upload into it comes behind (the call synchronises).  A
 * device destination is ordered like dsm_cloud_compose's. */
int dsm_frame_cloud(dsm_handle *h, int slot, const double *pose7, void *dst, int dst_on_device, int32_t cap, int32_t *n);

/* ---- the hexagon mesh (the reference's save_mesh, surfel_map.cpp:1176-1280): six vertices per surfel -- the corners of a
 * hexagon of circumradius `size` in the surfel's plane, exactly push_a_surfel's arithmetic -- and four triangles ---- */
typedef enum {
    DSM_MESH_VERTEX_REF6 = 0,      /* x y z c c c as six floats, c = (float)(int)color: the reference's `vertexs`; 144 bytes per surfel */
    DSM_MESH_VERTEX_XYZ_RGBA8 = 1  /* x y z as floats, then the bytes r g b 255 with r = g = b = (int)color clamped to 0..255: a
                                      vertex buffer; 96 bytes per surfel */
} dsm_mesh_vertex_layout;
/* The vertices of the store's RECORD runs [store_begin[s], +store_count[s]) for s < n_segments, in list order, THEN those of
 * the map part chosen by `select` (dsm_cloud_select), in map order: save_mesh's order, the REVERSE of dsm_cloud_compose's (map
 * part first).  cap_surfels and *n_surfels count surfels (six vertices each); dst holds cap_surfels * 144 or * 96 bytes, host
 * memory (dst_on_device = 0) or device memory (4-byte aligned; 16-byte alignment is faster).  (int)color of a NaN or of a
 * value outside int is INT_MIN, as the reference's x86 conversion gives.  Everything else as dsm_cloud_compose: a bad run is
 * DSM_E_INVALID before any device work; more than cap_surfels: DSM_E_CAPACITY, *n_surfels = the count needed, nothing written
 * past cap_surfels; a device destination is written behind the work enqueued on the null stream so far.  Synchronises. */
int dsm_mesh_compose(dsm_handle *h, int select, int32_t n_segments, const int32_t *store_begin, const int32_t *store_count,
                     int vertex_layout, void *dst, int dst_on_device, int32_t cap_surfels, int32_t *n_surfels);
/* The index buffer of n_surfels hexagons: 12 uint32 each, 6 i + {0,1,2, 1,3,2, 2,3,4, 4,3,5} (the faces of :1274-1277), into
 * host or device memory (n_surfels * 48 bytes; at most 715827882 surfels: the vertex index is 32 bits).  Synchronises. */
int dsm_mesh_indices(dsm_handle *h, int32_t n_surfels, void *dst, int dst_on_device);

/* ---- the map as an image: what a pinhole camera at any pose sees of the surfels (no counterpart in the reference) ----
 * The surfel sequence is dsm_mesh_compose's: the store's RECORD runs in list order, then the map part chosen by `select`;
 * surfel number i of a render is surfel i of the mesh.  A surfel is a disc of radius `size` about its position in the plane
 * of its normal.  The ray of pixel (u, v) is ((u - cx) / fx, (v - cy) / fy, 1): it passes through the integer pixel
 * coordinate, as the fuse kernel's projection assumes.  With p_c, n_c the surfel's centre and normal in the camera frame,
 * z = (n_c . p_c) / (n_c . ray); the pixel is hit iff near_dist < z < far_dist (z finite) and |z ray - p_c|^2 <= size * size.
 * So a zero normal, an edge-on disc and a record with a NaN or an infinity never hit.  The pixel shows the hit with the
 * smallest 64-bit key (bits of z) << 32 | surfel number: the nearest, the lower number on an exact tie -- a minimum over a
 * total order, so the image does not depend on the order the GPU finds the hits in and is reproducible bit for bit. */
typedef struct dsm_render_camera {
    int32_t width, height;     /* 1 .. 8192 each; independent of the handle's frame size */
    float fx, fy, cx, cy;      /* fx, fy > 0 */
    float near_dist, far_dist; /* 0 < near_dist < far_dist */
} dsm_render_camera;
/* tight row-major planes, host or device memory; any may be NULL (not written), not all */
typedef struct dsm_render_planes {
    float *depth;       /* [height][width]     camera-frame z of the nearest hit; 0.0f where nothing is hit */
    int32_t *index;     /* [height][width]     its surfel number in the sequence; -1 */
    float *normal;      /* [height][width][3]  its normal rotated into the camera frame (in DSM_FLAG_EIGEN33_PRODUCTS' order on a
                                               handle created with that flag); 0 0 0 */
    uint8_t *intensity; /* [height][width]     (int)color clamped to 0..255, the byte of DSM_MESH_VERTEX_XYZ_RGBA8; 0 */
} dsm_render_planes;
#define DSM_RENDER_CULL_BACKFACES 1u /* also drop surfels with n_c . p_c >= 0 (the default is two-sided) */
/* pose16: cam -> world, 16 column-major floats as for dsm_fuse_map; pose_inv16: the caller's own world -> cam matrix (the
 * rule of the *_inv entry points) or NULL = the closed-form inverse.  *n_surfels = the length of the sequence: index values
 * are below it.  Checked before any device work (DSM_E_INVALID, nothing written): a run outside the store, width / height
 * outside 1..8192, fx / fy not positive, near_dist <= 0 or near_dist >= far_dist, a non-finite camera or pose entry, all four
 * planes NULL, unknown flags.  Launched eagerly on the handle's stream behind the frames enqueued so far; a device
 * destination is ordered like dsm_cloud_compose's.  Synchronises. */
int dsm_render_compose(dsm_handle *h, int select, int32_t n_segments, const int32_t *store_begin, const int32_t *store_count,
                       const dsm_render_camera *camera, const float *pose16, const float *pose_inv16, uint32_t flags,
                       const dsm_render_planes *planes, int dst_on_device, int32_t *n_surfels);

/* ---- the map as an occupancy voxel grid: what a planner or a collision checker consumes (no counterpart in the reference) ----
 * The grid is fixed to the world: origin = the low corner of voxel (0, 0, 0), `voxel` the edge in metres, nx x ny x nz voxels;
 * the centre of voxel i along axis a is c_a = origin_a + ((float)i + 0.5f) * voxel.  The surfel sequence is dsm_render_compose's
 * (the store's RECORD runs in list order, then the map part chosen by `select`); a surfel is the renderer's disc -- centre p,
 * normal n (not assumed unit), radius `size`, in world coordinates as stored; no pose is involved.  fp32, non-fused, in the
 * order written.  Per surfel: rejected unless px, py, pz are finite, size >= 0 (a NaN fails, +inf stays) and
 * nn = (nx nx + ny ny) + nz nz is finite and > 0; then h = voxel * 0.5f, l1 = (|nx| + |ny|) + |nz|, ta = (h l1) (h l1),
 * r = size + h, rb = (r r) nn.  Per voxel: d = c - p, e = (nx dx + ny dy) + nz dz, e2 = e e, q = (dx dx + dy dy) + dz dz; the
 * voxel is COVERED iff e2 <= ta and q nn - e2 <= rb: the disc's plane cuts the cube, and the centre's distance from the disc's
 * axis is at most size + h.  No division, no square root; a NaN fails every comparison; an infinite size covers its whole slab.
 * Every output is a minimum or an OR over a total order: the result does not depend on the order the GPU finds the covers in
 * and is reproducible bit for bit. */
typedef struct dsm_grid_spec {
    uint32_t struct_size; /* sizeof(dsm_grid_spec) */
    float origin[3];      /* finite */
    float voxel;          /* finite, > 0 */
    int32_t nx, ny, nz;   /* >= 1 each, nx * ny * nz <= 2^28 */
    int32_t inflate;      /* radius of the inflation in voxels, 0 .. 16 */
} dsm_grid_spec;
/* origin 0, voxel 0.1 m, 1 x 1 x 1, inflate 0 */
void dsm_grid_spec_init(dsm_grid_spec *spec);
/* A grid of nx x ny x nz voxels around `centre` on the lattice of multiples of `voxel`: origin_a = (float)(floor((double)centre_a
 * / voxel - n_a / 2.0) * (double)voxel), so that grids taken around successive poses share one lattice.  struct_size and inflate
 * are left as they are.  Nothing is checked here: dsm_grid_compose does. */
void dsm_grid_spec_around(dsm_grid_spec *spec, const float *centre /* 3 */, float voxel, int32_t nx, int32_t ny, int32_t nz);
/* tight row-major planes, host or device memory; any may be NULL (not written), not all; no two may be the same memory, and
 * device planes are 4-byte aligned.  wx = (nx + 31) / 32. */
typedef struct dsm_grid_planes {
    uint32_t *occupied; /* [nz][ny][wx]  bit x & 31 of word x >> 5 is set iff voxel (x, y, z) is covered; pad bits (x >= nx) are 0 */
    uint32_t *inflated; /* [nz][ny][wx]  set iff some occupied voxel lies at an integer offset with dx^2 + dy^2 + dz^2 <= inflate^2
                                         (outside the grid everything is free; inflate = 0 gives a copy): the configuration-space map
                                         of a robot of radius inflate * voxel */
    int32_t *index;     /* [nz][ny][nx]  the lowest surfel number among the surfels covering the voxel; -1 */
    int32_t *cells;     /* [cells_cap]   the linear indices (z ny + y) nx + x of the set voxels of `occupied` (of `inflated` with
                                         DSM_GRID_CELLS_OF_INFLATED), ascending: the voxel-down-sampled cloud */
    int32_t cells_cap;  /* >= 0 when cells is not NULL */
} dsm_grid_planes;
#define DSM_GRID_CELLS_OF_INFLATED 1u
/* *n_surfels = the length of the sequence (index values are below it), *n_cells = the number of cells (0 without `cells`).  More
 * cells than cells_cap: DSM_E_CAPACITY with *n_cells = the count needed; the other planes are complete and nothing is written
 * past the cap.  Checked before any device work (DSM_E_INVALID, nothing written): a run outside the store, a wrong struct_size,
 * a non-finite origin, voxel not finite or not positive, a dimension < 1, nx * ny * nz > 2^28, inflate outside 0..16, all four
 * planes NULL, two planes the same pointer, a device plane not 4-byte aligned, cells with cells_cap < 0, unknown flags.  The map, the store and the frame slots are not changed.  Launched
 * eagerly on the handle's stream behind the frames enqueued so far; a device destination is ordered like dsm_cloud_compose's.
 * Synchronises. */
int dsm_grid_compose(dsm_handle *h, int select, int32_t n_segments, const int32_t *store_begin, const int32_t *store_count,
                     const dsm_grid_spec *spec, uint32_t flags, const dsm_grid_planes *planes, int dst_on_device, int32_t *n_surfels,
                     int32_t *n_cells);
/* The inflation alone, on a caller's bit set in DEVICE memory ([nz][ny][wx] words each, read and written behind the work
 * enqueued on the null stream so far): dst = src dilated by the voxels within `radius` (0 .. 16).  Pad bits of src are ignored,
 * pad bits of dst are 0.  src and dst overlapping (src == dst included) or not 4-byte aligned, a NULL, a dimension < 1, more than
 * 2^28 voxels, a radius outside 0..16: DSM_E_INVALID
 * before any device work.  Synchronises. */
int dsm_grid_inflate(dsm_handle *h, int32_t nx, int32_t ny, int32_t nz, int32_t radius, const void *src_device, void *dst_device);

/* ---- the truncated Euclidean distance field of the grid: what a planner or a trajectory optimiser consumes ----
 * Input: a bit set O in the grid layout ([nz][ny][wx] words, wx = (nx + 31) / 32, pad bits ignored) and a truncation radius
 * max_dist = R in voxels, 1 <= R <= DSM_FIELD_MAX_DIST.  Outside the grid everything is free, as for the inflation.  For voxel
 * v = (x, y, z) let key(o) = (uint64)|v - o|^2 << 32 | lin(o) over the set voxels o with |v - o|^2 <= R^2, where |.|^2 is the
 * integer squared distance in voxels and lin(o) = (oz ny + oy) nx + ox.  The result for v is the MINIMUM key: the nearest occupied
 * voxel, on an exact tie the one with the lowest linear index.  A minimum over a total order: it does not depend on how the GPU
 * arranges its passes and is reproducible bit for bit.  An occupied voxel has dist2 0 and nearest = itself;
 * inflated(r) == (dist2 <= r * r) for every r <= R.  `distance` is table[dist2] with table[k] = (float)((double)voxel *
 * sqrt((double)k)), k = 0 .. R^2, built on the host and uploaded: no square root is taken on the device.  A voxel with no key gets
 * table[R^2], "at least this far"; dist2 tells the two cases apart.
 * Not provided: a signed field (the distance to free space inside obstacles), gradients, and the field of the inflated set. */
#define DSM_FIELD_MAX_DIST 64
#define DSM_FIELD_FAR 65535u
/* tight row-major [nz][ny][nx] planes; any may be NULL (not written), not all; no two may be the same memory; device planes are
 * aligned to their element */
typedef struct dsm_field_planes {
    uint16_t *dist2;  /* the high half of the minimum key (<= 4096); DSM_FIELD_FAR when no key exists */
    int32_t *nearest; /* the low half of the minimum key: the linear index of the nearest set voxel; -1 */
    float *distance;  /* metres: table[dist2]; table[R^2] when no key exists */
} dsm_field_planes;
/* The field of a caller's bit set in DEVICE memory into device planes, ordered and synchronised as dsm_grid_inflate.  `voxel` is
 * the edge in metres (read only when `distance` is asked for).  The intermediates cost up to 8 bytes a voxel of grow-only handle
 * scratch, hence the limit of 2^26 voxels.  DSM_E_INVALID before any device work, nothing written: a NULL handle, source or
 * planes; a dimension < 1; more than 2^26 voxels; max_dist outside 1..64; voxel not finite or not > 0 while `distance` is asked
 * for; all three planes NULL; two planes the same pointer; a plane overlapping the source; the source, `nearest` or `distance`
 * not 4-byte aligned, `dist2` not 2-byte aligned.  Synchronises. */
int dsm_grid_distance(dsm_handle *h, int32_t nx, int32_t ny, int32_t nz, int32_t max_dist, float voxel, const void *src_device,
                      const dsm_field_planes *planes_device);
/* The field of the map: the occupied set of dsm_grid_compose for the same sequence and `spec` (composed into handle scratch), then
 * its field into host or device planes (dst_on_device as for dsm_grid_compose; the alignment rule holds for device planes).
 * spec->inflate is validated as always and otherwise unused; at most 2^26 voxels; flags must be 0.  *n_surfels = the length of the
 * sequence, as dsm_grid_compose reports it.  Checked before any device work (DSM_E_INVALID, nothing written): what
 * dsm_grid_compose checks of the sequence and the spec, and what dsm_grid_distance checks of max_dist, the voxel and the planes.
 * The map, the store and the frame slots are not changed.  Synchronises. */
int dsm_field_compose(dsm_handle *h, int select, int32_t n_segments, const int32_t *store_begin, const int32_t *store_count,
                      const dsm_grid_spec *spec, int32_t max_dist, uint32_t flags, const dsm_field_planes *planes, int dst_on_device,
                      int32_t *n_surfels);

/* ---- free and unknown space: the grid carved by depth frames, the three-state map and its frontier ----
 * The occupied set and its field say where surfaces are; they cannot tell a voxel the sensor has seen through from one it has
 * never observed.  dsm_grid_carve answers "which voxels of this grid does this depth frame see through?" for the frames in the
 * handle's frame slots.  It is defined PER VOXEL, so no order of execution matters; fp32, non-fused, in the order written:
 *   1. c = the voxel's centre (c_a = origin_a + ((float)i + 0.5f) * voxel, as for the grid).
 *   2. q = inv c, with inv the world -> camera matrix: the caller's pose_inv16 bit for bit, or, with NULL, the closed-form inverse
 *      of pose16 (the rule of dsm_render_compose); q_i = ((inv[i] cx + inv[4 + i] cy) + inv[8 + i] cz) + inv[12 + i].
 *   3. unless near_dist < q.z && q.z < far_dist (the carve's own range; a NaN fails): not carved.
 *   4. u = int((q.x * fx) / q.z + cx + 0.5) (in double after the fp32 sum, as the fuse rounds to a pixel), v likewise with fy, cy;
 *      unless 0 <= u < width && 0 <= v < height: not carved.  The camera is the handle's; a pad column is never read.
 *   5. d = depth[v][u]; unless d > 0 (a NaN fails): not carved.  d == +inf: not carved, unless DSM_CARVE_TRUST_INFINITE is given
 *      (a zero disparity then frees the whole range along that ray).
 *   6. FREE iff (q.z + margin) < d.
 * Two limits, stated plainly.  (a) The voxel is CENTRE-SAMPLED: one ray, the one through its centre, decides.  A voxel whose
 * centre projects outside the image or onto a pixel without a measurement stays as it was however much of its volume other pixels
 * see through; the margin (metres kept clear in front of the measured surface) is what keeps the voxels holding the surface itself
 * from being freed, so it should not be smaller than a voxel diagonal.  (b) The set is only as good as the poses it was carved
 * with: a caller that moves its map (a loop closure) has to clear the set and carve again. */
#define DSM_CARVE_MAX_FRAMES 32
#define DSM_CARVE_REPLACE 1u        /* the old contents of the set are ignored instead of OR-ed in */
#define DSM_CARVE_TRUST_INFINITE 2u /* a depth of +inf is a measurement: nothing within far_dist */
typedef struct dsm_carve_params {
    uint32_t struct_size; /* sizeof(dsm_carve_params) */
    float near_dist;      /* 0 < near_dist < far_dist, finite */
    float far_dist;
    float margin;         /* >= 0, finite: metres of clearance kept in front of the measured surface */
} dsm_carve_params;
/* near_dist 0.1 m, far_dist 10 m, margin 0.1732051 m = one voxel diagonal of a 0.1 m grid */
void dsm_carve_params_init(dsm_carve_params *p);
/* free_device |= the union over the n_frames frames of FREE (with DSM_CARVE_REPLACE: free_device = that union).  free_device:
 * [nz][ny][wx] words in DEVICE memory, read and written; pad bits (x >= nx) are written 0.  slots[i]: the frame slot of frame i,
 * poses16 + 16 i its cam -> world matrix, poses_inv16 + 16 i (poses_inv16 may be NULL) its inverse.  *n_free (may be NULL) = the
 * population count of the set after the call.  All frames are tested inside one pass over the set.  Checked before any device work
 * (DSM_E_INVALID, nothing written): what dsm_grid_compose checks of the spec (inflate is validated and unused), a wrong
 * struct_size, near_dist / far_dist / margin out of range or not finite, a pose entry that is not finite, a slot outside the
 * handle's, n_frames outside 1..32, a NULL or not 4-byte aligned set, unknown flags.  Ordered and synchronised like
 * dsm_grid_inflate, and behind the handle's work so far, the uploads and fuses that touch the slots included.  Synchronises. */
int dsm_grid_carve(dsm_handle *h, const dsm_grid_spec *spec, const dsm_carve_params *params, uint32_t flags, int32_t n_frames,
                   const int32_t *slots, const float *poses16, const float *poses_inv16, void *free_device, int64_t *n_free);

#define DSM_SPACE_UNKNOWN 0
#define DSM_SPACE_FREE 1
#define DSM_SPACE_OCCUPIED 2
/* device memory; any may be NULL (not written), not all; no two the same memory; the word planes and cells 4-byte aligned */
typedef struct dsm_space_planes {
    uint8_t *state;       /* [nz][ny][nx]  DSM_SPACE_UNKNOWN / _FREE / _OCCUPIED; occupied wins over free */
    uint32_t *known_free; /* [nz][ny][wx]  free & ~occupied; pad bits 0 */
    uint32_t *frontier;   /* [nz][ny][wx]  the known-free voxels with at least one of the six face neighbours INSIDE the grid
                                           unknown; pad bits 0 */
    int32_t *cells;       /* [cells_cap]   the linear indices (z ny + y) nx + x of the frontier voxels, ascending */
    int32_t cells_cap;    /* >= 0 when cells is not NULL */
} dsm_space_planes;
/* The three states and the frontier of two bit sets in DEVICE memory: `occupied` (dsm_grid_compose's) and `free` (carved), both
 * [nz][ny][wx], pad bits ignored.  Outside the grid nothing is unknown: the grid's own border makes no frontier.  *n_frontier =
 * the number of frontier voxels, whichever planes are asked for.  More than cells_cap: DSM_E_CAPACITY with *n_frontier = the
 * count needed; the other planes are complete and nothing is written past the cap.  DSM_E_INVALID before any device work: a NULL
 * handle, source, planes or n_frontier, a dimension < 1, more than 2^28 voxels, all planes NULL, two planes the same pointer, a
 * plane overlapping a source, a source, word plane or cells not 4-byte aligned, cells with cells_cap < 0.  Ordered and
 * synchronised like dsm_grid_inflate.  Synchronises. */
int dsm_grid_classify(dsm_handle *h, int32_t nx, int32_t ny, int32_t nz, const void *occupied_device, const void *free_device,
                      const dsm_space_planes *planes_device, int32_t *n_frontier);

/* ---- connected components of a bit set: frontier clusters, obstacles as objects, the pocket of free space a robot sits in ----
 * Input: a bit set S in the grid layout ([nz][ny][wx] words, pad bits ignored) and a connectivity.  Two set voxels are ADJACENT
 * when both lie inside the grid and their offset (dx, dy, dz) is not zero with |dx| + |dy| + |dz| == 1 (DSM_CONNECT_FACES) or
 * max(|dx|, |dy|, |dz|) == 1 (DSM_CONNECT_ALL).  A component is a class of the transitive closure of adjacency; nothing outside the
 * grid connects anything.  A component is NAMED by the lowest linear index lin = (z ny + y) nx + x of its voxels, its root.  Every
 * output is an integer minimum, maximum, sum or count over a set: the result does not depend on how the GPU arranges the work and
 * is reproducible bit for bit.
 * Not provided: clusters tracked from one call to the next, pose search (dsm_grid_view below scores the poses a caller proposes),
 * 18-connectivity, a component's voxel list. */
#define DSM_CONNECT_FACES 6
#define DSM_CONNECT_ALL 26
typedef struct dsm_component { /* 64 bytes */
    int32_t root;         /* the lowest linear index of the component */
    int32_t count;        /* its voxels */
    int64_t sum[3];       /* the sums of the x, y, z voxel indices: centroid_a = origin_a + (sum_a / count + 0.5) voxel, the caller's division */
    int32_t lo[3], hi[3]; /* the inclusive bounding box in voxel indices */
    int32_t tag;          /* tag_src[root] when a tag plane is given, else 0 */
    int32_t reserved;     /* 0 */
} dsm_component;
/* device memory; either may be NULL (not written), not both; label 4-byte and table 8-byte aligned */
typedef struct dsm_component_planes {
    int32_t *label;       /* [nz][ny][nx]  the root of the voxel's component; -1 for a voxel not in S.  Never filtered. */
    dsm_component *table; /* [table_cap]   the components with count >= min_count, ascending by root */
    int32_t table_cap;    /* >= 0 when table is not NULL */
} dsm_component_planes;
/* The components of a bit set in DEVICE memory.  tag_src_device: an int32 [nz][ny][nx] plane in device memory or NULL.
 * *n_components = the components with count >= min_count, *n_all (may be NULL) = all of them, whichever planes are asked for.
 * More than table_cap pass the filter: DSM_E_CAPACITY with *n_components = the count needed; `label` is complete, the first
 * table_cap entries are complete, and nothing is written past the cap.  The intermediates cost up to 8 bytes a voxel of grow-only
 * handle scratch, hence the limit of 2^26 voxels.  DSM_E_INVALID before any device work, nothing written: a NULL handle, source,
 * planes or n_components; a dimension < 1; more than 2^26 voxels; a connectivity other than 6 or 26; min_count < 1; both outputs
 * NULL; table with table_cap < 0; the two outputs the same pointer; an output overlapping the source or the tag plane; the
 * source, the tag plane or `label` not 4-byte aligned, `table` not 8-byte aligned.  Ordered and synchronised like dsm_grid_inflate.
 * Synchronises. */
int dsm_grid_components(dsm_handle *h, int32_t nx, int32_t ny, int32_t nz, int32_t connectivity, int32_t min_count, const void *src_device,
                        const int32_t *tag_src_device, const dsm_component_planes *planes_device, int32_t *n_components, int32_t *n_all);

/* ---- viewpoint gain: what a camera at a candidate pose would see of the grid (no counterpart in the reference) ----
 * Inputs: a grid spec (inflate is validated and unused); two bit sets in DEVICE memory in the grid layout ([nz][ny][wx] words, pad
 * bits ignored), `occupied` and `free`; optionally a third, `target` (the frontier of dsm_grid_classify, a cluster the caller
 * painted); a view camera (dsm_render_camera: independent of the handle's frame size, so a planner can use a coarse sensor
 * model); n_poses candidate poses, cam -> world, 16 column-major floats each, with optional inverses under the *_inv rule (NULL =
 * the closed-form inverse, as for dsm_grid_carve).  The outcome is defined PER POSE AND PER VOXEL, so no order of execution matters.
 *   IN VIEW    steps 1-4 of the carve's definition above with the view camera in place of the handle's: c = the voxel's centre,
 *              q = inv c evaluated exactly as there; in view iff near_dist < q.z && q.z < far_dist (a NaN fails) and the rounded
 *              pixel satisfies 0 <= u < width && 0 <= v < height.  fp32, non-fused, in that order (the code is shared).
 *   THE CAMERA'S VOXEL   a_i = floor(((double)pose16[12 + i] - origin_i) / voxel), in double on the host.  The call is refused unless
 *              -DSM_VIEW_MAX_REACH <= a_i < n_i + DSM_VIEW_MAX_REACH on every axis: this bounds the length of every line, and so
 *              the work of the call, without reference to the data.
 *   THE LINE   to voxel v: d = v - a (integers), n = max(|dx|, |dy|, |dz|); the interior points are p_k = a + floor((2 k d + n) /
 *              (2 n)) per axis for k = 1 .. n - 1 -- the mathematical floor, not C truncation, defined in int64.  Both end voxels
 *              are excluded: the camera's own voxel never blocks, a voxel never blocks itself, and with n <= 1 there is no
 *              interior.  This is k d / n rounded half up: the line is the same walked from either end, and consecutive points are
 *              26-adjacent.
 *   BLOCKED    iff some interior point that lies inside the grid is a blocker: a voxel of `occupied`, or, with
 *              DSM_VIEW_UNKNOWN_BLOCKS, any voxel that is not known free (free & ~occupied).  Outside the grid nothing blocks.
 *   VISIBLE    in view and not blocked.
 * Every output is a count or an OR over a set: reproducible bit for bit.
 * Limits, stated plainly.  (1) Centre-sampled, as the carve is: one ray per voxel.  (2) The line is 26-connected, so a blocker set
 * that is itself only 26-connected leaks: in a numpy trial a one-voxel diagonal sheet let 41 % of the voxels behind it through.
 * (3) dsm_grid_compose's own cover of a surfel disc passes e2 <= (h l1)^2, a plane of thickness |n|_1, which has no such tunnels:
 * in the same trial random planes covered by that test were crossed by 10 456 random lines with no leak -- a measurement, not a
 * proof.  (4) The remedy for caller-made sets is to pass the set inflated by 1 (dsm_grid_inflate).  (5) Not provided: a gain
 * weighted by distance or by pixel footprint, viewpoint sampling or pose search, occlusion by anything outside the grid. */
#define DSM_VIEW_MAX_REACH 4096
#define DSM_VIEW_MAX_POSES 4096
#define DSM_VIEW_UNKNOWN_BLOCKS 1u /* a blocker is any voxel that is not known free, instead of any occupied voxel */
typedef struct dsm_view_score { /* 32 bytes, per pose */
    int32_t in_view;            /* voxels in view */
    int32_t visible;            /* ... and not blocked */
    int32_t unknown;            /* the visible voxels by state (DSM_SPACE_*; occupied wins over free): unknown + free + occupied == visible */
    int32_t free;
    int32_t occupied;
    int32_t target;             /* visible voxels of the target set; 0 without one */
    int32_t reserved[2];        /* 0 */
} dsm_view_score;
/* scores: [n_poses] in host memory, or in device memory with scores_on_device (4-byte aligned), or NULL.  visible_device: NULL or
 * [n_poses][nz][ny][wx] words in DEVICE memory, the visible set of every pose, pad bits 0.  target_device may be NULL.  At most
 * 2^28 voxels, n_poses 1 .. DSM_VIEW_MAX_POSES.  DSM_E_INVALID before any device work, nothing written: what dsm_grid_carve checks
 * of the spec and the poses; what dsm_render_compose checks of the camera; the reach rule; a NULL spec, camera, poses or source; a
 * device pointer not 4-byte aligned; an output overlapping a source or the other output; unknown flags; scores and visible_device
 * both NULL.  Ordered and synchronised like dsm_grid_classify.  Synchronises. */
int dsm_grid_view(dsm_handle *h, const dsm_grid_spec *spec, const dsm_render_camera *camera, uint32_t flags, int32_t n_poses,
                  const float *poses16, const float *poses_inv16, const void *occupied_device, const void *free_device,
                  const void *target_device, dsm_view_score *scores, int scores_on_device, uint32_t *visible_device);

/* ---- a depth frame against the map: projective association and point-to-plane alignment (no counterpart in the reference) ----
 * What dsm_render_compose predicts for a camera (the MODEL camera: depth plane Zm, camera-frame normal plane Nm) is compared with
 * the depth plane of a frame slot, whichever upload wrote it.  T is a rigid transform from the frame camera to the model camera,
 * 16 column-major floats.  One EVALUATION visits the frame pixels (u, v) with u % stride == 0 and v % stride == 0 (never a pad
 * column); fp32, non-fused, in the order written:
 *   1. d = depth[v][u]; skip unless near_dist < d < far_dist (the handle's; d finite)
 *   2. p = (((u - cx) / fx) d, ((v - cy) / fy) d, d)              3. q = R p + t as ((a0 x + a1 y) + a2 z) + a3
 *   4. skip unless near_m < q.z < far_m and |q|^2 <= qmax^2, qmax = far_m times the length of the most oblique ray one pixel
 *      outside the model image
 *   5. um = int((q.x fx_m) / q.z + cx_m + 0.5), vm likewise (the + 0.5 in double, truncating: the fuse kernel's rounding); skip
 *      unless inside the model image          6. zm = Zm[vm][um]; skip unless zm > 0
 *   7. n = Nm[vm][um]; skip unless 0.5 <= |n|^2 <= 2
 *   8. pm = (((um - cx_m) / fx_m) zm, ((vm - cy_m) / fy_m) zm, zm), e = q - pm; skip unless |e|^2 <= dist_max^2
 *   9. skip unless (n . q)^2 >= min_view_cos^2 |q|^2
 *  10. in double, from those floats: r = n . e, J = (n, q x n), w = 1 or, with huber > 0, w = |r| <= huber ? 1 : huber / |r|
 * and adds to 29 sums: the 21 upper-triangle entries of w J J^T row by row, the 6 of w J r, w r^2, and the count.  Every term
 * but the count enters as llrint(term * 2^scale_log2) (round to nearest even) into an int64: integer addition is associative, so
 * the sums are the same bits whatever the launch geometry and the order of the atomics.  scale_log2 is the largest value <= 40
 * for which no sum can leave int64 for this model camera and this many sampled pixels (csrc/dsm_align.h derives the bound); a
 * camera that leaves less than 10 is refused.
 * The LOOP (dsm_align_frame) renders the map at pose16_guess once, starts from T = I and repeats: evaluate; fewer than min_pixels
 * pixels: TOO_FEW; solve A xi = -b (double, LDL^T in a fixed order; a pivot not > 1e-9 trace(A): SINGULAR), xi = (v, omega);
 * T <- [Rodrigues(omega) R, Rodrigues(omega) t + v] (kept in double, cast to float for each evaluation); |v| < stop_translation and
 * |omega| < stop_rotation: CONVERGED; max_iterations steps taken: MAX_ITERATIONS.  One last evaluation at the final estimate gives
 * n_pixels, rms = sqrt(sum w r^2 / count) and the sums reported.  pose16 = pose16_guess . T, a double product cast to float. */
typedef enum {
    DSM_ALIGN_CONVERGED = 0,
    DSM_ALIGN_MAX_ITERATIONS = 1,
    DSM_ALIGN_TOO_FEW = 2,
    DSM_ALIGN_SINGULAR = 3
} dsm_align_status;
typedef struct dsm_align_params {
    uint32_t struct_size;   /* sizeof(dsm_align_params) */
    int32_t max_iterations; /* >= 1; default 10 */
    int32_t stride;         /* >= 1; default 2: a quarter of the pixels */
    float dist_max;         /* metres, in (0, qmax]; default 0.25 */
    float min_view_cos;     /* in [0, 1]; default 0.2 */
    float huber;            /* metres, >= 0, 0 = every weight 1; default 0.05 */
    int32_t min_pixels;     /* default 200 */
    float stop_translation; /* metres; default 1e-4 */
    float stop_rotation;    /* radians; default 1e-4 */
} dsm_align_params;
#define DSM_ALIGN_SUMS 29
typedef struct dsm_align_result {
    float pose16[16];  /* the refined cam -> world pose */
    float T16[16];     /* the correction: frame camera -> the camera at pose16_guess */
    int32_t status;    /* dsm_align_status */
    int32_t iterations; /* steps taken */
    int32_t n_pixels;  /* pixels that passed in the last evaluation */
    int32_t scale_log2;
    double rms;        /* of the last evaluation; 0 when n_pixels is 0 */
    int64_t sums[DSM_ALIGN_SUMS]; /* of the last evaluation */
} dsm_align_result;
void dsm_align_params_init(dsm_align_params *p);
/* One evaluation against the caller's DEVICE planes (model_depth_dev [height][width] floats, model_normal_dev [height][width][3],
 * tight, as dsm_render_compose writes them for model_cam), read behind the work enqueued on the null stream so far.  The 29
 * device words are cleared on the handle's stream before every evaluation and come back through page-locked memory.
 * Checked before any device work (DSM_E_INVALID, outputs untouched): slot out of range, a camera dsm_render_compose would refuse
 * or one that leaves scale_log2 < 10, a non-finite T16 entry, struct_size, stride < 1, dist_max not in (0, qmax], min_view_cos
 * outside [0, 1], huber negative or not finite, max_iterations < 1.  Synchronises. */
int dsm_align_equations(dsm_handle *h, int slot, const dsm_render_camera *model_cam, const void *model_depth_dev, const void *model_normal_dev,
                        const float *T16, const dsm_align_params *params, int64_t *sums /* 29 */, int32_t *scale_log2);
/* The loop, against the surfel sequence of dsm_render_compose(select, runs) rendered at pose16_guess (two-sided, the closed-form
 * inverse) into scratch of the handle (allocated at the first call).  model_cam NULL = the handle's camera and fuse distances.
 * The checks of dsm_align_equations and of dsm_render_compose (run bounds, non-finite pose) come before any device work; *result
 * is written only on DSM_OK.  The map, the store and the frame are not changed.  Synchronises. */
int dsm_align_frame(dsm_handle *h, int slot, int select, int32_t n_segments, const int32_t *store_begin, const int32_t *store_count,
                    const dsm_render_camera *model_cam, const float *pose16_guess, const dsm_align_params *params, dsm_align_result *result);

/* Copy a frame into frame slot `slot` (0 .. frame_slots-1 of the config) and return when it is there (the host
 * buffers may be reused).  By default the copy is ordered behind everything enqueued so far.  With
 * DSM_FLAG_UPLOAD_STREAM it runs on the handle's upload stream instead: it waits only for the enqueued frames that
 * still read this slot and overlaps frames in flight on OTHER slots -- alternate two slots to upload frame t+1
 * while frame t is fused. */
int dsm_frame_upload(dsm_handle *h, int slot, const uint8_t *image, size_t img_step, const float *depth,
                     size_t depth_step);
/* same, sources already in device memory (the caller makes sure they have been written) */
int dsm_frame_upload_device(dsm_handle *h, int slot, const void *image_dev, size_t img_step,
                            const void *depth_dev, size_t depth_step);

/* ---- streamed input: frames of a replay arrive from host memory while earlier frames are being fused (the reference
 * receives every frame through image_input / depth_input, surfel_map.cpp:83-101).  dsm_frame_upload_async returns at once:
 * the copy runs on the device's upload stream, ordered behind the frames enqueued so far that may still read the slots it
 * writes -- the newest dsm_replay_enqueue call that reads one of them (the last four calls are kept apart by the slots they
 * read); behind EVERYTHING enqueued so far for the handle if frames were enqueued any other way (frame by frame, through a
 * batch) since its last upload -- and a frame enqueued AFTER the call, alone or through a batch, waits for it if it reads
 * one of the slots it writes (the last four uploads of a handle are kept apart by slot range; older ones count as one).
 * So a replay buffers in chunks: upload chunk k+1, THEN enqueue chunk k -- chunk k waits for upload k only, and upload k+1
 * runs beside its kernels.  With two groups of slots upload k+1 waits for chunk k-1, whose slots it overwrites; with three
 * in turn it waits for chunk k-2, which finished long ago, and never holds up the hardware queue it shares with the handle's
 * own streams (densesurfelmapping_amd/replay.py: 13-14 k instead of 11 k frames/s for one sequence at 1226x370).  The source must be page-locked (dsm_host_alloc) and stay untouched until
 * dsm_frame_uploads_wait (or dsm_synchronize after a frame that reads the slot).  Rows laid out with the slot pitch
 * (dsm_frame_pitch elements per row: img_step = pitch, depth_step = 4 * pitch; the pad columns are never read) go up
 * as one transfer per plane, any other step row by row. ---- */
int dsm_frame_pitch(const dsm_handle *h, int32_t *pitch);
int dsm_frame_upload_async(dsm_handle *h, int slot, const uint8_t *image, size_t img_step, const float *depth,
                           size_t depth_step);
/* n frames into slots slot0 .. slot0+n-1: frame i at image + i * img_frame_step / depth + i * depth_frame_step (bytes).
 * Frames laid out back to back exactly like the slots (row steps = the pitch, frame steps = pitch * height elements) go
 * up as ONE transfer per plane for all n -- a replay that keeps its frames in that layout pays two transfers per chunk
 * instead of two per frame.  TIGHT rows (row steps = width elements, frames back to back) are taken too: one transfer per
 * plane into a staging buffer of the handle (allocated at the first such call: that call waits for the upload stream) and
 * a kernel that sets the rows to the slots' pitch -- 4.4 % fewer bytes over the link at 1226 pixels, yet measured SLOWER than
 * the pitched layout (the kernel sits between two transfers of its stream); any other layout goes row by row. */
int dsm_frames_upload_async(dsm_handle *h, int slot0, int n, const uint8_t *image, size_t img_step, size_t img_frame_step,
                            const float *depth, size_t depth_step, size_t depth_frame_step);
int dsm_frame_uploads_wait(dsm_handle *h); /* blocks the host until this handle's asynchronous uploads have landed */

/* ---- sensor-native depth: the frame's depth as uint16 (TUM RGB-D PNGs, ROS 16UC1, KITTI-style PNGs), converted to float
 * metres on the device.  depth_op DSM_DEPTH_U16_DIVIDE: d = (float)u / depth_scale, an IEEE fp32 divide (numpy's
 * u16.astype(np.float32) / np.float32(scale): TUM 5000, KITTI 256, 1 = the plain value); DSM_DEPTH_U16_MULTIPLY:
 * d = (float)u * depth_scale, an fp32 multiply (depth_image_proc's depth * 0.001f for millimetres).  0 stays 0 (invalid).
 * depth_scale must be finite and > 0, depth_op one of the two, depth steps are in BYTES (>= 2 * width); anything else is
 * DSM_E_INVALID before any device work.  The slot's float depth plane then holds exactly what the float upload of the
 * host-converted frame would have written, so every kernel downstream is unchanged.  The u16 rows go up into a staging plane
 * of the slot (pitch * height * 2 bytes per slot, allocated at the handle's first u16 call) and one kernel per call converts
 * them into the slot, on the stream of the copy, before whatever says the upload has landed.  Rows at the slot pitch
 * (depth_step = 2 * dsm_frame_pitch) are the fast layout; tight rows (2 * width) are taken too. ---- */
#define DSM_DEPTH_U16_DIVIDE 0
#define DSM_DEPTH_U16_MULTIPLY 1
/* dsm_frame_upload with u16 depth: synchronous, on the upload stream with DSM_FLAG_UPLOAD_STREAM */
int dsm_frame_upload_u16(dsm_handle *h, int slot, const uint8_t *image, size_t img_step, const uint16_t *depth, size_t depth_step,
                         float depth_scale, int32_t depth_op);
/* dsm_frame_upload_device with u16 depth (device memory; the kernel reads it in place when the pointer and step are even) */
int dsm_frame_upload_device_u16(dsm_handle *h, int slot, const void *image_dev, size_t img_step, const void *depth_dev, size_t depth_step,
                                float depth_scale, int32_t depth_op);
/* dsm_frame(s)_upload_async with u16 depth: the same slot-ordering contract, the upload's event is recorded behind the conversion */
int dsm_frame_upload_async_u16(dsm_handle *h, int slot, const uint8_t *image, size_t img_step, const uint16_t *depth, size_t depth_step,
                               float depth_scale, int32_t depth_op);
int dsm_frames_upload_async_u16(dsm_handle *h, int slot0, int n, const uint8_t *image, size_t img_step, size_t img_frame_step,
                                const uint16_t *depth, size_t depth_step, size_t depth_frame_step, float depth_scale, int32_t depth_op);
/* dsm_replay_enqueue_host with u16 depth: each group's depth is converted on the stream that runs its superpixel stages, right
 * behind its copy.  Frame f still goes to slot f mod pipeline_depth, overwriting what that slot held, as in the float form. */
int dsm_replay_enqueue_host_u16(dsm_handle *h, int32_t n, const uint8_t *image, size_t img_step, size_t img_frame_step, const uint16_t *depth,
                                size_t depth_step, size_t depth_frame_step, const int32_t *ref_idx, const float *poses16,
                                const float *inv_poses16 /* may be NULL */, float depth_scale, int32_t depth_op);
/* dsm_host_pack_frames with u16 depth planes (copied as they are: the conversion happens on the device) */
int dsm_host_pack_frames_u16(int32_t n, int32_t width, int32_t height, const uint8_t *const *images, const size_t *image_steps,
                             const uint16_t *const *depths, const size_t *depth_steps, uint8_t *dst_image, size_t dst_img_step,
                             size_t dst_img_frame_step, uint16_t *dst_depth, size_t dst_depth_step, size_t dst_depth_frame_step);

/* ---- colour camera images, and one descriptor for both halves of a sensor's frame.  The reference takes whatever encoding the
 * camera driver publishes: SurfelMap::image_input runs cv_bridge::toCvCopy(msg, MONO8) (surfel_map.cpp:86), which for rgb8 / bgr8 /
 * rgba8 / bgra8 is OpenCV's 8-bit colour-to-grey -- a fixed-point weighted sum, computed here on the device in exact integer
 * arithmetic (alpha is ignored):
 *     grey = (R * gray_wr + G * gray_wg + B * gray_wb + (1 << (gray_shift - 1))) >> gray_shift
 * The weights are an input because cv_bridge's result depends on the OpenCV it was built with (as the pose inverse depends on the
 * caller's Eigen).  The presets restate OpenCV's and Pillow's constants; the two OpenCV rows are written from OpenCV's source as
 * remembered, including which version uses which, and are NOT checked against an OpenCV build; the Pillow
 * row is checked against Pillow by the test suite.  A caller with another OpenCV passes its own weights.
 * Rules (DSM_E_INVALID before any device work): struct_size == sizeof(dsm_frame_format); image_format and depth_format known; for a
 * colour format weights >= 0, 1 <= gray_shift <= 22 and gray_wr + gray_wg + gray_wb <= 1 << gray_shift (the result stays <= 255 and
 * the sum inside int32: no saturation); for DSM_DEPTH_U16 the rules of the *_u16 calls; image step in BYTES >= channels * width,
 * depth step in bytes >= 4 (2) * width.  mono8 + f32 does exactly what the plain calls do, mono8 + u16 what the *_u16 calls do.
 * Colour rows go up into a staging area of the handle (4 * pitch * height bytes per slot, allocated at the handle's first colour
 * call) and ONE kernel per call writes the grey bytes of the w pixels of each row into the slots' image planes, on the stream of
 * the copy, before whatever says the upload has landed.  Rows at the slot pitch (img_step = channels * dsm_frame_pitch) are the
 * fast layout; tight rows (channels * width) are taken too, any other step goes row by row; a device pointer is read in place. ---- */
#define DSM_IMAGE_MONO8 0
#define DSM_IMAGE_RGB8 1
#define DSM_IMAGE_BGR8 2
#define DSM_IMAGE_RGBA8 3
#define DSM_IMAGE_BGRA8 4
#define DSM_DEPTH_F32 0
#define DSM_DEPTH_U16 1
/* gray_wr, gray_wg, gray_wb, gray_shift (initialisers of an int32_t[4]) */
#define DSM_GRAY_OPENCV_14BIT {4899, 9617, 1868, 14}   /* OpenCV 2.4 / 3.x RGB2Gray<uchar>: R2Y, G2Y, B2Y, yuv_shift, CV_DESCALE (ROS Kinetic / Melodic: the reference's era); the default */
#define DSM_GRAY_OPENCV_15BIT {9798, 19235, 3735, 15}  /* OpenCV 4.x 8-bit path */
#define DSM_GRAY_PIL_L {19595, 38470, 7471, 16}        /* Pillow's convert("L") */
typedef struct dsm_frame_format {
    uint32_t struct_size;   /* sizeof(dsm_frame_format) */
    int32_t image_format;   /* DSM_IMAGE_MONO8, _RGB8, _BGR8, _RGBA8, _BGRA8 */
    int32_t gray_wr, gray_wg, gray_wb, gray_shift;
    int32_t depth_format;   /* DSM_DEPTH_F32, DSM_DEPTH_U16 */
    float depth_scale;      /* DSM_DEPTH_U16: as the *_u16 calls */
    int32_t depth_op;
} dsm_frame_format;
/* mono8 + f32, DSM_GRAY_OPENCV_14BIT, depth_scale 1 / DSM_DEPTH_U16_DIVIDE */
void dsm_frame_format_init(dsm_frame_format *f);
/* the *_u16 calls' signatures with `const void *` planes, steps in bytes and the format in place of (scale, op) */
int dsm_frame_upload_fmt(dsm_handle *h, int slot, const void *image, size_t img_step, const void *depth, size_t depth_step,
                         const dsm_frame_format *fmt);
int dsm_frame_upload_device_fmt(dsm_handle *h, int slot, const void *image_dev, size_t img_step, const void *depth_dev, size_t depth_step,
                                const dsm_frame_format *fmt);
int dsm_frame_upload_async_fmt(dsm_handle *h, int slot, const void *image, size_t img_step, const void *depth, size_t depth_step,
                               const dsm_frame_format *fmt);
int dsm_frames_upload_async_fmt(dsm_handle *h, int slot0, int n, const void *image, size_t img_step, size_t img_frame_step,
                                const void *depth, size_t depth_step, size_t depth_frame_step, const dsm_frame_format *fmt);
/* each group's colour rows are converted on the stream that runs its superpixel stages, right behind their copy */
int dsm_replay_enqueue_host_fmt(dsm_handle *h, int32_t n, const void *image, size_t img_step, size_t img_frame_step, const void *depth,
                                size_t depth_step, size_t depth_frame_step, const int32_t *ref_idx, const float *poses16,
                                const float *inv_poses16 /* may be NULL */, const dsm_frame_format *fmt);
/* dsm_host_pack_frames for any format: the planes are copied as they are (channels * width image bytes and 4 or 2 * width depth
 * bytes of each row); the weights are not looked at */
int dsm_host_pack_frames_fmt(int32_t n, int32_t width, int32_t height, const void *const *images, const size_t *image_steps,
                             const void *const *depths, const size_t *depth_steps, void *dst_image, size_t dst_img_step,
                             size_t dst_img_frame_step, void *dst_depth, size_t dst_depth_step, size_t dst_depth_frame_step,
                             const dsm_frame_format *fmt);

/* debug tap: the planes of frame slot `slot` as the kernels read them, tight rows (image: height * width bytes, depth: height *
 * width floats); either output may be NULL.  Comes behind everything enqueued for the handle and the uploads that wrote the slot
 * (synchronises). */
int dsm_debug_get_frame(dsm_handle *h, int slot, uint8_t *image, float *depth);
/* debug tap: the WHOLE planes of frame slot `slot`, rows dsm_frame_pitch elements apart with their pad columns (image: pitch * height
 * bytes, depth: pitch * height floats; either may be NULL), read -- or, with write != 0, overwritten: a test fills a slot with a
 * pattern, uploads, and looks at what the upload left alone.  Ordered like dsm_debug_get_frame (synchronises). */
int dsm_debug_frame_planes(dsm_handle *h, int slot, int write, uint8_t *image, float *depth);

/* enqueue SurfelMap::fuse_map for the frame in `slot` against the resident map */
int dsm_fuse_frame_resident(dsm_handle *h, int slot, int reference_frame_index, const float *pose16);
/* enqueue n frames: frame i uses slots[i], ref_idx[i], poses16[16*i .. 16*i+16) */
int dsm_replay_enqueue(dsm_handle *h, int32_t n, const int32_t *slots, const int32_t *ref_idx,
                       const float *poses16);
/* the same with the caller's own pose inverses (see dsm_fuse_map_inv); inv_pose(s)16 may be NULL */
int dsm_fuse_frame_resident_inv(dsm_handle *h, int slot, int reference_frame_index, const float *pose16,
                                const float *inv_pose16);
int dsm_replay_enqueue_inv(dsm_handle *h, int32_t n, const int32_t *slots, const int32_t *ref_idx,
                           const float *poses16, const float *inv_poses16);
/* The same with the frames COMING WITH THE CALL (round 6): n frames in page-locked host memory (dsm_host_alloc), frame i at
 * image + i * img_frame_step / depth + i * depth_frame_step, rows img_step / depth_step bytes apart (rows at the frame slots' own
 * pitch -- dsm_frame_pitch elements -- and frames one slot apart go up as one transfer per plane and group of frames).  What a
 * replay of a log does (the reference receives every frame through image_input / depth_input, surfel_map.cpp:83-101).  Each
 * group of frames is uploaded ON THE STREAM THAT RUNS ITS SUPERPIXEL STAGES, right in front of them, into the frame slots of the
 * pipelines that take it (frame f -> slot f mod pipeline_depth: the handle needs frame_slots >= pipeline_depth, and whatever
 * those slots held is overwritten): no upload stream and no event between a transfer and its consumer, the transfer of one
 * group runs beside the kernels of the groups before it, and nothing is waited for on the host.  The host memory of a call
 * may be rewritten once dsm_replay_wait says the call's frames are done. */
int dsm_replay_enqueue_host(dsm_handle *h, int32_t n, const uint8_t *image, size_t img_step, size_t img_frame_step, const float *depth,
                            size_t depth_step, size_t depth_frame_step, const int32_t *ref_idx, const float *poses16,
                            const float *inv_poses16 /* may be NULL */);
/* host wait until the frames of the dsm_replay_enqueue_host call `calls_back` calls ago (0 = the latest; < 8) have been fused */
int dsm_replay_wait(dsm_handle *h, int32_t calls_back);
int dsm_synchronize(dsm_handle *h);
/* number of new surfels created by the last completed frame; synchronises */
int dsm_last_new_count(dsm_handle *h, int32_t *n_new);
/* the handle's hipStream_t, for event timing by the caller.  (A handle that advances with a batch: its stream is put behind
 * the batch's work at the handle's next dsm_* call -- this one included -- not after every batch call; fetch the stream after
 * the batch calls whose results the caller's own work on it should come behind.) */
int dsm_stream(dsm_handle *h, void **hip_stream);

/* ---- batches: handles of equal image size on one device, each with its own map and frames (independent subsequences,
 * surfel_map.cpp has no counterpart: it fuses one frame at a time), advancing in LOCKSTEP: every kernel of a frame is
 * launched once for the whole batch (grid z = handle).  Launch overheads, cold caches and the slowest waves of a kernel
 * are shared by all subsequences instead of paid by each: this is what bench.py's headline replays.  Handles must have
 * pipeline_depth 1 and a resident map; they stay usable on their own between batch calls (a handle's stream is ordered
 * behind the batch when it is next used, by every per-handle call and by dsm_batch_synchronize; a batch call itself touches
 * no stream but the batch's own -- the handles' streams share hardware queues with the other batches). ---- */
typedef struct dsm_batch dsm_batch;
/* the handles: pipeline_depth 1, no DSM_FLAG_UPLOAD_STREAM, one device and image size, the same number of frames fused, and
 * all or none with DSM_FLAG_EIGEN33_PRODUCTS; otherwise DSM_E_INVALID (DSM_E_STATE for the frame count) */
int dsm_batch_create(dsm_handle *const *handles, int32_t n, dsm_batch **out);
void dsm_batch_destroy(dsm_batch *b);
const char *dsm_batch_last_error(const dsm_batch *b);
/* enqueue n_frames frames for every handle: frame i of handle j uses slots[j * n_frames + i], ref_idx[...], and
 * poses16[(j * n_frames + i) * 16 ..] */
int dsm_batch_replay_enqueue(dsm_batch *b, int32_t n_frames, const int32_t *slots, const int32_t *ref_idx, const float *poses16);
int dsm_batch_replay_enqueue_inv(dsm_batch *b, int32_t n_frames, const int32_t *slots, const int32_t *ref_idx,
                                 const float *poses16, const float *inv_poses16); /* inv_poses16 laid out like poses16; may be NULL */
/* wait for everything enqueued and report the first handle's error, if any */
int dsm_batch_synchronize(dsm_batch *b);

/* ---- parity taps (state after the last completed frame; synchronise) ------------------- */
int dsm_get_labels(dsm_handle *h, int32_t *out /* height*width */);
int dsm_get_seeds(dsm_handle *h, dsm_seed *out /* (width/8)*(height/8) */);
int dsm_seed_count(const dsm_handle *h);

/* ---- state-level test taps (poke superpixel state, run single stages) ------------------
 * Stage indices are positions in the frame's kernel sequence: 0 init_seeds, 1 assign_0, 2 update_seeds_0,
 * 3 commit_seeds_0, 4 assign_1, 5 resolve_1, 6 update_seeds_1, 7 commit_seeds_1, 8 assign_2, 9 resolve_2,
 * 10 update_seeds_2, 11 commit_seeds_2, 12 seed_points, 13 seed_fit, 14 fuse_surfels, 15 frame_tail.
 * ABI 3 notes for users of these taps:
 *  - there is ONE label image, updated in place from sweep to sweep; `which` = 0 and 1 both name it (the sweeps used to take
 *    turns between two buffers, and old callers pass `sweep & 1`);
 *  - a sweep >= 1 is the PAIR assign_k + resolve_k (stages 4-5 and 8-9): assign rewrites the label image where a pixel's
 *    old superpixel was not stable and leaves the other picks in a side plane; resolve stores those of them that count.
 *    Re-running assign_k alone reads the already updated image and does not reproduce the sweep: inject the pre-sweep
 *    image (dsm_debug_set_label_buffer) and run the pair;
 *  - dsm_debug_set_label_buffer checks the image: every entry a superpixel index of this grid, and -1 exactly at the pixels
 *    beyond every cell's reach (image sizes with (size mod 8) > 4), where the assignment stage itself writes -1 --
 *    DSM_E_INVALID otherwise (the kernels index per-seed arrays with the labels they read). */
int dsm_debug_run_stages(dsm_handle *h, int slot, int reference_frame_index, const float *pose16, int first_stage,
                         int last_stage);
int dsm_debug_get_label_buffer(dsm_handle *h, int which, int32_t *out);
int dsm_debug_set_label_buffer(dsm_handle *h, int which, const int32_t *in);
/* live seed state during the sweeps: core = (x, y, mean_intensity, mean_depth) per seed, stable = 0/1 */
int dsm_debug_get_seed_state(dsm_handle *h, float *core4, int32_t *stable);
int dsm_debug_set_seed_state(dsm_handle *h, const float *core4, const int32_t *stable);

/* debug tap: shader-clock stamps of the phases of the per-seed kernels, [5][n_seed][8] (kernel 0..2 =
 * update_seeds of sweep 0..2, 3 = seed_points, 4 = seed_fit at the first seed of each group of four); needs DSM_FLAG_WAVE_STAMPS in dsm_config.flags */
int dsm_debug_wave_stamps(dsm_handle *h, int64_t *out);

/* test knob: longest point list (<= 120) the short-column tier of the batched plane fit takes; fresh handles only (before the
 * first frame, before dsm_batch_create) */
int dsm_debug_set_fit_small_cap(dsm_handle *h, int32_t cap);

/* debug tap: occupancy of the second tiers of the lane-per-seed kernels (launches batched over >= 8 frames) in the LATEST
 * frame of this handle, counted over the superpixels sweep s recomputes (the ones not stable when it begins) by the length of
 * their depth list -- the member depths above 0.1 inside the statistics window, FF.cpp:508 -- and only where that list holds
 * no +inf (such a superpixel's robust mean is +inf and is finished in place, whatever the length):
 * out[2 s + 0] = lists of 1 to 123 depths whose robust mean (FF.cpp:530-556) needed more than one Huber pass, the first
 * stepping by 0.01 or more; out[2 s + 1] = lists of 124 depths or more, queued for a wave of their own (a lane keeps 123 depths
 * in its LDS row; the spare rows up to 127 only take what a quad adds before the end is clamped); out[6] = groups of four
 * superpixels the plane fit (FF.cpp:128-180) took in its full-length tier, out[7] = 0 (reserved).  All zero after a frame that
 * ran the wave-per-seed kernels.  Both counts are exact: the test suite holds them to a census of the CPU restatement's
 * state per handle, frame and sweep.  Synchronises. */
int dsm_debug_tier_counts(dsm_handle *h, int32_t *out /* 8 */);

/* debug tap: the drop-in calls (dsm_fuse_map / dsm_fuse_initialize_map) bring back only the 64-record groups of the map a frame
 * changed: out[0] = drop-in calls so far, out[1] = of them, calls that took the delta path (the others changed most of the map
 * and took one full download), out[2] = groups those brought back in all, out[3] = groups of the latest call; out[4..7] = host
 * microseconds spent so far in dsm_fuse_map calls on: staging the frame and launching its superpixel stages | comparing the
 * caller's array with the shadow (and uploading it if it differs) | waiting for the GPU | fetching and patching what changed. */
int dsm_debug_dropin_stats(dsm_handle *h, int64_t *out /* 8 */);

/* ---- per-kernel timing (hip events on the handle's stream) ----------------------------- */
#define DSM_MAX_STAGES 32
typedef struct dsm_stage_times {
    int32_t n_stages;
    const char *name[DSM_MAX_STAGES];
    double ms[DSM_MAX_STAGES];      /* accumulated kernel time per stage */
    int64_t launches[DSM_MAX_STAGES];
    int64_t frames;
    double event_overhead_ms;       /* accumulated length of one empty event-to-event interval per frame */
    int64_t sum_new;                /* surfels created, summed over the frames (K of SURVEY.md's B_alg) */
    int64_t sum_local;              /* live map size after each frame, summed over the frames (M) */
} dsm_stage_times;
/* run the resident fuse for n frames eagerly with an event pair around every kernel and
 * accumulate per-stage durations */
int dsm_replay_timed(dsm_handle *h, int32_t n, const int32_t *slots, const int32_t *ref_idx,
                     const float *poses16, dsm_stage_times *out);
/* the same for a batch (arguments as dsm_batch_replay_enqueue): durations are those of the batched launches; `frames`,
 * sum_new and sum_local count handle-frames */
int dsm_batch_replay_timed(dsm_batch *b, int32_t n_frames, const int32_t *slots, const int32_t *ref_idx,
                           const float *poses16, dsm_stage_times *out);

#ifdef __cplusplus
}
#endif
#endif /* DSM_H */
