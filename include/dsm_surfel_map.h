/* dsm_surfel_map.h -- the node-level interface of DenseSurfelMapping's `surfel_fusion` without ROS.
 *
 * Mirrors class SurfelMap (reference surfel_fusion/src/surfel_map.h:48-147): the three callbacks the node
 * wires to its subscribers (ros_node.cpp:24-32) plus save_cloud / save_mesh / save_map, with the ROS
 * message types replaced by plain C structs that carry the same fields the callbacks read.  Everything
 * the callbacks do between the messages and the per-frame engine -- exact-stamp matching
 * (synchronize_msgs, surfel_map.cpp:103-203), the KITTI axis transform and pose-graph bookkeeping
 * (orb_results_input, :205-365), the drift-free window (get_driftfree_poses / get_add_remove_poses,
 * :1597-1673), moving keyframes' surfels between the active map and the inactive set
 * (move_add_surfels, :1456-1595) and the loop-closure deformation (warp_surfels, :681-824) -- is host
 * logic in this library; the surfels themselves never leave HBM: the active map is the resident map of
 * a dsm_handle (include/dsm.h) and the inactive set is its device-side store (dsm_store_*).
 *
 * Point-cloud topics: the five clouds of publish_{active,inactive,all,neighbor,raw}_pointcloud (surfel_map.cpp:1115-1151,
 * 1283-1454) are built on the GPU, bit-identical to the reference's, and either pulled (dsm_surfel_map_get_cloud*) or handed
 * to a callback after every fuse (dsm_surfel_map_set_publish), at the point where the reference publishes (:189-197).
 * Not mirrored: the RViz markers of publish_pose_graph / publish_camera_position (:906-1058) -- read the same data through
 * the taps at the end of this header.
 *
 * Errors: the reference returns void and prints; these return a dsm_status (include/dsm.h) and keep a
 * message for dsm_surfel_map_last_error.  Inputs on which the reference indexes out of range (undefined
 * behaviour) are refused with DSM_E_INVALID instead. */
#ifndef DSM_SURFEL_MAP_H
#define DSM_SURFEL_MAP_H

#include <stddef.h>
#include <stdint.h>

#include "dsm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dsm_surfel_map dsm_surfel_map;

/* ros::Time: toSec() = sec + 1e-9 nsec; stamps are matched by exact equality of that double
 * (surfel_map.cpp:116-139). */
typedef struct dsm_stamp {
    uint32_t sec, nsec;
} dsm_stamp;

/* geometry_msgs::Pose */
typedef struct dsm_pose_msg {
    double px, py, pz;
    double qx, qy, qz, qw;
} dsm_pose_msg;

/* the node's parameters (surfel_map.cpp:13-28) */
typedef struct dsm_surfel_map_config {
    uint32_t struct_size;    /* sizeof(dsm_surfel_map_config) of the caller's header: a caller built against another
                                layout is refused (DSM_E_INVALID) instead of having trailing fields read from garbage */
    int32_t cam_width, cam_height;
    float cam_fx, cam_fy, cam_cx, cam_cy;
    float fuse_far_distence, fuse_near_distence; /* spelling of the reference's parameter names */
    int32_t drift_free_poses;
    int32_t rgbd;            /* constant set of fusion_functions.h:17-21 instead of :7-16 */
    int32_t device;          /* HIP device ordinal */
    int32_t surfel_capacity; /* active-map capacity, 0 = default of dsm_create */
    int32_t max_buffered_frames; /* images / depths kept waiting for a pose, oldest dropped (and reported on stderr)
                                    beyond; 0 = 5000, the depth of the reference's subscriber queues (ros_node.cpp:24-25;
                                    its own lists behind them are unbounded, surfel_map.h:96-97); < 0 = unbounded.  Only the
                                    first 256 waiting frames of each kind sit in page-locked memory, the rest is pageable */
    uint32_t engine_flags;   /* 0 or DSM_FLAG_EIGEN33_PRODUCTS (include/dsm.h): the engine's 3x3 products, and with them the
                                RAW cloud, in Eigen >= 3.3's order; any other bit is refused (DSM_E_INVALID).  A caller built
                                against the header before this field (struct_size ending at max_buffered_frames) reads as 0 */
} dsm_surfel_map_config;

int dsm_surfel_map_create(const dsm_surfel_map_config *cfg, dsm_surfel_map **out); /* SurfelMap::SurfelMap */
void dsm_surfel_map_destroy(dsm_surfel_map *m);
const char *dsm_surfel_map_last_error(const dsm_surfel_map *m);

/* SurfelMap::image_input (surfel_map.cpp:83-91): sensor_msgs/Image already in MONO8 (the reference
 * converts with cv_bridge; other encodings are refused here).  The pixels are copied. */
int dsm_surfel_map_image_input(dsm_surfel_map *m, dsm_stamp stamp, int32_t width, int32_t height, size_t step,
                               const char *encoding, const uint8_t *data);
/* The same for a colour camera's image: rgb8, bgr8, rgba8 or bgra8 (anything else: DSM_E_INVALID), converted to grey on the device
 * as dsm_frame_upload_fmt does -- what the reference's cv_bridge::toCvCopy(msg, MONO8) computes on the host (include/dsm.h:
 * dsm_frame_format).  gray_weights4 = {wr, wg, wb, shift}, NULL = DSM_GRAY_OPENCV_14BIT; they are checked here (weights >= 0,
 * 1 <= shift <= 22, sum <= 1 << shift).  step is in bytes (>= channels * width).  The frame waits for its pose at 3 or 4 bytes a
 * pixel (beyond the page-locked pool: in pageable memory) and goes up together with a depth_input or a depth_input_u16 frame.
 * DSM_E_STATE on an engine without dsm_frame_upload_fmt.  dsm_surfel_map_image_input itself keeps refusing colour. */
int dsm_surfel_map_image_input_color(dsm_surfel_map *m, dsm_stamp stamp, int32_t width, int32_t height, size_t step,
                                     const char *encoding, const void *data, const int32_t *gray_weights4 /* [4], may be NULL */);
/* SurfelMap::depth_input (:93-101): TYPE_32FC1, metres, 0 = invalid. */
int dsm_surfel_map_depth_input(dsm_surfel_map *m, dsm_stamp stamp, int32_t width, int32_t height, size_t step,
                               const char *encoding, const void *data);
/* The same for a sensor's own depth: TYPE_16UC1 (or mono16), converted to metres on the device as dsm_frame_upload_u16 does
 * (include/dsm.h: depth_scale finite > 0, depth_op DSM_DEPTH_U16_DIVIDE or DSM_DEPTH_U16_MULTIPLY; ROS drivers' millimetres:
 * 0.001f, DSM_DEPTH_U16_MULTIPLY).  The frame waits for its pose at 2 bytes a pixel. */
int dsm_surfel_map_depth_input_u16(dsm_surfel_map *m, dsm_stamp stamp, int32_t width, int32_t height, size_t step,
                                   const char *encoding, const uint16_t *data, float depth_scale, int32_t depth_op);
/* SurfelMap::orb_results_input (:205-365).
 *   loop_stamp       header.stamp of the sensor_msgs/PointCloud (it becomes the fuse stamp, :363)
 *   loop_values      channels[0].values: flat pairs of keyframe indices, as float32
 *   loop_path        nav_msgs/Path poses (loop-corrected keyframe poses, SLAM frame)
 *   this_stamp       header.stamp of the nav_msgs/Odometry
 *   this_pose        pose.pose
 *   covariance       pose.covariance: [0] > 0 marks a new keyframe, [1] = reference keyframe index */
int dsm_surfel_map_orb_results_input(dsm_surfel_map *m, dsm_stamp loop_stamp, const float *loop_values,
                                     int32_t n_loop_values, const dsm_pose_msg *loop_path, int32_t n_loop_path,
                                     dsm_stamp this_stamp, const dsm_pose_msg *this_pose, const double *covariance36);

int dsm_surfel_map_save_cloud(dsm_surfel_map *m, const char *path); /* :1153-1174, ASCII PCD of XYZI points */
int dsm_surfel_map_save_mesh(dsm_surfel_map *m, const char *path);  /* :1176-1281, ASCII PLY, one hexagon per surfel */
int dsm_surfel_map_save_map(dsm_surfel_map *m, const char *path);   /* :75-81 = save_mesh */

/* ---- point clouds: 4 floats per point (x, y, z, intensity), the reference's PointXYZI ---- */
typedef enum {
    DSM_CLOUD_ACTIVE = 0,   /* publish_active_pointcloud (:1398-1417): resident surfels with update_times >= 5, map order */
    DSM_CLOUD_INACTIVE = 1, /* publish_inactive_pointcloud (:1385-1396): inactive_pointcloud as it is */
    DSM_CLOUD_ALL = 2,      /* publish_all_pointcloud (:1419-1454): ACTIVE, then INACTIVE */
    DSM_CLOUD_NEIGHBOR = 3, /* publish_neighbor_pointcloud (:1283-1319, method 1): resident surfels with update_times != 0, then
                               the inactive points of the non-local poses of get_driftfree_poses(relative_index, 2 *
                               drift_free_poses), in its breadth-first order */
    DSM_CLOUD_RAW = 4,      /* publish_raw_pointcloud (:1115-1151): the fused frame, cam_width * cam_height points, unfiltered,
                               column-major (point i * cam_height + j = pixel column i, row j), posed with fuse_pose_ros */
    DSM_CLOUD_KINDS = 5
} dsm_cloud_kind;
#define DSM_CLOUD_BIT(kind) (1u << (kind))

/* The cloud of `kind` for the current state; NEIGHBOR and RAW refer to the latest fuse (its relative_index, its frame and
 * fuse_pose_ros).  DSM_E_STATE before the first fuse; more than cap points: DSM_E_CAPACITY with *n = the count needed.
 * Synchronises. */
int dsm_surfel_map_get_cloud(dsm_surfel_map *m, int kind, float *xyzi_out, int32_t cap, int32_t *n);
/* the same into device memory of the node's GPU (e.g. a torch tensor's data_ptr) */
int dsm_surfel_map_get_cloud_device(dsm_surfel_map *m, int kind, void *dst_device, int32_t cap, int32_t *n);

/* What one fuse publishes.  points[k] / n_points[k] for every kind k in the mask (NULL / 0 for the others) are page-locked
 * buffers of the library, valid until the callback returns. */
typedef struct dsm_surfel_map_publication {
    dsm_stamp stamp;          /* fuse_stamp: header.stamp of the clouds */
    int32_t relative_index;   /* the reference keyframe of the fused frame */
    dsm_pose_msg fuse_pose;   /* fuse_pose_ros */
    uint32_t kinds_mask;
    const float *points[DSM_CLOUD_KINDS];
    int32_t n_points[DSM_CLOUD_KINDS];
} dsm_surfel_map_publication;
typedef void (*dsm_surfel_map_publish_fn)(void *user, const dsm_surfel_map_publication *pub);
/* After every fuse (synchronize_msgs, after fuse_map and before the next pose is handled) build the clouds of kinds_mask
 * (DSM_CLOUD_BIT(kind) | ...) and call fn(user, &publication) on the calling thread.  kinds_mask 0 or fn NULL: off (the
 * default; no extra work, no synchronisation). */
int dsm_surfel_map_set_publish(dsm_surfel_map *m, uint32_t kinds_mask, dsm_surfel_map_publish_fn fn, void *user);

/* ---- the hexagon mesh of save_mesh as vertex buffers, built on the GPU (dsm_mesh_compose of dsm.h) ----
 * Six vertices per surfel in `vertex_layout` (dsm_mesh_vertex_layout: 144 or 96 bytes per surfel), in save_mesh's order
 * (:1226-1248): the attached surfels keyframe by keyframe in poses_database order (not store order), then the active surfels
 * with update_times >= 5.  Triangles: dsm_mesh_indices.  DSM_E_STATE before the first fuse; more than cap_surfels:
 * DSM_E_CAPACITY with *n_surfels = the count needed.  Synchronises. */
int dsm_surfel_map_get_mesh(dsm_surfel_map *m, int vertex_layout, void *out, int32_t cap_surfels, int32_t *n_surfels);
/* the same into device memory of the node's GPU (4-byte aligned; 16-byte alignment is faster) */
int dsm_surfel_map_get_mesh_device(dsm_surfel_map *m, int vertex_layout, void *dst_device, int32_t cap_surfels, int32_t *n_surfels);
/* save_mesh's mesh as `format binary_little_endian 1.0`: the same elements and properties as the ASCII file, a vertex = three
 * floats and three uchar (the int colour clamped to 0..255), a face = the uchar 3 and three int.  The vertices come from the
 * GPU in chunks: the attached surfels 256 Ki at a time (24 MiB of page-locked memory at most), the active surfels in ONE piece
 * -- the engine composes the map part whole, so that piece is bounded by the surfel capacity (96 bytes per mature active
 * surfel, on the host and in device staging).  Unlike save_mesh (which returns silently, as the reference does) an unopenable
 * path is DSM_E_INVALID; the file is opened after the last call that can fail without it, and removed if a later one fails. */
int dsm_surfel_map_save_mesh_binary(dsm_surfel_map *m, const char *path);

/* ---- the map as images: what a camera sees of it (dsm_render_compose of dsm.h, where a render is defined) ----
 * kind = DSM_CLOUD_ACTIVE / INACTIVE / ALL / NEIGHBOR: the surfel set of that cloud, as RECORD runs in the mesh's order -- the
 * attached surfels keyframe by keyframe first (ALL, INACTIVE: in poses_database order, so that for ALL surfel number i is
 * surfel i of dsm_surfel_map_get_mesh; NEIGHBOR: the non-local drift-free neighbours in their breadth-first order), then the
 * active surfels (ACTIVE, ALL: update_times >= 5; NEIGHBOR: update_times != 0).  DSM_CLOUD_RAW: DSM_E_INVALID.  camera NULL:
 * the node's own camera and fuse distances.  pose16 (cam -> world, 16 column-major floats) NULL: the pose of the latest fuse --
 * the map's prediction of the frame just fused.  flags: DSM_RENDER_*.  DSM_E_STATE before the first fuse.  Synchronises. */
int dsm_surfel_map_render(dsm_surfel_map *m, int kind, const dsm_render_camera *camera, const float *pose16, uint32_t flags,
                          const dsm_render_planes *planes, int32_t *n_surfels);
/* the same with the planes in device memory of the node's GPU */
int dsm_surfel_map_render_device(dsm_surfel_map *m, int kind, const dsm_render_camera *camera, const float *pose16, uint32_t flags,
                                 const dsm_render_planes *planes_device, int32_t *n_surfels);

/* ---- the map as an occupancy voxel grid (dsm_grid_compose of dsm.h, where a grid is defined) ----
 * kind = DSM_CLOUD_ACTIVE / INACTIVE / ALL / NEIGHBOR with the surfel sets, runs and numbering of dsm_surfel_map_render (for ALL,
 * index i is surfel i of dsm_surfel_map_get_mesh); DSM_CLOUD_RAW: DSM_E_INVALID.  spec, flags, planes, *n_surfels, *n_cells and
 * DSM_E_CAPACITY as for dsm_grid_compose; dsm_grid_spec_around with the translation of dsm_surfel_map_last_pose16 centres the
 * grid on the robot.  DSM_E_STATE before the first fuse.  The map is not changed.  Synchronises. */
int dsm_surfel_map_grid(dsm_surfel_map *m, int kind, const dsm_grid_spec *spec, uint32_t flags, const dsm_grid_planes *planes, int32_t *n_surfels,
                        int32_t *n_cells);
/* the same with the planes in device memory of the node's GPU */
int dsm_surfel_map_grid_device(dsm_surfel_map *m, int kind, const dsm_grid_spec *spec, uint32_t flags, const dsm_grid_planes *planes_device,
                               int32_t *n_surfels, int32_t *n_cells);

/* ---- the map as a truncated Euclidean distance field (dsm_field_compose of dsm.h, where the field is defined) ----
 * The field of the occupied set of dsm_surfel_map_grid for the same kind and spec: kinds, runs and numbering as there; DSM_CLOUD_RAW
 * and unknown kinds: DSM_E_INVALID.  spec, max_dist, flags, planes and *n_surfels as for dsm_field_compose.  DSM_E_STATE before the
 * first fuse.  The map is not changed.  Synchronises. */
int dsm_surfel_map_field(dsm_surfel_map *m, int kind, const dsm_grid_spec *spec, int32_t max_dist, uint32_t flags, const dsm_field_planes *planes,
                         int32_t *n_surfels);
/* the same with the planes in device memory of the node's GPU */
int dsm_surfel_map_field_device(dsm_surfel_map *m, int kind, const dsm_grid_spec *spec, int32_t max_dist, uint32_t flags,
                                const dsm_field_planes *planes_device, int32_t *n_surfels);

/* ---- free and unknown space (dsm_grid_carve / dsm_grid_classify of dsm.h, where both are defined) ----
 * Which voxels the sensor has seen through can only be told from the depth frames while they pass through the node, and the node
 * decides when a frame is fused and keeps only two of them: so the node accumulates itself, opt-in.  From the next fuse on every
 * fused frame is carved, with the slot and the pose it was fused with, into a device bit set the node owns (before the
 * publications of that fuse).  spec NULL: switched off, the memory released (the default: the node then does exactly what it did
 * without this call).  A new spec -- any call with one -- clears the set.  params NULL: dsm_carve_params_init's.  flags:
 * DSM_CARVE_TRUST_INFINITE only.  spec, params and flags are checked here as dsm_grid_carve checks them (DSM_E_INVALID, nothing
 * changed).
 * LIMIT, a loop closure: the warp that follows one moves the map and rewrites the keyframe poses, so what was carved with the old
 * poses is stale.  The set is CLEARED at every warp that changes a pose, and dsm_surfel_map_free_space_resets counts how often:
 * after a reset the set holds only the frames fused since.  Carving again would need the old frames, which the node does not keep.
 * LIMIT, centre sampling: see dsm_grid_carve. */
int dsm_surfel_map_set_free_space(dsm_surfel_map *m, const dsm_grid_spec *spec, const dsm_carve_params *params, uint32_t flags);
int64_t dsm_surfel_map_free_space_resets(const dsm_surfel_map *m);
/* A copy of the accumulated set, [nz][ny][wx] words of the accumulator's spec, into host memory; *n_free (may be NULL) = its
 * population count.  DSM_E_STATE before dsm_surfel_map_set_free_space or before the first fuse.  Synchronises. */
int dsm_surfel_map_free_space(dsm_surfel_map *m, uint32_t *free_out, int64_t *n_free);
/* the same into device memory of the node's GPU (4-byte aligned), ordered like the grid's device destination */
int dsm_surfel_map_free_space_device(dsm_surfel_map *m, void *free_device, int64_t *n_free);
/* The occupied set of dsm_surfel_map_grid for `kind` and the accumulator's spec, classified against the accumulated free set:
 * planes, *n_frontier and DSM_E_CAPACITY as for dsm_grid_classify, but the planes in HOST memory; *n_surfels as for
 * dsm_surfel_map_grid (either count may be NULL).  DSM_E_STATE before dsm_surfel_map_set_free_space or before the first fuse.
 * Synchronises. */
int dsm_surfel_map_space(dsm_surfel_map *m, int kind, const dsm_space_planes *planes, int32_t *n_surfels, int32_t *n_frontier);
/* the same with the planes in device memory of the node's GPU */
int dsm_surfel_map_space_device(dsm_surfel_map *m, int kind, const dsm_space_planes *planes_device, int32_t *n_surfels, int32_t *n_frontier);
/* The stateless counterpart, for callers with their own grid: one dsm_grid_carve of the latest fused frame, with the pose it was
 * fused with, into the caller's set in device memory.  params NULL: the defaults.  DSM_E_STATE before the first fuse. */
int dsm_surfel_map_carve_last(dsm_surfel_map *m, const dsm_grid_spec *spec, const dsm_carve_params *params, uint32_t flags, void *free_device);

/* ---- frontier clusters: the frontier of dsm_surfel_map_space as connected components (dsm_grid_components of dsm.h) ----
 * The occupied set of `kind` in the accumulator's grid is classified against the accumulated free set exactly as
 * dsm_surfel_map_space does it, and the frontier is labelled with q->connectivity; clusters of fewer than q->min_count voxels are
 * left out of the table (never out of `label`).  With q->has_from the known-free set is labelled as well, with DSM_CONNECT_FACES,
 * and a cluster's `tag` is the root of the known-free region that holds the cluster's ROOT voxel (never -1: a frontier voxel is
 * known free).  With 6-connected clusters the whole cluster lies in that region; with 26 it is the region of the root voxel only.
 * *from_root = the known-free root at the voxel of q->from, i_a = (int)floor(((double)from_a - (double)origin_a) / (double)voxel),
 * or -1 when that voxel is outside the grid or not known free.  A cluster can be reached from `from` through known-free space iff
 * tag == *from_root.  Without has_from: tag 0, *from_root -1.
 * table: [table_cap] entries, label: [nz][ny][nx] (may be NULL), in host memory; *n_clusters = the clusters that pass min_count
 * (more than table_cap: DSM_E_CAPACITY with the count needed, the first table_cap entries and `label` complete), *n_all (may be
 * NULL) = all of them.  DSM_E_STATE before dsm_surfel_map_set_free_space or before the first fuse; DSM_E_INVALID for a wrong
 * struct_size, a kind dsm_surfel_map_space refuses, and what dsm_grid_components refuses (more than 2^26 voxels among it).  The map
 * and the accumulator are not changed.  Synchronises.
 * Not provided: clusters tracked across calls, pose search (dsm_surfel_map_view_gain below scores the poses a caller proposes),
 * and labelling across a loop-closure reset (the accumulator starts again there, and so do the clusters). */
typedef struct dsm_frontier_query {
    uint32_t struct_size; /* sizeof(dsm_frontier_query) */
    int32_t connectivity; /* of the frontier clusters: DSM_CONNECT_FACES or DSM_CONNECT_ALL */
    int32_t min_count;    /* >= 1 */
    int32_t has_from;     /* 0: no reachability */
    float from[3];        /* a world point, e.g. the translation of dsm_surfel_map_last_pose16 */
} dsm_frontier_query;
/* DSM_CONNECT_ALL, min_count 1, no from */
void dsm_frontier_query_init(dsm_frontier_query *q);
int dsm_surfel_map_frontier_clusters(dsm_surfel_map *m, int kind, const dsm_frontier_query *q, dsm_component *table, int32_t table_cap, int32_t *label,
                                     int32_t *n_clusters, int32_t *n_all, int32_t *from_root);
/* the same with table (8-byte aligned) and label (4-byte aligned) in device memory of the node's GPU */
int dsm_surfel_map_frontier_clusters_device(dsm_surfel_map *m, int kind, const dsm_frontier_query *q, dsm_component *table_device, int32_t table_cap,
                                            int32_t *label_device, int32_t *n_clusters, int32_t *n_all, int32_t *from_root);

/* ---- viewpoint gain: what a camera at a candidate pose would see of the node's space (dsm_grid_view of dsm.h, where it is defined) ----
 * The occupied set of `kind` in the accumulator's grid is composed and classified against the accumulated free set exactly as
 * dsm_surfel_map_space does it; then the n_poses poses (cam -> world, 16 column-major floats each; the closed-form inverse is
 * taken) are scored by dsm_grid_view with q->camera and q->flags (DSM_VIEW_*), the frontier being the target set with
 * DSM_VIEW_TARGET_FRONTIER.  scores: [n_poses], visible: [n_poses][nz][ny][wx] words (may be NULL), in host memory; one of them
 * may be NULL, not both.  DSM_E_STATE before dsm_surfel_map_set_free_space or before the first fuse; DSM_E_INVALID for a wrong
 * struct_size, an unknown target, a kind dsm_surfel_map_space refuses, and what dsm_grid_view refuses.  After a loop-closure
 * reset the accumulator is empty, so everything but the occupied set is unknown again.  The map and the accumulator are not
 * changed.  Synchronises. */
#define DSM_VIEW_TARGET_NONE 0
#define DSM_VIEW_TARGET_FRONTIER 1
typedef struct dsm_view_query {
    uint32_t struct_size;     /* sizeof(dsm_view_query) */
    dsm_render_camera camera; /* the view camera: any size and intrinsics, as for dsm_grid_view */
    uint32_t flags;           /* DSM_VIEW_UNKNOWN_BLOCKS or 0 */
    int32_t target;           /* DSM_VIEW_TARGET_NONE or DSM_VIEW_TARGET_FRONTIER */
} dsm_view_query;
/* The node's own image size and intrinsics with the accumulator's carve range (dsm_carve_params_init's range while free space is
 * switched off); flags 0; the frontier as target.  m NULL: the camera is left zero for the caller to fill. */
void dsm_view_query_init(const dsm_surfel_map *m, dsm_view_query *q);
int dsm_surfel_map_view_gain(dsm_surfel_map *m, int kind, const dsm_view_query *q, int32_t n_poses, const float *poses16, dsm_view_score *scores,
                             uint32_t *visible);
/* the same with scores and visible (4-byte aligned) in device memory of the node's GPU */
int dsm_surfel_map_view_gain_device(dsm_surfel_map *m, int kind, const dsm_view_query *q, int32_t n_poses, const float *poses16,
                                    dsm_view_score *scores_device, uint32_t *visible_device);

/* ---- the latest frame against the map (dsm_align_frame of dsm.h, where the alignment is defined) ----
 * Aligns the depth frame of the latest fuse, still in its engine slot, against the surfel set of `kind` with the rules and runs of
 * dsm_surfel_map_render (ACTIVE: refine or judge a pose; INACTIVE: verify a loop closure against the inactive map), seen by the
 * node's own camera at pose16_guess (cam -> world, 16 column-major floats; NULL: the pose of the latest fuse).  DSM_CLOUD_RAW and
 * unknown kinds: DSM_E_INVALID.  DSM_E_STATE before the first fuse.  The map, the store and the frame are not changed: what to do
 * with the refined pose is the caller's decision.  Synchronises. */
int dsm_surfel_map_align_last(dsm_surfel_map *m, int kind, const float *pose16_guess, const dsm_align_params *params, dsm_align_result *result);
/* The pose of the latest fuse as the engine was given it (cam -> world, 16 column-major floats): the guess and the render pose
 * that NULL stands for above.  fuse_pose of a publication is the same pose as a quaternion.  DSM_E_STATE before the first fuse. */
int dsm_surfel_map_last_pose16(const dsm_surfel_map *m, float *pose16);

/* ---- taps (what the publish_* methods read) ---- */
dsm_handle *dsm_surfel_map_engine(dsm_surfel_map *m); /* active map: dsm_map_size / dsm_map_download */
int64_t dsm_surfel_map_frames_fused(const dsm_surfel_map *m);
/* poses whose image or depth never arrived (a newer frame was already waiting): the reference spins forever on
 * these (surfel_map.cpp:114-139); here they are dropped so that later poses proceed */
int64_t dsm_surfel_map_dropped_poses(const dsm_surfel_map *m);
int32_t dsm_surfel_map_pose_count(const dsm_surfel_map *m);
/* poses_database[i]: cam_pose, loop_pose, number of attached (inactive) surfels, points_begin_index,
 * whether i is in local_surfels_indexs; any output may be NULL */
int dsm_surfel_map_get_pose(const dsm_surfel_map *m, int32_t i, dsm_pose_msg *cam_pose, dsm_pose_msg *loop_pose,
                            int32_t *n_attached, int32_t *points_begin_index, int32_t *is_local);
/* poses_database[i].linked_pose_index, in insertion order; returns the count (or a negative status) */
int32_t dsm_surfel_map_get_links(const dsm_surfel_map *m, int32_t i, int32_t *out, int32_t cap);
/* poses_database[i].attached_surfels */
int dsm_surfel_map_get_attached(dsm_surfel_map *m, int32_t i, dsm_surfel *out, int32_t cap, int32_t *n);
/* inactive_pointcloud: 4 floats per point (x, y, z, intensity) */
int dsm_surfel_map_get_inactive_cloud(dsm_surfel_map *m, float *xyzi_out, int32_t cap, int32_t *n);

#ifdef __cplusplus
}
#endif
#endif
