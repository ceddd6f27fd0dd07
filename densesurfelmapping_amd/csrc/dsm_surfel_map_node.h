// dsm_surfel_map_node.h -- the state of the node (include/dsm_surfel_map.h), shared by its eight translation units:
// dsm_surfel_map.cpp (the host logic of class SurfelMap), dsm_surfel_map_clouds.cpp (the point-cloud publications),
// dsm_surfel_map_mesh.cpp, dsm_surfel_map_render.cpp and dsm_surfel_map_align.cpp (the mesh, the rendered images, the alignment),
// dsm_surfel_map_grid.cpp, dsm_surfel_map_field.cpp and dsm_surfel_map_space.cpp (the voxel grid, its distance field, free space).
// dsm_surfel_map.cpp calls only the engine entry points it always called; the publications reach it through the function
// pointers of struct dsm_surfel_map.  Internal: not installed, not part of the C ABI.
#pragma once
#include "../../include/dsm_surfel_map.h"

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <list>
#include <set>
#include <string>
#include <tuple>
#include <vector>

namespace dsm_node {

// ------------------------------------------------------------------ fp64 rigid-transform helpers
struct Mat4 {
    double d[16]; // column-major, d[j*4+i] = (i,j)
    double &operator()(int i, int j) { return d[j * 4 + i]; }
    double operator()(int i, int j) const { return d[j * 4 + i]; }
};

inline Mat4 identity4() {
    Mat4 m;
    for (int k = 0; k < 16; k++) m.d[k] = 0.0;
    m(0, 0) = m(1, 1) = m(2, 2) = m(3, 3) = 1.0;
    return m;
}

// ------------------------------------------------------------------ node state
struct PoseElement { // surfel_map.h:36-46; attached_surfels live in the handle's store
    dsm_pose_msg cam_pose, loop_pose;
    std::vector<int> linked_pose_index;
    int segment = -1; // index into dsm_surfel_map::segments while the keyframe is inactive, else -1
    dsm_stamp cam_stamp = {0, 0};
};

// The inactive set as a segment table.  The handle's store holds the surfels of the inactive keyframes back to
// back in deactivation order; entry i of the table says which keyframe owns the i-th run and how long it is, and a
// run starts where the runs before it end.  This one table is what the reference spreads over three members:
// PoseElement::attached_surfels.size() (count), PoseElement::points_begin_index (start) and
// pointcloud_pose_index / PoseElement::points_pose_index (the table order and its inverse), surfel_map.h:36-46,134.
struct Segment {
    int keyframe;
    int begin; // sum of the counts before this entry (kept, not recomputed: the taps read it)
    int count;
};

struct FramePool;
struct Frame {
    dsm_stamp stamp;
    uint8_t *bytes; // tightly packed rows: a page-locked block of the node's pool, or (overflow) pageable memory
    bool pinned;
    FramePool *pool;       // the pool the bytes came from (release them there)
    float u16_scale = 0;   // > 0: a uint16 depth frame (dsm_surfel_map_depth_input_u16), converted on upload with u16_op
    int32_t u16_op = 0;
    int32_t image_format = 0; // != DSM_IMAGE_MONO8: a colour image frame (dsm_surfel_map_image_input_color), 3 or 4 bytes a pixel,
    int32_t gray[4] = {0, 0, 0, 0}; // converted to grey on upload with these weights (wr, wg, wb, shift)
};

// Frames wait for their pose in page-locked memory so that the upload of a frame is one DMA -- but only the first
// kPinnedFrames of each kind: the reference's subscriber queues are 5000 deep (ros_node.cpp:24-25) in PAGEABLE memory, and
// a stalled pose source must not pin 5000 x 2.3 MB of host RAM.  The overflow lives in pageable blocks (their upload is a
// staged copy: slower, still correct) that are freed as soon as they leave the queue; free page-locked blocks beyond
// kPooledFrames go back to the system as well.
constexpr size_t kPinnedFrames = 256, kPooledFrames = 64;

struct FramePool {
    std::vector<uint8_t *> free_blocks; // page-locked, ready for reuse
    size_t pinned_live = 0;             // page-locked blocks handed out and not yet released
    uint8_t *take(size_t bytes, bool *pinned) {
        if (!free_blocks.empty()) {
            uint8_t *p = free_blocks.back();
            free_blocks.pop_back();
            pinned_live++;
            *pinned = true;
            return p;
        }
        if (pinned_live < kPinnedFrames) {
            void *p = nullptr;
            if (dsm_host_alloc(&p, bytes) == DSM_OK) {
                pinned_live++;
                *pinned = true;
                return (uint8_t *)p;
            }
        }
        *pinned = false;
        return (uint8_t *)malloc(bytes ? bytes : 1);
    }
    void release(const Frame &f) {
        if (f.pool != this) { f.pool->release(f); return; } // (a depth list holds float and uint16 frames)
        if (!f.pinned) { free(f.bytes); return; }
        pinned_live--;
        if (free_blocks.size() < kPooledFrames) free_blocks.push_back(f.bytes);
        else dsm_host_free(f.bytes);
    }
    void drain() {
        for (uint8_t *p : free_blocks) dsm_host_free(p);
        free_blocks.clear();
    }
};

// what the publications of one fuse refer to (synchronize_msgs, surfel_map.cpp:143-152)
struct FuseInfo {
    bool valid = false;
    dsm_stamp stamp = {0, 0};   // fuse_stamp
    int relative_index = -1;
    dsm_pose_msg fuse_pose = {}; // fuse_pose_ros = pose_eigen2ros(reference_pose * relative_pose)
    int slot = 0;               // the engine frame slot that holds the fused frame
    float pose16[16] = {};      // the cam -> world matrix the engine fused it with (dsm_surfel_map_render's default pose)
};

} // namespace dsm_node

struct dsm_surfel_map {
    using Frame = dsm_node::Frame;
    using FramePool = dsm_node::FramePool;
    using PoseElement = dsm_node::PoseElement;
    using Segment = dsm_node::Segment;
    using FuseInfo = dsm_node::FuseInfo;
    using Mat4 = dsm_node::Mat4;
    dsm_surfel_map_config cfg;
    dsm_handle *engine = nullptr;
    std::list<Frame> image_buffer, depth_buffer;                                 // surfel_map.h:96-97
    FramePool image_pool, depth_pool, depth16_pool;                              // where the buffered frames' bytes live (depth16: uint16 frames)
    FramePool color3_pool, color4_pool;                                          // colour image frames, 3 and 4 bytes a pixel
    std::list<std::tuple<dsm_stamp, dsm_pose_msg, int>> pose_reference_buffer; // :98
    std::vector<PoseElement> poses_database;                                     // :120
    std::set<int> local_surfels_indexs;                                          // :122
    std::vector<Segment> segments;                                               // inactive set, store order (:134)
    int64_t poses_dropped = 0, frames_dropped = 0;
    bool failed = false; // an engine call failed half-way through a state change: refuse further input
    Mat4 transform_kitti = dsm_node::identity4();                                          // function-static at surfel_map.cpp:215
    int64_t frames_fused = 0;
    std::string err;
    // the latest fuse, what the clouds of dsm_surfel_map_get_cloud refer to (set by synchronize_msgs; last.valid false before)
    FuseInfo last;
    // dsm_surfel_map_set_publish (dsm_surfel_map_clouds.cpp) installs these: called after every fuse where the reference
    // publishes (surfel_map.cpp:189-197), and by dsm_surfel_map_destroy.  Null (the default): no extra work, no synchronisation.
    int (*on_fused)(dsm_surfel_map *m) = nullptr;
    void (*release_publish)(dsm_surfel_map *m) = nullptr;
    void *publish = nullptr; // the publisher's own state
    // dsm_surfel_map_set_free_space (dsm_surfel_map_space.cpp) installs these: on_carve at the fuse site, before on_fused (the fused
    // frame into the accumulated free set); on_warped after a warp_surfels that went through (the set is stale: cleared and counted);
    // release_space by dsm_surfel_map_destroy.  Null (the default): no extra work, no synchronisation.
    int (*on_carve)(dsm_surfel_map *m) = nullptr;
    int (*on_warped)(dsm_surfel_map *m) = nullptr;
    void (*release_space)(dsm_surfel_map *m) = nullptr;
    void *space = nullptr; // the accumulator's own state
    int64_t free_space_resets = 0;
};

namespace dsm_node {

// the node's last error (dsm_surfel_map_last_error) and the code to return with it; m may be null
inline int fail(dsm_surfel_map *m, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (m) m->err = buf;
    return code;
}

// an engine call failed with rc: its name and the engine's own text
inline int engine_fail(dsm_surfel_map *m, int rc, const char *what) { return fail(m, rc, "%s: %s", what, dsm_last_error(m->engine)); }

// SurfelMap::get_driftfree_poses (:1643-1673): breadth-first over linked_pose_index, root first,
// driftfree_range - 1 levels, each pose once in discovery order
inline void get_driftfree_poses(const dsm_surfel_map *m, int root_index, std::vector<int> &driftfree_poses, int driftfree_range) {
    if ((int)m->poses_database.size() < root_index + 1) return;
    std::vector<int> this_level, next_level;
    this_level.push_back(root_index);
    driftfree_poses.push_back(root_index);
    for (int i = 1; i < driftfree_range; i++) {
        for (int p : this_level)
            for (int linked : m->poses_database[p].linked_pose_index)
                if (std::find(driftfree_poses.begin(), driftfree_poses.end(), linked) == driftfree_poses.end()) {
                    next_level.push_back(linked);
                    driftfree_poses.push_back(linked);
                }
        this_level.swap(next_level);
        next_level.clear();
    }
}

// save_mesh's order of the attached surfels (surfel_map.cpp:1226-1238): keyframe by keyframe, in poses_database order (not
// store order), as runs of the store
inline void attached_runs(const dsm_surfel_map *m, std::vector<int32_t> &begin, std::vector<int32_t> &count) {
    for (const dsm_surfel_map::PoseElement &pe : m->poses_database) {
        if (pe.segment < 0) continue;
        const dsm_surfel_map::Segment &sg = m->segments[(size_t)pe.segment];
        if (sg.count <= 0) continue;
        begin.push_back(sg.begin);
        count.push_back(sg.count);
    }
}

// The surfel set of a cloud kind as dsm_render_compose takes it: the map part's `select` and the store's record runs in the mesh's
// order (dsm_surfel_map_render's rules; NEIGHBOR: surfel_map.cpp:1292-1319).  False: the kind has no such set (RAW, unknown).
inline bool render_runs(const dsm_surfel_map *m, int kind, int &select, std::vector<int32_t> &begin, std::vector<int32_t> &count) {
    select = DSM_CLOUD_SELECT_NONE;
    if (kind == DSM_CLOUD_ACTIVE || kind == DSM_CLOUD_INACTIVE || kind == DSM_CLOUD_ALL) {
        if (kind != DSM_CLOUD_INACTIVE) select = DSM_CLOUD_SELECT_MATURE;
        if (kind != DSM_CLOUD_ACTIVE) attached_runs(m, begin, count);
        return true;
    }
    if (kind != DSM_CLOUD_NEIGHBOR) return false;
    select = DSM_CLOUD_SELECT_NONZERO;
    std::vector<int> neighbor_indexs;
    get_driftfree_poses(m, m->last.relative_index, neighbor_indexs, 2 * m->cfg.drift_free_poses);
    for (int this_pose : neighbor_indexs) {
        if (m->local_surfels_indexs.count(this_pose)) continue;
        const int sg = m->poses_database[(size_t)this_pose].segment;
        if (sg < 0 || m->segments[(size_t)sg].count <= 0) continue;
        begin.push_back(m->segments[(size_t)sg].begin);
        count.push_back(m->segments[(size_t)sg].count);
    }
    return true;
}

} // namespace dsm_node
