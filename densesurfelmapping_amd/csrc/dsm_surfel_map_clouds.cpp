// dsm_surfel_map_clouds.cpp -- the node's point-cloud topics (include/dsm_surfel_map.h: dsm_surfel_map_get_cloud*,
// dsm_surfel_map_set_publish) over the engine's dsm_cloud_compose / dsm_frame_cloud.  Line numbers refer to the reference's
// surfel_fusion/src/surfel_map.cpp.  A translation unit of its own: dsm_surfel_map.cpp reaches it only through the function
// pointers of struct dsm_surfel_map (dsm_surfel_map_node.h), so the node's host logic links against the engine entry points
// it always used.
#include "dsm_surfel_map_node.h"

#include <cstring>

namespace {

using namespace dsm_node;

// One cloud of the current state into dst (host or device memory of the node's GPU).
int build_cloud(dsm_surfel_map *m, int kind, void *dst, int on_device, int32_t cap, int32_t *n) {
    if (!m->last.valid) return fail(m, DSM_E_STATE, "no frame fused yet");
    if (kind == DSM_CLOUD_RAW) { // :1115-1151 with the latest fuse's frame and fuse_pose_ros
        const dsm_pose_msg &p = m->last.fuse_pose;
        const double pose7[7] = {p.px, p.py, p.pz, p.qx, p.qy, p.qz, p.qw};
        const int rc = dsm_frame_cloud(m->engine, m->last.slot, pose7, dst, on_device, cap, n);
        return rc ? engine_fail(m, rc, "dsm_frame_cloud") : DSM_OK;
    }
    int select = DSM_CLOUD_SELECT_NONE;
    std::vector<int32_t> begin, count;
    if (kind == DSM_CLOUD_ACTIVE || kind == DSM_CLOUD_INACTIVE || kind == DSM_CLOUD_ALL) {
        if (kind != DSM_CLOUD_INACTIVE) select = DSM_CLOUD_SELECT_MATURE; // :1404-1405
        if (kind != DSM_CLOUD_ACTIVE) { // (*pointcloud) += (*inactive_pointcloud), :1391, :1441
            int32_t total = 0;
            const int rc = dsm_store_size(m->engine, &total);
            if (rc) return engine_fail(m, rc, "dsm_store_size");
            begin.push_back(0);
            count.push_back(total);
        }
    } else if (kind == DSM_CLOUD_NEIGHBOR) { // :1292-1319
        select = DSM_CLOUD_SELECT_NONZERO;
        std::vector<int> neighbor_indexs;
        get_driftfree_poses(m, m->last.relative_index, neighbor_indexs, 2 * m->cfg.drift_free_poses);
        for (int this_pose : neighbor_indexs) {
            if (m->local_surfels_indexs.count(this_pose)) continue;
            const int sg = m->poses_database[(size_t)this_pose].segment;
            if (sg < 0 || m->segments[(size_t)sg].count <= 0) continue; // attached_surfels.size() <= 0
            begin.push_back(m->segments[(size_t)sg].begin);
            count.push_back(m->segments[(size_t)sg].count);
        }
    } else {
        return fail(m, DSM_E_INVALID, "cloud kind %d", kind);
    }
    const int rc = dsm_cloud_compose(m->engine, select, (int32_t)begin.size(), begin.data(), count.data(), dst, on_device, cap, n);
    return rc ? engine_fail(m, rc, "dsm_cloud_compose") : DSM_OK;
}

// the publisher installed by dsm_surfel_map_set_publish: page-locked buffers that only grow
struct Publisher {
    uint32_t mask = 0;
    dsm_surfel_map_publish_fn fn = nullptr;
    void *user = nullptr;
    float *buf[DSM_CLOUD_KINDS] = {};
    int32_t cap[DSM_CLOUD_KINDS] = {};
};

void release_publisher(dsm_surfel_map *m) {
    Publisher *pub = (Publisher *)m->publish;
    if (!pub) return;
    for (int k = 0; k < DSM_CLOUD_KINDS; k++)
        if (pub->buf[k]) dsm_host_free(pub->buf[k]);
    delete pub;
    m->publish = nullptr;
    m->on_fused = nullptr;
    m->release_publish = nullptr;
}

int grow(dsm_surfel_map *m, Publisher *pub, int k, int32_t need) {
    if (need <= pub->cap[k]) return DSM_OK;
    if (pub->buf[k]) dsm_host_free(pub->buf[k]);
    pub->buf[k] = nullptr;
    pub->cap[k] = 0;
    int64_t want = (int64_t)need + need / 2 + 1024;
    if (want > INT32_MAX) want = INT32_MAX;
    void *p = nullptr;
    const int rc = dsm_host_alloc(&p, (size_t)want * 4 * sizeof(float));
    if (rc) return fail(m, rc, "no page-locked memory for %lld cloud points", (long long)want);
    pub->buf[k] = (float *)p;
    pub->cap[k] = (int32_t)want;
    return DSM_OK;
}

// :189-197, after fuse_map: build every requested cloud, hand them to the callback
int publish_fused(dsm_surfel_map *m) {
    Publisher *pub = (Publisher *)m->publish;
    dsm_surfel_map_publication out;
    memset(&out, 0, sizeof out);
    out.stamp = m->last.stamp;
    out.relative_index = m->last.relative_index;
    out.fuse_pose = m->last.fuse_pose;
    out.kinds_mask = pub->mask;
    for (int k = 0; k < DSM_CLOUD_KINDS; k++) {
        if (!(pub->mask & DSM_CLOUD_BIT(k))) continue;
        int32_t n = 0;
        int rc = build_cloud(m, k, pub->buf[k], 0, pub->cap[k], &n);
        if (rc == DSM_E_CAPACITY && n > pub->cap[k]) { // the cloud outgrew its buffer: grow it and build again
            if ((rc = grow(m, pub, k, n))) return rc;
            rc = build_cloud(m, k, pub->buf[k], 0, pub->cap[k], &n);
        }
        if (rc) return rc;
        out.points[k] = pub->buf[k];
        out.n_points[k] = n;
    }
    pub->fn(pub->user, &out);
    return DSM_OK;
}

} // namespace

extern "C" {

int dsm_surfel_map_get_cloud(dsm_surfel_map *m, int kind, float *xyzi_out, int32_t cap, int32_t *n) {
    if (!m || !n || cap < 0 || (cap && !xyzi_out)) return DSM_E_INVALID;
    return build_cloud(m, kind, xyzi_out, 0, cap, n);
}

int dsm_surfel_map_get_cloud_device(dsm_surfel_map *m, int kind, void *dst_device, int32_t cap, int32_t *n) {
    if (!m || !n || cap < 0 || (cap && !dst_device)) return DSM_E_INVALID;
    return build_cloud(m, kind, dst_device, 1, cap, n);
}

int dsm_surfel_map_set_publish(dsm_surfel_map *m, uint32_t kinds_mask, dsm_surfel_map_publish_fn fn, void *user) {
    if (!m) return DSM_E_INVALID;
    if (kinds_mask & ~((1u << DSM_CLOUD_KINDS) - 1u)) return fail(m, DSM_E_INVALID, "cloud kinds mask 0x%x", kinds_mask);
    if (!kinds_mask || !fn) {
        release_publisher(m);
        return DSM_OK;
    }
    Publisher *pub = (Publisher *)m->publish;
    if (!pub) {
        pub = new Publisher();
        m->publish = pub;
        m->release_publish = release_publisher;
    }
    pub->mask = kinds_mask;
    pub->fn = fn;
    pub->user = user;
    m->on_fused = publish_fused;
    return DSM_OK;
}

} // extern "C"
