// dsm_surfel_map_render.cpp -- the node's map as images (include/dsm_surfel_map.h: dsm_surfel_map_render*) over the engine's
// dsm_render_compose.  The surfel sets are those of the clouds of the same kind, as RECORD runs in the mesh's order: the
// attached surfels keyframe by keyframe first (dsm_node::attached_runs; for NEIGHBOR the runs of the drift-free neighbours in
// publish_neighbor_pointcloud's breadth-first order), then the map part.  A translation unit of its own, like the clouds and the mesh.
#include "dsm_surfel_map_node.h"

namespace {

using namespace dsm_node;

int render(dsm_surfel_map *m, int kind, const dsm_render_camera *camera, const float *pose16, uint32_t flags, const dsm_render_planes *planes,
           int on_device, int32_t *n_surfels) {
    if (!m || !planes || !n_surfels) return DSM_E_INVALID;
    if (!m->last.valid) return fail(m, DSM_E_STATE, "no frame fused yet");
    int select = DSM_CLOUD_SELECT_NONE;
    std::vector<int32_t> begin, count;
    if (!render_runs(m, kind, select, begin, count)) return fail(m, DSM_E_INVALID, "render kind %d", kind);
    dsm_render_camera own;
    if (!camera) { // the node's camera
        own.width = m->cfg.cam_width;
        own.height = m->cfg.cam_height;
        own.fx = m->cfg.cam_fx;
        own.fy = m->cfg.cam_fy;
        own.cx = m->cfg.cam_cx;
        own.cy = m->cfg.cam_cy;
        own.near_dist = m->cfg.fuse_near_distence;
        own.far_dist = m->cfg.fuse_far_distence;
        camera = &own;
    }
    const int rc = dsm_render_compose(m->engine, select, (int32_t)begin.size(), begin.data(), count.data(), camera, pose16 ? pose16 : m->last.pose16,
                                      nullptr, flags, planes, on_device, n_surfels);
    return rc ? fail(m, rc, "dsm_render_compose: %s", dsm_last_error(m->engine)) : DSM_OK;
}

} // namespace

extern "C" {

int dsm_surfel_map_render(dsm_surfel_map *m, int kind, const dsm_render_camera *camera, const float *pose16, uint32_t flags,
                          const dsm_render_planes *planes, int32_t *n_surfels) {
    return render(m, kind, camera, pose16, flags, planes, 0, n_surfels);
}

int dsm_surfel_map_render_device(dsm_surfel_map *m, int kind, const dsm_render_camera *camera, const float *pose16, uint32_t flags,
                                 const dsm_render_planes *planes_device, int32_t *n_surfels) {
    return render(m, kind, camera, pose16, flags, planes_device, 1, n_surfels);
}

} // extern "C"
