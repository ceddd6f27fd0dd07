// dsm_surfel_map_align.cpp -- the node's latest frame against its map (include/dsm_surfel_map.h: dsm_surfel_map_align_last) over
// the engine's dsm_align_frame.  The frame is still in the slot the latest fuse read; the surfel sets and their runs are those
// of dsm_surfel_map_render (dsm_node::render_runs).  A translation unit of its own, like the clouds, the mesh and the renders.
#include "dsm_surfel_map_node.h"

extern "C" {

int dsm_surfel_map_align_last(dsm_surfel_map *m, int kind, const float *pose16_guess, const dsm_align_params *params, dsm_align_result *result) {
    if (!m || !params || !result) return DSM_E_INVALID;
    // the state before the runs, as in dsm_surfel_map_render: render_runs reads the pose of the latest fuse (NEIGHBOR)
    if (kind == DSM_CLOUD_RAW || kind < DSM_CLOUD_ACTIVE || kind > DSM_CLOUD_RAW) {
        m->err = "align kind " + std::to_string(kind);
        return DSM_E_INVALID;
    }
    if (!m->last.valid) {
        m->err = "no frame fused yet";
        return DSM_E_STATE;
    }
    int select = DSM_CLOUD_SELECT_NONE;
    std::vector<int32_t> begin, count;
    if (!dsm_node::render_runs(m, kind, select, begin, count)) {
        m->err = "align kind " + std::to_string(kind);
        return DSM_E_INVALID;
    }
    dsm_render_camera cam; // the node's camera
    cam.width = m->cfg.cam_width;
    cam.height = m->cfg.cam_height;
    cam.fx = m->cfg.cam_fx;
    cam.fy = m->cfg.cam_fy;
    cam.cx = m->cfg.cam_cx;
    cam.cy = m->cfg.cam_cy;
    cam.near_dist = m->cfg.fuse_near_distence;
    cam.far_dist = m->cfg.fuse_far_distence;
    const int rc = dsm_align_frame(m->engine, m->last.slot, select, (int32_t)begin.size(), begin.data(), count.data(), &cam,
                                   pose16_guess ? pose16_guess : m->last.pose16, params, result);
    if (rc) m->err = std::string("dsm_align_frame: ") + dsm_last_error(m->engine);
    return rc;
}

int dsm_surfel_map_last_pose16(const dsm_surfel_map *m, float *pose16) {
    if (!m || !pose16) return DSM_E_INVALID;
    if (!m->last.valid) return DSM_E_STATE;
    for (int k = 0; k < 16; k++) pose16[k] = m->last.pose16[k];
    return DSM_OK;
}

} // extern "C"
