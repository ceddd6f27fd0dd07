// dsm_surfel_map_grid.cpp -- the node's map as an occupancy voxel grid (include/dsm_surfel_map.h: dsm_surfel_map_grid*) over the
// engine's dsm_grid_compose.  The surfel sets and their runs are those of dsm_surfel_map_render (dsm_node::render_runs): the
// attached surfels keyframe by keyframe first, then the map part.  A translation unit of its own, like the clouds, the mesh and
// the renders.
#include "dsm_surfel_map_node.h"

namespace {

using namespace dsm_node;

int grid(dsm_surfel_map *m, int kind, const dsm_grid_spec *spec, uint32_t flags, const dsm_grid_planes *planes, int on_device, int32_t *n_surfels,
         int32_t *n_cells) {
    if (!m || !spec || !planes || !n_surfels || !n_cells) return DSM_E_INVALID;
    if (!m->last.valid) return fail(m, DSM_E_STATE, "no frame fused yet");
    int select = DSM_CLOUD_SELECT_NONE;
    std::vector<int32_t> begin, count;
    if (!render_runs(m, kind, select, begin, count)) return fail(m, DSM_E_INVALID, "grid kind %d", kind);
    const int rc = dsm_grid_compose(m->engine, select, (int32_t)begin.size(), begin.data(), count.data(), spec, flags, planes, on_device, n_surfels, n_cells);
    return rc ? fail(m, rc, "dsm_grid_compose: %s", dsm_last_error(m->engine)) : DSM_OK;
}

} // namespace

extern "C" {

int dsm_surfel_map_grid(dsm_surfel_map *m, int kind, const dsm_grid_spec *spec, uint32_t flags, const dsm_grid_planes *planes, int32_t *n_surfels,
                        int32_t *n_cells) {
    return grid(m, kind, spec, flags, planes, 0, n_surfels, n_cells);
}

int dsm_surfel_map_grid_device(dsm_surfel_map *m, int kind, const dsm_grid_spec *spec, uint32_t flags, const dsm_grid_planes *planes_device,
                               int32_t *n_surfels, int32_t *n_cells) {
    return grid(m, kind, spec, flags, planes_device, 1, n_surfels, n_cells);
}

} // extern "C"
