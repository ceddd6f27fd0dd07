// dsm_surfel_map_field.cpp -- the node's map as a truncated Euclidean distance field (include/dsm_surfel_map.h:
// dsm_surfel_map_field*) over the engine's dsm_field_compose.  The surfel sets and their runs are those of dsm_surfel_map_grid
// (dsm_node::render_runs).  A translation unit of its own, like the grid's.
#include "dsm_surfel_map_node.h"

namespace {

using namespace dsm_node;

int field(dsm_surfel_map *m, int kind, const dsm_grid_spec *spec, int32_t max_dist, uint32_t flags, const dsm_field_planes *planes, int on_device,
          int32_t *n_surfels) {
    if (!m || !spec || !planes || !n_surfels) return DSM_E_INVALID;
    if (!m->last.valid) return fail(m, DSM_E_STATE, "no frame fused yet");
    int select = DSM_CLOUD_SELECT_NONE;
    std::vector<int32_t> begin, count;
    if (!render_runs(m, kind, select, begin, count)) return fail(m, DSM_E_INVALID, "field kind %d", kind);
    const int rc = dsm_field_compose(m->engine, select, (int32_t)begin.size(), begin.data(), count.data(), spec, max_dist, flags, planes, on_device, n_surfels);
    return rc ? fail(m, rc, "dsm_field_compose: %s", dsm_last_error(m->engine)) : DSM_OK;
}

} // namespace

extern "C" {

int dsm_surfel_map_field(dsm_surfel_map *m, int kind, const dsm_grid_spec *spec, int32_t max_dist, uint32_t flags, const dsm_field_planes *planes,
                         int32_t *n_surfels) {
    return field(m, kind, spec, max_dist, flags, planes, 0, n_surfels);
}

int dsm_surfel_map_field_device(dsm_surfel_map *m, int kind, const dsm_grid_spec *spec, int32_t max_dist, uint32_t flags,
                                const dsm_field_planes *planes_device, int32_t *n_surfels) {
    return field(m, kind, spec, max_dist, flags, planes_device, 1, n_surfels);
}

} // extern "C"
