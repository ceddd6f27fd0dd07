// dsm_surfel_map_space.cpp -- the node's free and unknown space (include/dsm_surfel_map.h: dsm_surfel_map_set_free_space,
// _free_space*, _space*, _carve_last, _frontier_clusters*, _view_gain*) over the engine's dsm_grid_carve, dsm_grid_classify,
// dsm_grid_components and dsm_grid_view.  The accumulator is a bit set in
// device memory that this file owns; dsm_surfel_map.cpp reaches it through the function pointers of struct dsm_surfel_map
// (on_carve at the fuse site, on_warped after a warp, release_space at destruction), all null until dsm_surfel_map_set_free_space
// installs them.  The per-fuse carve is the SYNCHRONISING dsm_grid_carve: it is enqueued behind the fuse on the engine's stream and
// has returned before the slot's next upload is issued.  The set is cleared and copied on the null stream; dsm_grid_carve orders
// itself behind that stream (a caller's device memory), so a clear cannot overtake or be overtaken by a carve.
#include "dsm_components.h"
#include "dsm_grid_shape.h"
#include "dsm_surfel_map_node.h"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstring>

namespace {

using namespace dsm_node;

struct Space {
    dsm_grid_spec spec;
    dsm_carve_params params;
    uint32_t flags = 0;
    dsm::GridDims d = {};       // of spec
    uint32_t *d_free = nullptr; // the accumulated set, [nz][ny][wx]
    uint32_t *d_occ = nullptr;  // dsm_surfel_map_space: the occupied set of the same spec (allocated at its first call)
    uint8_t *d_tmp = nullptr;   // dsm_surfel_map_space with host planes: their device staging, grow-only
    size_t tmp_bytes = 0;
    int64_t n_free = 0;
    int64_t frames = 0; // frames carved since the set was last cleared
};

#define SPACE_HIP(m, call)                                                                                     \
    do {                                                                                                       \
        const hipError_t e_ = (call);                                                                          \
        if (e_ != hipSuccess) return fail(m, DSM_E_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

void release(dsm_surfel_map *m) {
    Space *s = (Space *)m->space;
    if (!s) return;
    if (hipSetDevice(m->cfg.device) == hipSuccess) {
        if (s->d_free) (void)hipFree(s->d_free);
        if (s->d_occ) (void)hipFree(s->d_occ);
        if (s->d_tmp) (void)hipFree(s->d_tmp);
    }
    delete s;
    m->space = nullptr;
    m->on_carve = nullptr;
    m->on_warped = nullptr;
    m->release_space = nullptr;
}

int clear(dsm_surfel_map *m, Space *s) {
    SPACE_HIP(m, hipSetDevice(m->cfg.device));
    SPACE_HIP(m, hipMemset(s->d_free, 0, s->d.set_bytes()));
    s->n_free = 0;
    s->frames = 0;
    return DSM_OK;
}

// the fuse site of synchronize_msgs: m->last is the frame just fused
int carve_fused(dsm_surfel_map *m) {
    Space *s = (Space *)m->space;
    const int32_t slot = m->last.slot;
    const int rc = dsm_grid_carve(m->engine, &s->spec, &s->params, s->flags, 1, &slot, m->last.pose16, nullptr, s->d_free, &s->n_free);
    if (rc) return fail(m, rc, "dsm_grid_carve: %s", dsm_last_error(m->engine));
    s->frames++;
    return DSM_OK;
}

// after warp_surfels: what was carved with the old poses is stale
int warped(dsm_surfel_map *m) {
    Space *s = (Space *)m->space;
    m->free_space_resets++;
    return clear(m, s);
}

// what dsm_grid_carve would refuse of these, before anything is changed
const char *request_error(const dsm_grid_spec *spec, const dsm_carve_params *p, uint32_t flags) {
    if (spec->struct_size != sizeof(dsm_grid_spec)) return "dsm_grid_spec struct_size";
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(spec->origin[a])) return "grid origin not finite";
    if (!std::isfinite(spec->voxel) || !(spec->voxel > 0.0f)) return "grid voxel not finite or not positive";
    if (spec->nx < 1 || spec->ny < 1 || spec->nz < 1) return "a grid dimension below 1";
    if (!dsm::grid_dims_ok(spec->nx, spec->ny, spec->nz)) return "more than 2^28 voxels";
    if (spec->inflate < 0 || spec->inflate > dsm::kGridMaxInflate) return "grid inflate outside 0..16";
    if (p->struct_size != sizeof(dsm_carve_params)) return "dsm_carve_params struct_size";
    if (!(p->near_dist > 0.0f) || !(p->near_dist < p->far_dist) || !std::isfinite(p->far_dist)) return "carve depth range";
    if (!(p->margin >= 0.0f) || !std::isfinite(p->margin)) return "carve margin";
    if (flags & ~(uint32_t)DSM_CARVE_TRUST_INFINITE) return "flags other than DSM_CARVE_TRUST_INFINITE";
    return nullptr;
}

// the accumulator, or null with the error set
Space *ready(dsm_surfel_map *m, int *rc) {
    if (!m->space) {
        *rc = fail(m, DSM_E_STATE, "free space is not switched on (dsm_surfel_map_set_free_space)");
        return nullptr;
    }
    if (!m->last.valid) {
        *rc = fail(m, DSM_E_STATE, "no frame fused yet");
        return nullptr;
    }
    return (Space *)m->space;
}

// the occupied set of `kind` in the accumulator's spec into s->d_occ (allocated at the first call): what dsm_surfel_map_space and
// dsm_surfel_map_frontier_clusters classify against the accumulated free set
int compose_occupied(dsm_surfel_map *m, Space *s, int kind, const char *what, int32_t *n_surfels) {
    int select = DSM_CLOUD_SELECT_NONE;
    std::vector<int32_t> begin, count;
    if (!render_runs(m, kind, select, begin, count)) return fail(m, DSM_E_INVALID, "%s kind %d", what, kind);
    SPACE_HIP(m, hipSetDevice(m->cfg.device));
    if (!s->d_occ) SPACE_HIP(m, hipMalloc((void **)&s->d_occ, s->d.set_bytes()));
    const dsm_grid_planes occupied = {s->d_occ, nullptr, nullptr, nullptr, 0};
    int32_t n = 0, cells = 0;
    const int rc = dsm_grid_compose(m->engine, select, (int32_t)begin.size(), begin.data(), count.data(), &s->spec, 0, &occupied, 1, &n, &cells);
    if (rc) return fail(m, rc, "dsm_grid_compose: %s", dsm_last_error(m->engine));
    if (n_surfels) *n_surfels = n;
    return DSM_OK;
}

// room for `bytes` of device staging in s->d_tmp (grow-only; growth drops the contents)
int tmp_reserve(dsm_surfel_map *m, Space *s, size_t bytes) {
    if (bytes <= s->tmp_bytes) return DSM_OK;
    if (s->d_tmp) (void)hipFree(s->d_tmp);
    s->d_tmp = nullptr;
    s->tmp_bytes = 0;
    SPACE_HIP(m, hipMalloc((void **)&s->d_tmp, bytes));
    s->tmp_bytes = bytes;
    return DSM_OK;
}

int space(dsm_surfel_map *m, int kind, const dsm_space_planes *planes, int on_device, int32_t *n_surfels, int32_t *n_frontier) {
    if (!m || !planes) return DSM_E_INVALID;
    int rc = DSM_OK;
    Space *s = ready(m, &rc);
    if (!s) return rc;
    if (!planes->state && !planes->known_free && !planes->frontier && !planes->cells) return fail(m, DSM_E_INVALID, "no output plane");
    if (planes->cells && planes->cells_cap < 0) return fail(m, DSM_E_INVALID, "cells_cap %d", planes->cells_cap);
    if ((rc = compose_occupied(m, s, kind, "space", n_surfels))) return rc;
    int32_t nf = 0;
    const int nx = s->d.nx, ny = s->d.ny, nz = s->d.nz;
    const size_t n_vox = (size_t)s->d.n_vox();
    if (on_device) {
        rc = dsm_grid_classify(m->engine, nx, ny, nz, s->d_occ, s->d_free, planes, &nf);
        if (n_frontier) *n_frontier = nf;
        return rc ? fail(m, rc, "dsm_grid_classify: %s", dsm_last_error(m->engine)) : DSM_OK;
    }
    // host planes: staged on the device, each part from a 256-byte boundary
    const size_t cap = planes->cells ? dsm::capped(planes->cells_cap, s->d.n_vox()) : 0;
    dsm::ScratchPlan plan(256);
    const size_t at_state = plan.take(planes->state != nullptr, n_vox);
    const size_t at_kf = plan.take(planes->known_free != nullptr, s->d.set_bytes());
    const size_t at_fr = plan.take(planes->frontier != nullptr, s->d.set_bytes());
    const size_t at_cells = plan.take(planes->cells != nullptr, (cap ? cap : 1) * sizeof(int32_t));
    if ((rc = tmp_reserve(m, s, plan.bytes()))) return rc;
    dsm_space_planes dev = {nullptr, nullptr, nullptr, nullptr, 0};
    if (planes->state) dev.state = s->d_tmp + at_state;
    if (planes->known_free) dev.known_free = (uint32_t *)(s->d_tmp + at_kf);
    if (planes->frontier) dev.frontier = (uint32_t *)(s->d_tmp + at_fr);
    if (planes->cells) { dev.cells = (int32_t *)(s->d_tmp + at_cells); dev.cells_cap = (int32_t)cap; }
    rc = dsm_grid_classify(m->engine, nx, ny, nz, s->d_occ, s->d_free, &dev, &nf);
    if (n_frontier) *n_frontier = nf;
    if (rc && rc != DSM_E_CAPACITY) return fail(m, rc, "dsm_grid_classify: %s", dsm_last_error(m->engine));
    if (planes->state) SPACE_HIP(m, hipMemcpy(planes->state, dev.state, n_vox, hipMemcpyDeviceToHost));
    if (planes->known_free) SPACE_HIP(m, hipMemcpy(planes->known_free, dev.known_free, s->d.set_bytes(), hipMemcpyDeviceToHost));
    if (planes->frontier) SPACE_HIP(m, hipMemcpy(planes->frontier, dev.frontier, s->d.set_bytes(), hipMemcpyDeviceToHost));
    const size_t n_out = dsm::capped(nf, (int64_t)cap);
    if (planes->cells && n_out) SPACE_HIP(m, hipMemcpy(planes->cells, dev.cells, n_out * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (planes->cells && nf > planes->cells_cap) return fail(m, DSM_E_CAPACITY, "%d frontier cells, room for %d", nf, planes->cells_cap);
    return DSM_OK;
}

// dsm_surfel_map_frontier_clusters: classify as space() does, then label the frontier (and, for reachability, the known-free set)
int frontier_clusters(dsm_surfel_map *m, int kind, const dsm_frontier_query *q, dsm_component *table, int32_t table_cap, int32_t *label, int on_device,
                      int32_t *n_clusters, int32_t *n_all, int32_t *from_root) {
    if (!m || !q || !n_clusters) return DSM_E_INVALID;
    int rc = DSM_OK;
    Space *s = ready(m, &rc);
    if (!s) return rc;
    if (q->struct_size != sizeof(dsm_frontier_query)) return fail(m, DSM_E_INVALID, "dsm_frontier_query struct_size %u, not %zu", q->struct_size, sizeof(dsm_frontier_query));
    if (q->connectivity != DSM_CONNECT_FACES && q->connectivity != DSM_CONNECT_ALL) return fail(m, DSM_E_INVALID, "frontier clusters: connectivity %d", q->connectivity);
    if (q->min_count < 1) return fail(m, DSM_E_INVALID, "frontier clusters: min_count %d", q->min_count);
    if (!table && !label) return fail(m, DSM_E_INVALID, "frontier clusters: no output");
    if (table && table_cap < 0) return fail(m, DSM_E_INVALID, "table_cap %d", table_cap);
    if (s->d.n_vox() > dsm::kFieldMaxVoxels) return fail(m, DSM_E_INVALID, "frontier clusters: more than 2^26 voxels");
    if ((rc = compose_occupied(m, s, kind, "frontier clusters", nullptr))) return rc;
    const int nx = s->d.nx, ny = s->d.ny, nz = s->d.nz;
    const size_t n_vox = (size_t)s->d.n_vox();
    const bool from = q->has_from != 0;
    const size_t cap = table ? dsm::capped(table_cap, s->d.n_vox()) : 0;
    // device staging, each part from a 256-byte boundary: the frontier, then for reachability the known-free set and its labels, then
    // what goes to host memory
    dsm::ScratchPlan plan(256);
    const size_t at_fr = plan.take(true, s->d.set_bytes());
    const size_t at_kf = plan.take(from, s->d.set_bytes());
    const size_t at_region = plan.take(from, n_vox * sizeof(int32_t));
    const size_t at_table = plan.take(table && !on_device, (cap ? cap : 1) * sizeof(dsm_component));
    const size_t at_label = plan.take(label && !on_device, n_vox * sizeof(int32_t));
    if ((rc = tmp_reserve(m, s, plan.bytes()))) return rc;
    uint32_t *frontier = (uint32_t *)(s->d_tmp + at_fr), *known_free = from ? (uint32_t *)(s->d_tmp + at_kf) : nullptr;
    int32_t *region = from ? (int32_t *)(s->d_tmp + at_region) : nullptr;
    const dsm_space_planes sp = {nullptr, known_free, frontier, nullptr, 0};
    int32_t nf = 0;
    rc = dsm_grid_classify(m->engine, nx, ny, nz, s->d_occ, s->d_free, &sp, &nf);
    if (rc) return fail(m, rc, "dsm_grid_classify: %s", dsm_last_error(m->engine));
    int32_t root = -1;
    if (from) {
        const dsm_component_planes rp = {region, nullptr, 0};
        int32_t n_regions = 0;
        rc = dsm_grid_components(m->engine, nx, ny, nz, DSM_CONNECT_FACES, 1, known_free, nullptr, &rp, &n_regions, nullptr);
        if (rc) return fail(m, rc, "dsm_grid_components: %s", dsm_last_error(m->engine));
        const int32_t i[3] = {dsm::comp_from_voxel(q->from[0], s->spec.origin[0], s->spec.voxel), dsm::comp_from_voxel(q->from[1], s->spec.origin[1], s->spec.voxel),
                              dsm::comp_from_voxel(q->from[2], s->spec.origin[2], s->spec.voxel)};
        if (i[0] >= 0 && i[0] < nx && i[1] >= 0 && i[1] < ny && i[2] >= 0 && i[2] < nz)
            SPACE_HIP(m, hipMemcpy(&root, region + ((size_t)i[2] * ny + i[1]) * nx + i[0], sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    dsm_component_planes cp = {label, table, table_cap};
    if (!on_device) {
        cp.label = label ? (int32_t *)(s->d_tmp + at_label) : nullptr;
        cp.table = table ? (dsm_component *)(s->d_tmp + at_table) : nullptr;
        cp.table_cap = (int32_t)cap;
    }
    int32_t n = 0, all = 0;
    rc = dsm_grid_components(m->engine, nx, ny, nz, q->connectivity, q->min_count, frontier, region, &cp, &n, &all);
    *n_clusters = n;
    if (n_all) *n_all = all;
    if (from_root) *from_root = root;
    if (rc && rc != DSM_E_CAPACITY) return fail(m, rc, "dsm_grid_components: %s", dsm_last_error(m->engine));
    if (!on_device) {
        const size_t n_out = dsm::capped(n, (int64_t)cap);
        if (table && n_out) SPACE_HIP(m, hipMemcpy(table, cp.table, n_out * sizeof(dsm_component), hipMemcpyDeviceToHost));
        if (label) SPACE_HIP(m, hipMemcpy(label, cp.label, n_vox * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    if (table && n > table_cap) return fail(m, DSM_E_CAPACITY, "%d frontier clusters, room for %d", n, table_cap);
    return DSM_OK;
}

// dsm_surfel_map_view_gain: classify as space() does, then score the poses against the two sets (and the frontier)
int view_gain(dsm_surfel_map *m, int kind, const dsm_view_query *q, int32_t n_poses, const float *poses16, dsm_view_score *scores, uint32_t *visible,
              int on_device) {
    if (!m || !q) return DSM_E_INVALID;
    int rc = DSM_OK;
    Space *s = ready(m, &rc);
    if (!s) return rc;
    if (q->struct_size != sizeof(dsm_view_query)) return fail(m, DSM_E_INVALID, "dsm_view_query struct_size %u, not %zu", q->struct_size, sizeof(dsm_view_query));
    if (q->target != DSM_VIEW_TARGET_NONE && q->target != DSM_VIEW_TARGET_FRONTIER) return fail(m, DSM_E_INVALID, "view gain: target %d", q->target);
    if (!scores && !visible) return fail(m, DSM_E_INVALID, "view gain: no output");
    if (!poses16 || n_poses < 1 || n_poses > DSM_VIEW_MAX_POSES) return fail(m, DSM_E_INVALID, "view gain: %d poses, outside 1..%d, or none given", n_poses, DSM_VIEW_MAX_POSES);
    if ((rc = compose_occupied(m, s, kind, "view gain", nullptr))) return rc;
    const int nx = s->d.nx, ny = s->d.ny, nz = s->d.nz;
    const bool frontier = q->target == DSM_VIEW_TARGET_FRONTIER, stage = visible && !on_device;
    const size_t set_bytes = s->d.set_bytes();
    // device staging, each part from a 256-byte boundary: the frontier, then the visible planes on their way to host memory
    dsm::ScratchPlan plan(256);
    const size_t at_fr = plan.take(frontier, set_bytes);
    const size_t at_vis = plan.take(stage, set_bytes * (size_t)n_poses);
    if ((rc = tmp_reserve(m, s, plan.bytes()))) return rc;
    uint32_t *d_frontier = frontier ? (uint32_t *)(s->d_tmp + at_fr) : nullptr;
    if (frontier) {
        const dsm_space_planes sp = {nullptr, nullptr, d_frontier, nullptr, 0};
        int32_t nf = 0;
        rc = dsm_grid_classify(m->engine, nx, ny, nz, s->d_occ, s->d_free, &sp, &nf);
        if (rc) return fail(m, rc, "dsm_grid_classify: %s", dsm_last_error(m->engine));
    }
    uint32_t *d_visible = stage ? (uint32_t *)(s->d_tmp + at_vis) : visible;
    rc = dsm_grid_view(m->engine, &s->spec, &q->camera, q->flags, n_poses, poses16, nullptr, s->d_occ, s->d_free, d_frontier, scores, on_device, d_visible);
    if (rc) return fail(m, rc, "dsm_grid_view: %s", dsm_last_error(m->engine));
    if (stage) SPACE_HIP(m, hipMemcpy(visible, d_visible, set_bytes * (size_t)n_poses, hipMemcpyDeviceToHost));
    return DSM_OK;
}

int free_space(dsm_surfel_map *m, void *dst, int on_device, int64_t *n_free) {
    if (!m || !dst) return DSM_E_INVALID;
    int rc = DSM_OK;
    Space *s = ready(m, &rc);
    if (!s) return rc;
    if (on_device && ((uintptr_t)dst & 3)) return fail(m, DSM_E_INVALID, "the destination is not 4-byte aligned");
    SPACE_HIP(m, hipSetDevice(m->cfg.device));
    SPACE_HIP(m, hipMemcpy(dst, s->d_free, s->d.set_bytes(), on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    if (on_device) SPACE_HIP(m, hipStreamSynchronize(nullptr));
    if (n_free) *n_free = s->n_free;
    return DSM_OK;
}

} // namespace

extern "C" {

int dsm_surfel_map_set_free_space(dsm_surfel_map *m, const dsm_grid_spec *spec, const dsm_carve_params *params, uint32_t flags) {
    if (!m) return DSM_E_INVALID;
    if (!spec) {
        release(m);
        return DSM_OK;
    }
    dsm_carve_params p;
    if (params) p = *params;
    else dsm_carve_params_init(&p);
    if (const char *bad = request_error(spec, &p, flags)) return fail(m, DSM_E_INVALID, "set_free_space: %s", bad);
    const dsm::GridDims d = dsm::grid_dims(spec->nx, spec->ny, spec->nz);
    if (hipSetDevice(m->cfg.device) != hipSuccess) return fail(m, DSM_E_HIP, "set_free_space: cannot select device %d", m->cfg.device);
    uint32_t *d_free = nullptr;
    SPACE_HIP(m, hipMalloc((void **)&d_free, d.set_bytes()));
    release(m); // (the old accumulator, if any: a new spec starts from an empty set)
    Space *s = new Space();
    s->spec = *spec;
    s->params = p;
    s->flags = flags;
    s->d = d;
    s->d_free = d_free;
    m->space = s;
    m->on_carve = carve_fused;
    m->on_warped = warped;
    m->release_space = release;
    return clear(m, s);
}

int64_t dsm_surfel_map_free_space_resets(const dsm_surfel_map *m) { return m ? m->free_space_resets : 0; }

int dsm_surfel_map_free_space(dsm_surfel_map *m, uint32_t *free_out, int64_t *n_free) { return free_space(m, free_out, 0, n_free); }

int dsm_surfel_map_free_space_device(dsm_surfel_map *m, void *free_device, int64_t *n_free) { return free_space(m, free_device, 1, n_free); }

int dsm_surfel_map_space(dsm_surfel_map *m, int kind, const dsm_space_planes *planes, int32_t *n_surfels, int32_t *n_frontier) {
    return space(m, kind, planes, 0, n_surfels, n_frontier);
}

int dsm_surfel_map_space_device(dsm_surfel_map *m, int kind, const dsm_space_planes *planes_device, int32_t *n_surfels, int32_t *n_frontier) {
    return space(m, kind, planes_device, 1, n_surfels, n_frontier);
}

void dsm_frontier_query_init(dsm_frontier_query *q) {
    if (!q) return;
    memset(q, 0, sizeof *q);
    q->struct_size = (uint32_t)sizeof(dsm_frontier_query);
    q->connectivity = DSM_CONNECT_ALL;
    q->min_count = 1;
}

int dsm_surfel_map_frontier_clusters(dsm_surfel_map *m, int kind, const dsm_frontier_query *q, dsm_component *table, int32_t table_cap, int32_t *label,
                                     int32_t *n_clusters, int32_t *n_all, int32_t *from_root) {
    return frontier_clusters(m, kind, q, table, table_cap, label, 0, n_clusters, n_all, from_root);
}

int dsm_surfel_map_frontier_clusters_device(dsm_surfel_map *m, int kind, const dsm_frontier_query *q, dsm_component *table_device, int32_t table_cap,
                                            int32_t *label_device, int32_t *n_clusters, int32_t *n_all, int32_t *from_root) {
    return frontier_clusters(m, kind, q, table_device, table_cap, label_device, 1, n_clusters, n_all, from_root);
}

void dsm_view_query_init(const dsm_surfel_map *m, dsm_view_query *q) {
    if (!q) return;
    memset(q, 0, sizeof *q);
    q->struct_size = (uint32_t)sizeof(dsm_view_query);
    q->target = DSM_VIEW_TARGET_FRONTIER;
    if (!m) return;
    dsm_carve_params p;
    if (m->space) p = ((const Space *)m->space)->params;
    else dsm_carve_params_init(&p);
    q->camera.width = m->cfg.cam_width;
    q->camera.height = m->cfg.cam_height;
    q->camera.fx = m->cfg.cam_fx;
    q->camera.fy = m->cfg.cam_fy;
    q->camera.cx = m->cfg.cam_cx;
    q->camera.cy = m->cfg.cam_cy;
    q->camera.near_dist = p.near_dist;
    q->camera.far_dist = p.far_dist;
}

int dsm_surfel_map_view_gain(dsm_surfel_map *m, int kind, const dsm_view_query *q, int32_t n_poses, const float *poses16, dsm_view_score *scores,
                             uint32_t *visible) {
    return view_gain(m, kind, q, n_poses, poses16, scores, visible, 0);
}

int dsm_surfel_map_view_gain_device(dsm_surfel_map *m, int kind, const dsm_view_query *q, int32_t n_poses, const float *poses16,
                                    dsm_view_score *scores_device, uint32_t *visible_device) {
    return view_gain(m, kind, q, n_poses, poses16, scores_device, visible_device, 1);
}

int dsm_surfel_map_carve_last(dsm_surfel_map *m, const dsm_grid_spec *spec, const dsm_carve_params *params, uint32_t flags, void *free_device) {
    if (!m || !spec || !free_device) return DSM_E_INVALID;
    if (!m->last.valid) return fail(m, DSM_E_STATE, "no frame fused yet");
    dsm_carve_params p;
    if (params) p = *params;
    else dsm_carve_params_init(&p);
    const int32_t slot = m->last.slot;
    const int rc = dsm_grid_carve(m->engine, spec, &p, flags, 1, &slot, m->last.pose16, nullptr, free_device, nullptr);
    return rc ? fail(m, rc, "dsm_grid_carve: %s", dsm_last_error(m->engine)) : DSM_OK;
}

} // extern "C"
