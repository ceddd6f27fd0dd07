// dsm_surfel_map_mesh.cpp -- the node's hexagon mesh as a device product (include/dsm_surfel_map.h: dsm_surfel_map_get_mesh*,
// dsm_surfel_map_save_mesh_binary) over the engine's dsm_mesh_compose.  Line numbers refer to the reference's
// surfel_fusion/src/surfel_map.cpp.  A translation unit of its own, like dsm_surfel_map_clouds.cpp: dsm_surfel_map.cpp (and
// its ASCII dsm_surfel_map_save_mesh) links against the engine entry points it always used.
#include "dsm_surfel_map_node.h"
#include "dsm_mesh_ply.h"

#include <cstdio>

namespace {

using namespace dsm_node;

// the attached surfels, then the active ones with update_times >= 5 (:1240-1248)
int build_mesh(dsm_surfel_map *m, int layout, void *dst, int on_device, int32_t cap, int32_t *n) {
    if (!m->last.valid) return fail(m, DSM_E_STATE, "no frame fused yet");
    std::vector<int32_t> begin, count;
    attached_runs(m, begin, count);
    const int rc = dsm_mesh_compose(m->engine, DSM_CLOUD_SELECT_MATURE, (int32_t)begin.size(), begin.data(), count.data(), layout, dst, on_device,
                                    cap, n);
    return rc ? engine_fail(m, rc, "dsm_mesh_compose") : DSM_OK;
}

struct HostBlock { // page-locked: the device-to-host copy of a chunk is one DMA
    void *p = nullptr;
    ~HostBlock() {
        if (p) dsm_host_free(p);
    }
};

struct File {
    std::FILE *f = nullptr;
    ~File() {
        if (f) std::fclose(f);
    }
};

constexpr int32_t kChunkSurfels = 1 << 18; // 24 MiB of DSM_MESH_VERTEX_XYZ_RGBA8 vertices

} // namespace

extern "C" {

int dsm_surfel_map_get_mesh(dsm_surfel_map *m, int vertex_layout, void *out, int32_t cap_surfels, int32_t *n_surfels) {
    if (!m || !n_surfels || cap_surfels < 0 || (cap_surfels && !out)) return DSM_E_INVALID;
    return build_mesh(m, vertex_layout, out, 0, cap_surfels, n_surfels);
}

int dsm_surfel_map_get_mesh_device(dsm_surfel_map *m, int vertex_layout, void *dst_device, int32_t cap_surfels, int32_t *n_surfels) {
    if (!m || !n_surfels || cap_surfels < 0 || (cap_surfels && !dst_device)) return DSM_E_INVALID;
    return build_mesh(m, vertex_layout, dst_device, 1, cap_surfels, n_surfels);
}

int dsm_surfel_map_save_mesh_binary(dsm_surfel_map *m, const char *path) {
    if (!m || !path) return DSM_E_INVALID;
    if (!m->last.valid) return fail(m, DSM_E_STATE, "no frame fused yet");
    std::vector<int32_t> begin, count;
    attached_runs(m, begin, count);
    int64_t n_attached = 0;
    for (int32_t c : count) n_attached += c;
    // how many active surfels are mature: a compose with no room returns the count and writes nothing
    int32_t n_active = 0;
    int rc = dsm_mesh_compose(m->engine, DSM_CLOUD_SELECT_MATURE, 0, nullptr, nullptr, DSM_MESH_VERTEX_XYZ_RGBA8, nullptr, 0, 0, &n_active);
    if (rc && rc != DSM_E_CAPACITY) return engine_fail(m, rc, "dsm_mesh_compose");
    const int64_t n_surfels = n_attached + n_active;
    if (n_surfels * 6 > INT32_MAX) return fail(m, DSM_E_INVALID, "%lld surfels: the PLY's int vertex_index cannot address them", (long long)n_surfels);
    // one page-locked block: a chunk of the attached surfels, or the whole active part (the engine composes the map part in
    // one piece) -- no larger than either needs
    int64_t chunk_cap = n_attached < kChunkSurfels ? n_attached : kChunkSurfels;
    if (chunk_cap < n_active) chunk_cap = n_active;
    HostBlock block;
    if (chunk_cap > 0 && (rc = dsm_host_alloc(&block.p, (size_t)chunk_cap * 96)))
        return fail(m, rc, "no page-locked memory for %lld surfels of vertices", (long long)chunk_cap);
    // the file is opened only now: an engine or allocation failure above leaves the path untouched; a failure below removes it
    File file;
    file.f = std::fopen(path, "wb");
    if (!file.f) return fail(m, DSM_E_INVALID, "cannot open %s", path);
    struct Unlink {
        const char *path;
        bool keep = false;
        ~Unlink() {
            if (!keep) std::remove(path);
        }
    } partial{path};
    std::vector<uint8_t> scratch;
    bool ok = dsm_mesh_ply::write_header(file.f, (uint64_t)n_surfels);
    // the attached surfels: the runs cut into chunks of at most kChunkSurfels
    std::vector<int32_t> cb, cc;
    int32_t in_chunk = 0;
    auto flush = [&](int select) -> int {
        if (cb.empty() && select == DSM_CLOUD_SELECT_NONE) return DSM_OK;
        int32_t got = 0;
        const int r = dsm_mesh_compose(m->engine, select, (int32_t)cb.size(), cb.data(), cc.data(), DSM_MESH_VERTEX_XYZ_RGBA8, block.p, 0,
                                       (int32_t)chunk_cap, &got);
        if (r) return engine_fail(m, r, "dsm_mesh_compose");
        ok = ok && dsm_mesh_ply::write_vertices(file.f, block.p, (size_t)got * 6, scratch);
        cb.clear();
        cc.clear();
        in_chunk = 0;
        return DSM_OK;
    };
    auto finish = [&](int code) { // close before the guard removes a partial file
        std::fclose(file.f);
        file.f = nullptr;
        return code;
    };
    for (size_t s = 0; s < begin.size(); s++) {
        int32_t b = begin[s], c = count[s];
        while (c > 0) {
            const int32_t take = c < kChunkSurfels - in_chunk ? c : kChunkSurfels - in_chunk;
            cb.push_back(b);
            cc.push_back(take);
            b += take;
            c -= take;
            in_chunk += take;
            if (in_chunk == kChunkSurfels && (rc = flush(DSM_CLOUD_SELECT_NONE))) return finish(rc);
        }
    }
    if ((rc = flush(DSM_CLOUD_SELECT_NONE))) return finish(rc);
    // the active surfels with update_times >= 5, one chunk
    if (n_active > 0 && (rc = flush(DSM_CLOUD_SELECT_MATURE))) return finish(rc);
    ok = ok && dsm_mesh_ply::write_faces(file.f, (uint64_t)n_surfels, scratch);
    std::FILE *f = file.f;
    file.f = nullptr;
    ok = (std::fclose(f) == 0) && ok;
    if (!ok) return fail(m, DSM_E_INVALID, "write to %s failed", path);
    partial.keep = true;
    return DSM_OK;
}

} // extern "C"
