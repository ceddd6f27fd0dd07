// components_host.cpp -- connected components of a bit set on the host (tests/test_cpu_components.py,
// tests/test_gpu_components.py): the definition of include/dsm.h evaluated directly, with none of the arrangements of
// csrc/dsm_k_components.h.  It shares csrc/dsm_components.h with the product -- the record, the adjacency rule, the voxel of a
// world point -- and nothing else.  Two independent forms:
//   form 0   a breadth-first flood fill started at every unlabelled set voxel in ascending linear order, so that the start IS the
//            component's lowest index; the statistics are taken voxel by voxel as the fill reaches them
//   form 1   a sequential union-find (union by lowest index, no path tricks beyond halving) over the voxels in ascending order,
//            each against its adjacent set voxels of lower index; labels by a find per voxel, the statistics in a second sweep
// Build: g++ -std=c++17 -O2 -shared -fPIC.  With -DCOMPONENTS_HOST_MAIN the file is a program: for every case file named on the
// command line (tests/components_cases.py's write_case) it runs both forms and compares labels, tables and counts; it prints one
// line and exits with status 0 iff everything agrees (run under the sanitizers by the tests).
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../densesurfelmapping_amd/csrc/dsm_components.h"

namespace {

struct Grid {
    const uint32_t *bits;
    int nx, ny, nz, wx;
    bool inside(int x, int y, int z) const { return x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz; }
    bool set(int x, int y, int z) const { return (bits[((size_t)z * ny + y) * wx + (x >> 5)] >> (x & 31)) & 1u; } // x < nx: never a pad bit
    int64_t lin(int x, int y, int z) const { return ((int64_t)z * ny + y) * nx + x; }
};

void add_voxel(dsm_component &c, int x, int y, int z) {
    const int p[3] = {x, y, z};
    c.count++;
    for (int a = 0; a < 3; a++) {
        c.sum[a] += p[a];
        if (p[a] < c.lo[a]) c.lo[a] = p[a];
        if (p[a] > c.hi[a]) c.hi[a] = p[a];
    }
}

// every component, ascending by root; label: [voxels]
void flood(const Grid &g, int conn, const int32_t *tags, int32_t *label, std::vector<dsm_component> &all) {
    const int64_t n_vox = (int64_t)g.nx * g.ny * g.nz;
    for (int64_t i = 0; i < n_vox; i++) label[i] = -1;
    std::vector<int32_t> queue;
    for (int z0 = 0; z0 < g.nz; z0++)
        for (int y0 = 0; y0 < g.ny; y0++)
            for (int x0 = 0; x0 < g.nx; x0++) {
                const int64_t root = g.lin(x0, y0, z0);
                if (!g.set(x0, y0, z0) || label[root] >= 0) continue;
                dsm_component c;
                dsm::comp_init(c, (int32_t)root, tags ? tags[root] : 0);
                queue.clear();
                queue.push_back((int32_t)root);
                label[root] = (int32_t)root;
                for (size_t head = 0; head < queue.size(); head++) {
                    const int32_t v = queue[head];
                    const int x = v % g.nx, y = (v / g.nx) % g.ny, z = v / (g.nx * g.ny);
                    add_voxel(c, x, y, z);
                    for (int dz = -1; dz <= 1; dz++)
                        for (int dy = -1; dy <= 1; dy++)
                            for (int dx = -1; dx <= 1; dx++) {
                                if (!dsm::comp_adjacent(dx, dy, dz, conn) || !g.inside(x + dx, y + dy, z + dz) || !g.set(x + dx, y + dy, z + dz)) continue;
                                const int64_t w = g.lin(x + dx, y + dy, z + dz);
                                if (label[w] >= 0) continue;
                                label[w] = (int32_t)root;
                                queue.push_back((int32_t)w);
                            }
                }
                all.push_back(c);
            }
}

int32_t uf_find(std::vector<int32_t> &parent, int32_t v) {
    while (parent[v] != v) {
        parent[v] = parent[parent[v]];
        v = parent[v];
    }
    return v;
}

void union_find(const Grid &g, int conn, const int32_t *tags, int32_t *label, std::vector<dsm_component> &all) {
    const int64_t n_vox = (int64_t)g.nx * g.ny * g.nz;
    std::vector<int32_t> parent((size_t)n_vox);
    for (int64_t i = 0; i < n_vox; i++) parent[i] = (int32_t)i;
    for (int z = 0; z < g.nz; z++)
        for (int y = 0; y < g.ny; y++)
            for (int x = 0; x < g.nx; x++) {
                if (!g.set(x, y, z)) continue;
                const int64_t v = g.lin(x, y, z);
                for (int dz = -1; dz <= 1; dz++)
                    for (int dy = -1; dy <= 1; dy++)
                        for (int dx = -1; dx <= 1; dx++) {
                            if (!dsm::comp_adjacent(dx, dy, dz, conn) || !g.inside(x + dx, y + dy, z + dz) || !g.set(x + dx, y + dy, z + dz)) continue;
                            const int64_t w = g.lin(x + dx, y + dy, z + dz);
                            if (w > v) continue;
                            const int32_t a = uf_find(parent, (int32_t)v), b = uf_find(parent, (int32_t)w);
                            if (a < b) parent[b] = a;
                            else parent[a] = b;
                        }
            }
    std::vector<int32_t> slot((size_t)n_vox, -1);
    for (int z = 0; z < g.nz; z++)
        for (int y = 0; y < g.ny; y++)
            for (int x = 0; x < g.nx; x++) {
                const int64_t v = g.lin(x, y, z);
                if (!g.set(x, y, z)) {
                    label[v] = -1;
                    continue;
                }
                const int32_t r = uf_find(parent, (int32_t)v);
                label[v] = r;
                if (r == v) { // a root comes before every other voxel of its component
                    dsm_component c;
                    dsm::comp_init(c, r, tags ? tags[r] : 0);
                    slot[r] = (int32_t)all.size();
                    all.push_back(c);
                }
                add_voxel(all[(size_t)slot[r]], x, y, z);
            }
}

} // namespace

extern "C" {

// label: [voxels] or null; table: [cap] or null -- no entry is written at or beyond cap; *n_all (may be null) = all components.
// Returns the number of components with count >= min_count.
int32_t components_host(const uint32_t *bits, int nx, int ny, int nz, int conn, int min_count, const int32_t *tags, int form, int32_t *label,
                        dsm_component *table, int32_t cap, int32_t *n_all) {
    const Grid g = {bits, nx, ny, nz, (nx + 31) / 32};
    std::vector<int32_t> own;
    if (!label) {
        own.resize((size_t)nx * ny * nz);
        label = own.data();
    }
    std::vector<dsm_component> all;
    if (form == 0) flood(g, conn, tags, label, all);
    else union_find(g, conn, tags, label, all);
    if (n_all) *n_all = (int32_t)all.size();
    int32_t kept = 0;
    for (const dsm_component &c : all) {
        if (c.count < min_count) continue;
        if (table && kept < cap) table[kept] = c;
        kept++;
    }
    return kept;
}

void components_host_from_voxel(const float *from, const float *origin, float voxel, int32_t *out) {
    for (int a = 0; a < 3; a++) out[a] = dsm::comp_from_voxel(from[a], origin[a], voxel);
}

// sizeof(dsm_component), then the offsets of root, count, sum, lo, hi, tag, reserved
void components_host_layout(int32_t *out) {
    out[0] = (int32_t)sizeof(dsm_component);
    out[1] = (int32_t)offsetof(dsm_component, root);
    out[2] = (int32_t)offsetof(dsm_component, count);
    out[3] = (int32_t)offsetof(dsm_component, sum);
    out[4] = (int32_t)offsetof(dsm_component, lo);
    out[5] = (int32_t)offsetof(dsm_component, hi);
    out[6] = (int32_t)offsetof(dsm_component, tag);
    out[7] = (int32_t)offsetof(dsm_component, reserved);
}

} // extern "C"

#ifdef COMPONENTS_HOST_MAIN
// a case file: int32 nx, ny, nz, connectivity, min_count, has_tags; the words; the tag plane if has_tags
int main(int argc, char **argv) {
    int cases = 0;
    for (int k = 1; k < argc; k++) {
        FILE *f = fopen(argv[k], "rb");
        if (!f) { fprintf(stderr, "cannot open %s\n", argv[k]); return 2; }
        int32_t hd[6];
        if (fread(hd, sizeof(int32_t), 6, f) != 6) { fprintf(stderr, "%s: short header\n", argv[k]); fclose(f); return 2; }
        const int nx = hd[0], ny = hd[1], nz = hd[2], conn = hd[3], min_count = hd[4];
        const size_t n_words = (size_t)((nx + 31) / 32) * ny * nz, n_vox = (size_t)nx * ny * nz;
        std::vector<uint32_t> bits(n_words);
        std::vector<int32_t> tags(hd[5] ? n_vox : 0);
        if (fread(bits.data(), sizeof(uint32_t), n_words, f) != n_words || (hd[5] && fread(tags.data(), sizeof(int32_t), n_vox, f) != n_vox)) {
            fprintf(stderr, "%s: short body\n", argv[k]);
            fclose(f);
            return 2;
        }
        fclose(f);
        std::vector<int32_t> label[2] = {std::vector<int32_t>(n_vox), std::vector<int32_t>(n_vox)};
        std::vector<dsm_component> table[2];
        int32_t kept[2], all[2];
        for (int form = 0; form < 2; form++) {
            kept[form] = components_host(bits.data(), nx, ny, nz, conn, min_count, hd[5] ? tags.data() : nullptr, form, label[form].data(), nullptr, 0, &all[form]);
            table[form].resize((size_t)kept[form]);
            if (!table[form].empty()) memset(table[form].data(), 0, table[form].size() * sizeof(dsm_component));
            components_host(bits.data(), nx, ny, nz, conn, min_count, hd[5] ? tags.data() : nullptr, form, nullptr, table[form].data(), kept[form], nullptr);
        }
        if (kept[0] != kept[1] || all[0] != all[1] || label[0] != label[1] ||
            (!table[0].empty() && memcmp(table[0].data(), table[1].data(), table[0].size() * sizeof(dsm_component)) != 0)) {
            printf("components_host: %s: the two forms differ (%d / %d kept, %d / %d in all)\n", argv[k], kept[0], kept[1], all[0], all[1]);
            return 1;
        }
        cases++;
    }
    printf("components_host: %d cases, the flood fill and the union-find agree\n", cases);
    return 0;
}
#endif
