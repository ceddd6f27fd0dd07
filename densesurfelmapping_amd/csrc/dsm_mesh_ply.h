// dsm_mesh_ply.h -- the binary PLY of dsm_surfel_map_save_mesh_binary, host code only (no engine call: tests/mesh_host.cpp
// runs it on a hand-made vertex buffer).  Same elements and properties as the ASCII file of SurfelMap::save_mesh
// (surfel_fusion/src/surfel_map.cpp:1250-1278 of the reference), `format binary_little_endian 1.0`: a vertex is three floats
// and three uchar (15 bytes), a face is the uchar 3 and three int (13 bytes).  Little-endian hosts only.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace dsm_mesh_ply {

inline bool write_header(std::FILE *f, uint64_t n_surfels) {
    return std::fprintf(f,
                        "ply\nformat binary_little_endian 1.0\nelement vertex %llu\nproperty float x\nproperty float y\nproperty float z\n"
                        "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face %llu\n"
                        "property list uchar int vertex_index\nend_header\n",
                        (unsigned long long)(n_surfels * 6), (unsigned long long)(n_surfels * 4)) > 0;
}

// n_vertices vertices of the DSM_MESH_VERTEX_XYZ_RGBA8 layout (16 bytes: x y z, r g b 255): the first 15 bytes of each
inline bool write_vertices(std::FILE *f, const void *xyz_rgba8, size_t n_vertices, std::vector<uint8_t> &scratch) {
    const size_t kBlock = 1 << 16;
    const uint8_t *src = (const uint8_t *)xyz_rgba8;
    scratch.resize(kBlock * 15);
    for (size_t v0 = 0; v0 < n_vertices; v0 += kBlock) {
        const size_t nv = n_vertices - v0 < kBlock ? n_vertices - v0 : kBlock;
        for (size_t v = 0; v < nv; v++) std::memcpy(&scratch[v * 15], src + (v0 + v) * 16, 15);
        if (std::fwrite(scratch.data(), 15, nv, f) != nv) return false;
    }
    return true;
}

// the four faces of each of n_surfels hexagons (:1270-1278): (p1 p2 p3) (p2 p4 p3) (p3 p4 p5) (p5 p4 p6), p1 = 6 i
inline bool write_faces(std::FILE *f, uint64_t n_surfels, std::vector<uint8_t> &scratch) {
    static const int32_t kCorner[12] = {0, 1, 2, 1, 3, 2, 2, 3, 4, 4, 3, 5};
    const uint64_t kBlock = 1 << 14;
    scratch.resize(kBlock * 4 * 13);
    for (uint64_t i0 = 0; i0 < n_surfels; i0 += kBlock) {
        const uint64_t ns = n_surfels - i0 < kBlock ? n_surfels - i0 : kBlock;
        uint8_t *o = scratch.data();
        for (uint64_t i = i0; i < i0 + ns; i++)
            for (int t = 0; t < 4; t++) {
                *o++ = 3;
                for (int k = 0; k < 3; k++) {
                    const int32_t idx = (int32_t)(i * 6) + kCorner[3 * t + k];
                    std::memcpy(o, &idx, 4);
                    o += 4;
                }
            }
        if (std::fwrite(scratch.data(), 13, (size_t)ns * 4, f) != (size_t)ns * 4) return false;
    }
    return true;
}

} // namespace dsm_mesh_ply
