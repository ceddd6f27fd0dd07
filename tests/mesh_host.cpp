// mesh_host.cpp -- the mesh arithmetic and writers compiled for the host (tests/test_cpu_mesh.py, tests/test_gpu_mesh.py):
//   mesh_host_vertices   surfel_hexagon of csrc/dsm_math.h -- the function the HIP kernels of csrc/dsm_k_mesh.h call --
//                        laid out as the two vertex layouts of include/dsm.h
//   mesh_host_print      a REF6 buffer printed as SurfelMap::save_mesh prints `vertexs` (ostream << float at the default
//                        precision, then the face lines; surfel_fusion/src/surfel_map.cpp:1250-1280 of the reference)
//   mesh_host_ply_binary the binary PLY writer of csrc/dsm_mesh_ply.h on a caller's XYZ_RGBA8 buffer
// Build: g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <vector>

#include "../densesurfelmapping_amd/csrc/dsm_math.h"
#include "../densesurfelmapping_amd/csrc/dsm_mesh_ply.h"
#include "../include/dsm.h"

extern "C" {

void mesh_host_vertices(const dsm_surfel *s, int64_t n, int layout, float *out) {
    for (int64_t i = 0; i < n; i++) {
        float pt[6][3];
        int ic;
        dsm::surfel_hexagon(s[i], pt, ic);
        if (layout == DSM_MESH_VERTEX_REF6) {
            float *o = out + i * 36;
            for (int k = 0; k < 6; k++) {
                for (int d = 0; d < 3; d++) o[6 * k + d] = pt[k][d];
                for (int d = 3; d < 6; d++) o[6 * k + d] = (float)ic;
            }
        } else {
            float *o = out + i * 24;
            const uint32_t b = dsm::surfel_color_byte(ic), rgba = b | (b << 8) | (b << 16) | 0xff000000u;
            for (int k = 0; k < 6; k++) {
                for (int d = 0; d < 3; d++) o[4 * k + d] = pt[k][d];
                memcpy(&o[4 * k + 3], &rgba, 4);
            }
        }
    }
}

int mesh_host_color_int(float color) { return dsm::surfel_color_int(color); }

int mesh_host_print(const char *path, const float *vertexs, int64_t n_surfels) {
    std::ofstream stream(path);
    if (!stream) return -1;
    const size_t numPoints = (size_t)n_surfels * 6, numSurfels = (size_t)n_surfels;
    stream << "ply\nformat ascii 1.0\nelement vertex " << numPoints << "\nproperty float x\nproperty float y\nproperty float z\n"
           << "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face " << numSurfels * 4
           << "\nproperty list uchar int vertex_index\nend_header\n";
    for (size_t i = 0; i < numPoints; i++) {
        for (int j = 0; j < 6; j++) stream << vertexs[i * 6 + (size_t)j] << " ";
        stream << "\n";
    }
    for (size_t i = 0; i < numSurfels; i++) {
        const size_t p1 = i * 6, p2 = i * 6 + 1, p3 = i * 6 + 2, p4 = i * 6 + 3, p5 = i * 6 + 4, p6 = i * 6 + 5;
        stream << "3 " << p1 << " " << p2 << " " << p3 << "\n";
        stream << "3 " << p2 << " " << p4 << " " << p3 << "\n";
        stream << "3 " << p3 << " " << p4 << " " << p5 << "\n";
        stream << "3 " << p5 << " " << p4 << " " << p6 << "\n";
    }
    stream.close();
    return stream ? 0 : -1;
}

int mesh_host_ply_binary(const char *path, const void *xyz_rgba8, int64_t n_surfels) {
    std::FILE *f = std::fopen(path, "wb");
    if (!f) return -1;
    std::vector<uint8_t> scratch;
    bool ok = dsm_mesh_ply::write_header(f, (uint64_t)n_surfels);
    ok = ok && dsm_mesh_ply::write_vertices(f, xyz_rgba8, (size_t)n_surfels * 6, scratch);
    ok = ok && dsm_mesh_ply::write_faces(f, (uint64_t)n_surfels, scratch);
    return (std::fclose(f) == 0 && ok) ? 0 : -1;
}

} // extern "C"
