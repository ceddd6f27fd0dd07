// dsm_carve.h -- free space carved out of the voxel grid by depth frames (dsm_grid_carve), and the three-state map with its
// frontier (dsm_grid_classify): the definitions, shared by the kernels of dsm_k_carve.h and the host checker
// tests/space_host.cpp.  Included at the end of dsm_math.h (it uses grid_centre, xform_point and round_to_pixel).
//
// Carving is defined PER VOXEL, so no order of execution can matter: the centre of the voxel is taken into the camera frame of a
// depth frame, projected to the nearest pixel, and the voxel is seen through (FREE) iff its depth plus a margin is less than the
// depth measured at that pixel.  fp32, non-fused, in the order written; every parenthesis is part of the definition.  What the
// centre-sampling means: a voxel is judged by one ray, the one through its centre -- a voxel whose centre projects outside the
// image or onto a pixel without a measurement stays as it was, however much of its volume other pixels see through, and the
// margin is what keeps the voxels that hold the measured surface itself from being freed.  The part of the definition that needs
// no depth plane, carve_project, is also what dsm_view.h (dsm_grid_view) judges a voxel IN VIEW by.
#pragma once

namespace dsm {

constexpr int kCarveMaxFrames = 32;          // DSM_CARVE_MAX_FRAMES
constexpr uint32_t kCarveReplace = 1u;       // DSM_CARVE_REPLACE
constexpr uint32_t kCarveTrustInfinite = 2u; // DSM_CARVE_TRUST_INFINITE

enum CarveExit { kCarveFree = 0, kCarveRange = 1, kCarveOutside = 2, kCarveNoDepth = 3, kCarveInfinite = 4, kCarveNotInFront = 5 };

struct CarveConst {
    float origin[3];
    float voxel;
    int w, h, pitch;          // the frame: pixels per row and rows, elements from one row to the next (the pad columns are never read)
    float fx, fy, cx, cy;
    float near_d, far_d, margin;
    uint32_t flags;
    float inv[16];            // world -> camera, column-major
};

// steps 1-4 of the definition, the part that needs no depth plane (dsm_view.h judges IN VIEW by it with its own camera in c):
// kCarveRange, kCarveOutside, or kCarveFree for a centre that passes both, with its camera-frame depth and its pixel
DSM_HD CarveExit carve_project(const CarveConst &c, int x, int y, int z, float &qz, int &u, int &v) {
    const float p[3] = {grid_centre(c.origin[0], c.voxel, x), grid_centre(c.origin[1], c.voxel, y), grid_centre(c.origin[2], c.voxel, z)};
    float q[3];
    xform_point(c.inv, p, q);
    qz = q[2];
    if (!(c.near_d < q[2] && q[2] < c.far_d)) return kCarveRange; // (a NaN fails)
    u = round_to_pixel((q[0] * c.fx) / q[2] + c.cx);
    v = round_to_pixel((q[1] * c.fy) / q[2] + c.cy);
    if (!(0 <= u && u < c.w && 0 <= v && v < c.h)) return kCarveOutside;
    return kCarveFree;
}

// the exit of voxel (x, y, z) against one frame; `depth` = the frame's plane, [h][pitch]
DSM_HD CarveExit carve_voxel(const CarveConst &c, const float *depth, int x, int y, int z) {
    float qz;
    int u, v;
    const CarveExit e = carve_project(c, x, y, z, qz, u, v);
    if (e != kCarveFree) return e;
    const float d = depth[(int64_t)v * c.pitch + u];
    if (!(d > 0.0f)) return kCarveNoDepth; // (a NaN fails)
    if (d == __builtin_inff() && !(c.flags & kCarveTrustInfinite)) return kCarveInfinite;
    return (qz + c.margin) < d ? kCarveFree : kCarveNotInFront;
}

// ---- the three states.  occupied wins over free; pad bits of either set are ignored.
constexpr uint8_t kSpaceUnknown = 0, kSpaceFree = 1, kSpaceOccupied = 2; // DSM_SPACE_*

DSM_HD uint8_t space_state(bool occupied, bool free_) { return occupied ? kSpaceOccupied : free_ ? kSpaceFree : kSpaceUnknown; }

} // namespace dsm
