// dsm_components.h -- connected components of a bit set in the grid layout (dsm_grid_components): what the kernels of
// dsm_k_components.h, the node (dsm_surfel_map_frontier_clusters) and the host checker tests/components_host.cpp share, and
// nothing else: the record, the adjacency rule and the voxel a world point lies in.  Plain C++ with no device side of its own.
//
// Two set voxels are adjacent when both lie inside the grid and their offset passes comp_adjacent.  A component is a class of the
// transitive closure; it is named by the lowest linear index (z ny + y) nx + x of its voxels.  Every statistic is an integer sum,
// minimum, maximum or count over the component, so no order of execution can show in a result.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/dsm.h"

#if defined(__HIPCC__) || defined(__HIP__)
#define DSM_COMP_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define DSM_COMP_HD static inline
#endif

namespace dsm {

constexpr int kConnectFaces = DSM_CONNECT_FACES, kConnectAll = DSM_CONNECT_ALL;

static_assert(sizeof(dsm_component) == 64, "dsm_component is 64 bytes");

// is the offset (dx, dy, dz), each in -1..1, an adjacency of this connectivity?
DSM_COMP_HD constexpr bool comp_adjacent(int dx, int dy, int dz, int connectivity) {
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
    const int sum = ax + ay + az, mx = ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az);
    return connectivity == kConnectFaces ? sum == 1 : (connectivity == kConnectAll && mx == 1);
}

// the voxel index of world coordinate `from` along one axis: floor of the quotient in double.  It may lie outside the grid, and
// is clamped to the int range so that it can be compared with the dimensions.
DSM_COMP_HD int32_t comp_from_voxel(float from, float origin, float voxel) {
    const double q = floor(((double)from - (double)origin) / (double)voxel);
    if (!(q > -2147483648.0)) return INT32_MIN; // (a NaN lands here: outside every grid)
    if (!(q < 2147483647.0)) return INT32_MAX;
    return (int32_t)q;
}

// a component with nothing accumulated yet
DSM_COMP_HD void comp_init(dsm_component &c, int32_t root, int32_t tag) {
    c.root = root;
    c.count = 0;
    c.tag = tag;
    c.reserved = 0;
    for (int a = 0; a < 3; a++) {
        c.sum[a] = 0;
        c.lo[a] = INT32_MAX;
        c.hi[a] = -1;
    }
}

} // namespace dsm
