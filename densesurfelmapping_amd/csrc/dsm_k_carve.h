// dsm_k_carve.h -- free space carved out of the voxel grid by depth frames (dsm_grid_carve) and the three-state map with its
// frontier (dsm_grid_classify).  The definitions (carve_voxel, space_state) are in dsm_carve.h and shared with the host checker
// tests/space_host.cpp; this file is how they are evaluated:
//   k_carve            a wave per 64 voxels of a row, a lane per voxel.  The old word of the free set is loaded first (unless the
//                      call replaces it): a voxel that is free already skips the frames, and OR makes that exact.  The other
//                      voxels run carve_voxel against the frames in turn, inside the kernel, until one sees through them, so n
//                      frames cost one pass over the bit set.  A ballot packs the 64 lanes into two words; each word has exactly
//                      one owning lane (0 and 32), which stores it whole: plain stores, no atomics on the set.  Pad bits are
//                      stored 0.  The population count is the ballots' popcount, summed per wave and added once per wave to a
//                      64-bit integer (order-free).
//   k_space_words      a thread per 32-voxel word: known-free = free & ~occupied, and the frontier = known-free voxels with an
//                      UNKNOWN face neighbour inside the grid.  Unknown = ~(occupied | free) under the row's valid-bit mask;
//                      a word outside the grid has no unknown voxel, so the grid's own border makes no frontier.  Along x the
//                      neighbour is the word shifted by one with the CARRY bit of the adjacent word (bit 31 of the word below,
//                      bit 0 of the word above); along y and z it is the same word of the adjacent row or slice.
//   k_space_state      a lane per voxel: the byte plane
//   the cell list      k_grid_cell_count / k_cloud_scan / k_grid_cell_scatter of dsm_k_grid.h on the frontier words
// No shortcut is taken that carve_voxel does not decide: no frustum rejection, nothing hoisted out of xform_point.  Every loop is
// bounded by the grid or by the frame count; no workgroup waits on another.
#pragma once
#include "dsm_k_grid.h"

namespace dsm {

struct CarveArgs {
    CarveConst c; // all but inv, which is the frame's
    GridDims g;
    int n_frames;
};
static_assert(offsetof(CarveArgs, g) == sizeof(CarveConst) && offsetof(CarveArgs, n_frames) == sizeof(CarveConst) + 16 && sizeof(CarveArgs) == sizeof(CarveConst) + 20,
              "as the kernel was built for");

__global__ __launch_bounds__(256) void k_carve(const float *__restrict__ depth_base, const CarveFrame *__restrict__ frames, uint32_t *__restrict__ bits,
                                               unsigned long long *__restrict__ count, const CarveArgs a) {
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int per_row = (a.g.nx + 63) >> 6;
    const int64_t units = (int64_t)a.g.ny * a.g.nz * per_row;
    const bool replace = (a.c.flags & kCarveReplace) != 0;
    unsigned long long freed = 0; // (wave-uniform)
    for (int64_t u = (int64_t)blockIdx.x * 4 + wv; u < units; u += (int64_t)gridDim.x * 4) {
        const int64_t row = u / per_row;
        const int x = (int)(u % per_row) * 64 + lane, y = (int)(row % a.g.ny), z = (int)(row / a.g.ny);
        const int w = x >> 5;
        const bool inside = x < a.g.nx; // (then w < wx)
        bool is_free = inside && !replace && ((bits[row * a.g.wx + w] >> (x & 31)) & 1u);
        if (inside && !is_free) {
            CarveConst c = a.c;
            for (int f = 0; f < a.n_frames; f++) {
                for (int k = 0; k < 16; k++) c.inv[k] = frames[f].inv[k];
                if (carve_voxel(c, depth_base + frames[f].depth_off, x, y, z) == kCarveFree) {
                    is_free = true;
                    break;
                }
            }
        }
        const unsigned long long m = __ballot(is_free);
        if ((lane & 31) == 0 && w < a.g.wx) bits[row * a.g.wx + w] = (uint32_t)(m >> (lane & 32));
        freed += (unsigned long long)__popcll(m);
    }
    if (lane == 0 && freed) atomicAdd(count, freed);
}

struct SpaceArgs {
    GridDims g;
};
static_assert(sizeof(SpaceArgs) == 16, "as the kernels were built for");

// the unknown voxels of word w of row (y, z): 0 outside the grid, the pad bits 0
__device__ __forceinline__ uint32_t space_unknown(const uint32_t *__restrict__ occ, const uint32_t *__restrict__ fre, int w, int y, int z, const SpaceArgs &a,
                                                  uint32_t last_mask) {
    if (w < 0 || w >= a.g.wx || y < 0 || y >= a.g.ny || z < 0 || z >= a.g.nz) return 0u;
    const int64_t i = ((int64_t)z * a.g.ny + y) * a.g.wx + w;
    const uint32_t unknown = ~(occ[i] | fre[i]);
    return w == a.g.wx - 1 ? unknown & last_mask : unknown;
}

__global__ __launch_bounds__(256) void k_space_words(const uint32_t *__restrict__ occ, const uint32_t *__restrict__ fre, uint32_t *__restrict__ known_free,
                                                     uint32_t *__restrict__ frontier, const SpaceArgs a) {
    const int64_t n_words = (int64_t)a.g.wx * a.g.ny * a.g.nz;
    const uint32_t last_mask = (a.g.nx & 31) ? (1u << (a.g.nx & 31)) - 1u : 0xffffffffu;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * 256) {
        const int w = (int)(i % a.g.wx);
        const int64_t row = i / a.g.wx;
        const int y = (int)(row % a.g.ny), z = (int)(row / a.g.ny);
        uint32_t kf = fre[i] & ~occ[i];
        if (w == a.g.wx - 1) kf &= last_mask;
        if (known_free) known_free[i] = kf;
        if (frontier) {
            const uint32_t here = space_unknown(occ, fre, w, y, z, a, last_mask);
            const uint32_t below = space_unknown(occ, fre, w - 1, y, z, a, last_mask), above = space_unknown(occ, fre, w + 1, y, z, a, last_mask);
            uint32_t nb = ((here << 1) | (below >> 31)) | ((here >> 1) | (above << 31)); // bit i: voxel i - 1 or i + 1 unknown
            nb |= space_unknown(occ, fre, w, y - 1, z, a, last_mask) | space_unknown(occ, fre, w, y + 1, z, a, last_mask);
            nb |= space_unknown(occ, fre, w, y, z - 1, a, last_mask) | space_unknown(occ, fre, w, y, z + 1, a, last_mask);
            frontier[i] = kf & nb;
        }
    }
}

__global__ __launch_bounds__(256) void k_space_state(const uint32_t *__restrict__ occ, const uint32_t *__restrict__ fre, uint8_t *__restrict__ state,
                                                     const SpaceArgs a) {
    const int64_t n_vox = (int64_t)a.g.nx * a.g.ny * a.g.nz;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_vox; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / a.g.nx;
        const int x = (int)(i - row * a.g.nx);
        const int64_t wi = row * a.g.wx + (x >> 5);
        state[i] = space_state((occ[wi] >> (x & 31)) & 1u, (fre[wi] >> (x & 31)) & 1u);
    }
}

hipError_t launch_carve(const float *depth_base, const CarveFrame *frames, int n_frames, const CarveConst &c, const GridDims &d, uint32_t *bits,
                        unsigned long long *count, hipStream_t st) {
    const hipError_t e0 = hipMemsetAsync(count, 0, sizeof(unsigned long long), st);
    if (e0 != hipSuccess) return e0;
    CarveArgs a;
    a.c = c;
    a.g = d;
    a.n_frames = n_frames;
    hipLaunchKernelGGL(k_carve, dim3(launch_blocks(d.units64(), 4, 16384)), dim3(256), 0, st, depth_base, frames, bits, count, a);
    return hipGetLastError();
}

// frontier: always written (the list and the count are taken from it); known_free, state, cells may be null.  cell_tiles:
// d.cell_tiles() ints of scratch, cells_total: one int.
hipError_t launch_space(const uint32_t *occ, const uint32_t *fre, const GridDims &d, uint8_t *state, uint32_t *known_free, uint32_t *frontier,
                        int32_t *cells, int cells_cap, int32_t *cell_tiles, int32_t *cells_total, hipStream_t st) {
    const SpaceArgs a = {d};
    hipLaunchKernelGGL(k_space_words, dim3(launch_blocks(d.n_words(), 256, 8192)), dim3(256), 0, st, occ, fre, known_free, frontier, a);
    if (state) hipLaunchKernelGGL(k_space_state, dim3(launch_blocks(d.n_vox(), 256, 16384)), dim3(256), 0, st, occ, fre, state, a);
    launch_cell_list(frontier, d, cell_tiles, cells_total, cells, cells_cap, st);
    return hipGetLastError();
}

} // namespace dsm
