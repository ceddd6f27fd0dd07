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
    int nx, ny, nz, wx, n_frames;
};

__global__ __launch_bounds__(256) void k_carve(const float *__restrict__ depth_base, const CarveFrame *__restrict__ frames, uint32_t *__restrict__ bits,
                                               unsigned long long *__restrict__ count, const CarveArgs a) {
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int per_row = (a.nx + 63) >> 6;
    const int64_t units = (int64_t)a.ny * a.nz * per_row;
    const bool replace = (a.c.flags & kCarveReplace) != 0;
    unsigned long long freed = 0; // (wave-uniform)
    for (int64_t u = (int64_t)blockIdx.x * 4 + wv; u < units; u += (int64_t)gridDim.x * 4) {
        const int64_t row = u / per_row;
        const int x = (int)(u % per_row) * 64 + lane, y = (int)(row % a.ny), z = (int)(row / a.ny);
        const int w = x >> 5;
        const bool inside = x < a.nx; // (then w < wx)
        bool is_free = inside && !replace && ((bits[row * a.wx + w] >> (x & 31)) & 1u);
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
        if ((lane & 31) == 0 && w < a.wx) bits[row * a.wx + w] = (uint32_t)(m >> (lane & 32));
        freed += (unsigned long long)__popcll(m);
    }
    if (lane == 0 && freed) atomicAdd(count, freed);
}

struct SpaceArgs {
    int nx, ny, nz, wx;
};

// the unknown voxels of word w of row (y, z): 0 outside the grid, the pad bits 0
__device__ __forceinline__ uint32_t space_unknown(const uint32_t *__restrict__ occ, const uint32_t *__restrict__ fre, int w, int y, int z, const SpaceArgs &a,
                                                  uint32_t last_mask) {
    if (w < 0 || w >= a.wx || y < 0 || y >= a.ny || z < 0 || z >= a.nz) return 0u;
    const int64_t i = ((int64_t)z * a.ny + y) * a.wx + w;
    const uint32_t unknown = ~(occ[i] | fre[i]);
    return w == a.wx - 1 ? unknown & last_mask : unknown;
}

__global__ __launch_bounds__(256) void k_space_words(const uint32_t *__restrict__ occ, const uint32_t *__restrict__ fre, uint32_t *__restrict__ known_free,
                                                     uint32_t *__restrict__ frontier, const SpaceArgs a) {
    const int64_t n_words = (int64_t)a.wx * a.ny * a.nz;
    const uint32_t last_mask = (a.nx & 31) ? (1u << (a.nx & 31)) - 1u : 0xffffffffu;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * 256) {
        const int w = (int)(i % a.wx);
        const int64_t row = i / a.wx;
        const int y = (int)(row % a.ny), z = (int)(row / a.ny);
        uint32_t kf = fre[i] & ~occ[i];
        if (w == a.wx - 1) kf &= last_mask;
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
    const int64_t n_vox = (int64_t)a.nx * a.ny * a.nz;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_vox; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / a.nx;
        const int x = (int)(i - row * a.nx);
        const int64_t wi = row * a.wx + (x >> 5);
        state[i] = space_state((occ[wi] >> (x & 31)) & 1u, (fre[wi] >> (x & 31)) & 1u);
    }
}

hipError_t launch_carve(const float *depth_base, const CarveFrame *frames, int n_frames, const CarveConst &c, int nx, int ny, int nz, uint32_t *bits,
                        unsigned long long *count, hipStream_t st) {
    const hipError_t e0 = hipMemsetAsync(count, 0, sizeof(unsigned long long), st);
    if (e0 != hipSuccess) return e0;
    CarveArgs a;
    a.c = c;
    a.nx = nx; a.ny = ny; a.nz = nz; a.wx = (nx + 31) / 32; a.n_frames = n_frames;
    const int64_t units = (int64_t)ny * nz * ((nx + 63) / 64); // <= 2^28
    const int blocks = (int)((units + 3) / 4 < 16384 ? (units + 3) / 4 : 16384);
    hipLaunchKernelGGL(k_carve, dim3(blocks), dim3(256), 0, st, depth_base, frames, bits, count, a);
    return hipGetLastError();
}

// frontier: always written (the list and the count are taken from it); known_free, state, cells may be null.  cell_tiles: (n_words +
// 255) / 256 ints of scratch, cells_total: one int.
hipError_t launch_space(const uint32_t *occ, const uint32_t *fre, int nx, int ny, int nz, uint8_t *state, uint32_t *known_free, uint32_t *frontier,
                        int32_t *cells, int cells_cap, int32_t *cell_tiles, int32_t *cells_total, hipStream_t st) {
    SpaceArgs a;
    a.nx = nx; a.ny = ny; a.nz = nz; a.wx = (nx + 31) / 32;
    const int64_t n_words = (int64_t)a.wx * ny * nz, n_vox = (int64_t)nx * ny * nz;
    {
        const int blocks = (int)((n_words + 255) / 256 < 8192 ? (n_words + 255) / 256 : 8192);
        hipLaunchKernelGGL(k_space_words, dim3(blocks), dim3(256), 0, st, occ, fre, known_free, frontier, a);
    }
    if (state) {
        const int blocks = (int)((n_vox + 255) / 256 < 16384 ? (n_vox + 255) / 256 : 16384);
        hipLaunchKernelGGL(k_space_state, dim3(blocks), dim3(256), 0, st, occ, fre, state, a);
    }
    launch_cell_list(frontier, n_words, nx, a.wx, cell_tiles, cells_total, cells, cells_cap, st);
    return hipGetLastError();
}

} // namespace dsm
