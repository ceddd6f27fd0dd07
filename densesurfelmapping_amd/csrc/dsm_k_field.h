// dsm_k_field.h -- the truncated Euclidean distance field of a bit set in the grid layout (dsm_grid_distance, dsm_field_compose):
// per voxel the squared distance in voxels to the nearest set voxel within R, that voxel's linear index, and the distance in
// metres.  The definition (field_key of dsm_math.h: the minimum of (d^2, linear index) over the set voxels within R) is shared
// with the host checker tests/field_host.cpp; this file is how it is evaluated.  A minimum over a union is the minimum of the
// minima, so three passes, one per axis:
//   k_field_x   a lane per voxel, straight from the bits: the nearest set bit at or below x and above x within R, by count-leading
//               / count-trailing zeros on 64-bit windows assembled from the row's words (distance 64 at or below x is the 65th
//               position, tested by itself); the lower x on a tie.  One signed byte per voxel: the offset -64 .. 64, or kFieldNone
//   k_field_y   64 x 64 voxels of a slice per workgroup, the byte plane with its y halo in LDS; a lane walks dy outward, comparing
//               the full key (-dy and +dy can tie), and stops once dy^2 exceeds the best d^2.  Four bytes per voxel: d^2 (16 bits),
//               the x offset, the y offset -- or kFieldMidNone
//   k_field_z   64 x 64 voxels of an (x, z) plane per workgroup, the same along z from the 4-byte plane; writes the planes asked for,
//               `distance` through the host-built table
// A column of a tile (one x, the tile's rows or slices with their halo) that holds no entry has nothing to walk to: its lanes skip
// the walk and write "none" (free space far from any surface is most of a map).
// For a fixed row (slice) the earlier pass holds the minimum key of that row (slice) whenever any of its voxels is within R: the
// later offsets only add a constant to d^2 and the linear index orders rows and slices first.  Every global access runs along x.
// No atomics; every loop is bounded by R or by the tile; no workgroup waits on another.
#pragma once
#include "dsm_k_grid.h"

namespace dsm {

constexpr int kFieldNone = -128;                // k_field_x: no set bit within R in this row
constexpr uint32_t kFieldMidNone = 0xffffffffu; // k_field_y: no set voxel within R in this slice (a real entry has d^2 <= 4096 below)
constexpr int kFieldTile = 64;                  // rows (slices) of output per workgroup of the y (z) pass; a wave takes every fourth

struct FieldArgs {
    GridDims g;
    int r;
};
static_assert(sizeof(FieldArgs) == 20 && offsetof(FieldArgs, r) == 16, "as the kernels were built for");

// word w of a row of the bit set: 0 outside the row, the pad bits of the last word masked
__device__ __forceinline__ uint32_t field_word(const uint32_t *__restrict__ row, int w, int wx, uint32_t last_mask) {
    if (w < 0 || w >= wx) return 0u;
    const uint32_t v = row[w];
    return w == wx - 1 ? v & last_mask : v;
}

// bit i = voxel start + i of the row, i = 0 .. 63; start >= -128
__device__ __forceinline__ unsigned long long field_window(const uint32_t *__restrict__ row, int start, int wx, uint32_t last_mask) {
    const int ws = ((start + 128) >> 5) - 4, s = (start + 128) & 31;
    unsigned long long v = (((unsigned long long)field_word(row, ws + 1, wx, last_mask) << 32) | field_word(row, ws, wx, last_mask)) >> s;
    if (s) v |= (unsigned long long)field_word(row, ws + 2, wx, last_mask) << (64 - s);
    return v;
}

__global__ __launch_bounds__(256) void k_field_x(const uint32_t *__restrict__ bits, int8_t *__restrict__ ox, const FieldArgs a) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)a.g.nx * a.g.ny * a.g.nz) return;
    const int64_t row = i / a.g.nx;
    const int x = (int)(i - row * a.g.nx);
    const uint32_t *rw = bits + row * a.g.wx;
    const uint32_t last_mask = (a.g.nx & 31) ? (1u << (a.g.nx & 31)) - 1u : 0xffffffffu;
    int below = kFieldMaxDist + 1, above = kFieldMaxDist + 1; // distances; R + 1 or more = none
    const unsigned long long lo = field_window(rw, x - 63, a.g.wx, last_mask); // bit 63 = x
    if (lo) below = __clzll((long long)lo);
    else if (x >= 64 && ((field_word(rw, (x - 64) >> 5, a.g.wx, last_mask) >> ((x - 64) & 31)) & 1u)) below = 64;
    const unsigned long long hi = field_window(rw, x + 1, a.g.wx, last_mask); // bit 0 = x + 1
    if (hi) above = __ffsll((long long)hi);
    int o = kFieldNone;
    if (below <= a.r && below <= above) o = -below; // (the lower x on a tie)
    else if (above <= a.r) o = above;
    ox[i] = (int8_t)o;
}

// LDS: [kFieldTile + 2r][64] x offsets, kFieldNone outside the grid
__global__ __launch_bounds__(256) void k_field_y(const int8_t *__restrict__ ox, uint32_t *__restrict__ mid, const FieldArgs a) {
    extern __shared__ int8_t s_field_ox[];
    __shared__ uint8_t s_any[4][64]; // per wave and column: did its rows of the tile hold an entry?
    const int r = a.r, rows = kFieldTile + 2 * r;
    const int tiles_x = (a.g.nx + 63) / 64, tiles_y = (a.g.ny + kFieldTile - 1) / kFieldTile;
    const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x % tiles_y, z = blockIdx.x / tiles_x / tiles_y;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = bx * 64 + lane, y0 = by * kFieldTile - r;
    const int64_t slice = (int64_t)z * a.g.ny;
    bool any = false;
    for (int j = wv; j < rows; j += 4) {
        const int y = y0 + j;
        int8_t v = (int8_t)kFieldNone;
        if (x < a.g.nx && y >= 0 && y < a.g.ny) v = ox[(slice + y) * a.g.nx + x];
        any |= v != (int8_t)kFieldNone;
        s_field_ox[j * 64 + lane] = v;
    }
    s_any[wv][lane] = any;
    __syncthreads();
    if (x >= a.g.nx) return;
    const int walk = (s_any[0][lane] | s_any[1][lane] | s_any[2][lane] | s_any[3][lane]) ? r : -1; // an empty column: nothing to walk to
    for (int t = wv; t < kFieldTile; t += 4) {
        const int y = by * kFieldTile + t;
        if (y >= a.g.ny) break; // (wave-uniform)
        const int c = t + r;  // this row in the tile: c - r >= 0, c + r < rows
        unsigned long long best = ~0ull;
        int best_o = 0, best_dy = 0;
        for (int d = 0; d <= walk; d++) {
            if ((unsigned long long)(d * d) > (best >> 32)) break;
            for (int dy = -d; dy <= d; dy += (d ? 2 * d : 1)) {
                const int o = s_field_ox[(c + dy) * 64 + lane];
                if (o == kFieldNone) continue;
                const int d2 = o * o + d * d;
                if (d2 > r * r) continue;
                const unsigned long long key = field_key((uint32_t)d2, (uint32_t)((y + dy) * a.g.nx + (x + o))); // (rows of one slice: y' nx + x' orders as lin)
                if (key < best) { best = key; best_o = o; best_dy = dy; }
            }
        }
        mid[(slice + y) * a.g.nx + x] =
            best == ~0ull ? kFieldMidNone : (uint32_t)(best >> 32) | ((uint32_t)(uint8_t)best_o << 16) | ((uint32_t)(uint8_t)best_dy << 24);
    }
}

struct FieldOut {       // device memory, tight [nz][ny][nx]; any may be null
    uint16_t *dist2;
    int32_t *nearest;
    float *distance;
};

// LDS: [kFieldTile + 2r][64] entries of k_field_y, kFieldMidNone outside the grid.  table: [r^2 + 1] metres by squared distance.
__global__ __launch_bounds__(256) void k_field_z(const uint32_t *__restrict__ mid, const float *__restrict__ table, const FieldOut out, const FieldArgs a) {
    extern __shared__ uint32_t s_field_mid[];
    __shared__ uint8_t s_any[4][64]; // as in k_field_y
    const int r = a.r, rows = kFieldTile + 2 * r;
    const int tiles_x = (a.g.nx + 63) / 64;
    const int bx = blockIdx.x % tiles_x, y = blockIdx.x / tiles_x % a.g.ny, bz = blockIdx.x / tiles_x / a.g.ny;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int x = bx * 64 + lane, z0 = bz * kFieldTile - r;
    bool any = false;
    for (int j = wv; j < rows; j += 4) {
        const int z = z0 + j;
        uint32_t v = kFieldMidNone;
        if (x < a.g.nx && z >= 0 && z < a.g.nz) v = mid[((int64_t)z * a.g.ny + y) * a.g.nx + x];
        any |= v != kFieldMidNone;
        s_field_mid[j * 64 + lane] = v;
    }
    s_any[wv][lane] = any;
    __syncthreads();
    if (x >= a.g.nx) return;
    const int walk = (s_any[0][lane] | s_any[1][lane] | s_any[2][lane] | s_any[3][lane]) ? r : -1;
    for (int t = wv; t < kFieldTile; t += 4) {
        const int z = bz * kFieldTile + t;
        if (z >= a.g.nz) break; // (wave-uniform)
        const int c = t + r;
        unsigned long long best = ~0ull;
        for (int d = 0; d <= walk; d++) {
            if ((unsigned long long)(d * d) > (best >> 32)) break;
            for (int dz = -d; dz <= d; dz += (d ? 2 * d : 1)) {
                const uint32_t m = s_field_mid[(c + dz) * 64 + lane];
                if (m == kFieldMidNone) continue;
                const int d2 = (int)(m & 0xffffu) + d * d;
                if (d2 > r * r) continue;
                const int xo = x + (int8_t)(m >> 16), yo = y + (int8_t)(m >> 24);
                const unsigned long long key = field_key((uint32_t)d2, (uint32_t)(((int64_t)(z + dz) * a.g.ny + yo) * a.g.nx + xo)); // < 2^26
                if (key < best) best = key;
            }
        }
        const int64_t i = ((int64_t)z * a.g.ny + y) * a.g.nx + x;
        const bool have = best != ~0ull;
        const uint32_t d2 = (uint32_t)(best >> 32);
        if (out.dist2) out.dist2[i] = have ? (uint16_t)d2 : kFieldFar;
        if (out.nearest) out.nearest[i] = have ? (int32_t)(uint32_t)best : -1;
        if (out.distance) out.distance[i] = table[have ? (int)d2 : r * r];
    }
}

// the three passes on one stream.  ox: [voxels] bytes, mid: [voxels] words of scratch.  1 <= r <= kFieldMaxDist, at most kFieldMaxVoxels voxels.
hipError_t launch_field(const uint32_t *bits, const GridDims &d, int r, const float *table, int8_t *ox, uint32_t *mid, uint16_t *dist2,
                        int32_t *nearest, float *distance, hipStream_t st) {
    FieldArgs a;
    a.g = d;
    a.r = r;
    const int64_t n_vox = d.n_vox(), tiles_x = (d.nx + 63) / 64;
    const int64_t blocks_y = tiles_x * ((d.ny + kFieldTile - 1) / kFieldTile) * d.nz, blocks_z = tiles_x * d.ny * ((d.nz + kFieldTile - 1) / kFieldTile);
    if (n_vox > kFieldMaxVoxels || r < 1 || r > kFieldMaxDist) return hipErrorInvalidValue; // (so every block count is at most 2^26)
    FieldOut out;
    out.dist2 = dist2; out.nearest = nearest; out.distance = distance;
    const size_t rows = (size_t)(kFieldTile + 2 * r); // <= 192: 12 KiB of bytes, 48 KiB of words
    hipLaunchKernelGGL(k_field_x, dim3((unsigned)((n_vox + 255) / 256)), dim3(256), 0, st, bits, ox, a);
    hipLaunchKernelGGL(k_field_y, dim3((unsigned)blocks_y), dim3(256), rows * 64, st, (const int8_t *)ox, mid, a);
    hipLaunchKernelGGL(k_field_z, dim3((unsigned)blocks_z), dim3(256), rows * 64 * sizeof(uint32_t), st, (const uint32_t *)mid, table, out, a);
    return hipGetLastError();
}

} // namespace dsm
