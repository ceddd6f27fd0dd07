// dsm_k_sequence.h -- the surfel sequence of the map products (RunTable / MapPart of dsm_device.h; DESIGN.md, "the surfel sequence
// and its walk"), once for the cloud, the mesh, the render and the grid:
//   run_source         the runs: which store record is output j of the run table
//   k_cloud_count      the map part, pass 1: how many records of every tile of kCloudTile pass `select`; k_cloud_scan
//                      (dsm_k_cloud.h) turns the counts into tile offsets in place
//   map_tile_walk      the map part, pass 2, inside a product's own kernel: the ballots again, then every 64-record chunk with the
//                      sequence number of its first passing record
//   two_ended_slot     where a survivor of the sequence goes in the render's and the grid's splat array
// Everything is integer and order-preserving, and no workgroup waits on another: update_times is read twice (once per pass); a
// look-back scan would read it once but spins on other workgroups.
#pragma once
#include "dsm_k_common.h"

namespace dsm {

__device__ __forceinline__ bool cloud_pass(int select, int32_t update_times) {
    return select == kCloudMature ? update_times >= 5 : update_times != 0;
}

// the store record behind output j of the runs (0 <= j < rt.total, rt.n_seg > 0)
__device__ __forceinline__ int64_t run_source(const RunTable &rt, int j) {
    int lo = 0, hi = rt.n_seg; // last run whose offset is <= j
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rt.seg[3 * mid + 2] <= j) lo = mid; else hi = mid;
    }
    return (int64_t)rt.seg[3 * lo] + (j - rt.seg[3 * lo + 2]);
}

// first record of my wave's kCloudChunks chunks: a workgroup of 256 takes the tile blockIdx.x
__device__ __forceinline__ int map_wave_first() { return blockIdx.x * kCloudTile + (threadIdx.x >> 6) * 64 * kCloudChunks; }

// mask[c] = the lanes whose record first + 64 c + lane is in the map (below min(*n_ptr, n_upper): the grid covers n_upper, the
// running bound of the handle) and passes; returns how many there are in the wave's chunks
__device__ __forceinline__ int map_wave_masks(const MapPart &mp, int first, unsigned long long (&mask)[kCloudChunks]) {
    const int n = mp.n_ptr[0] < mp.n_upper ? mp.n_ptr[0] : mp.n_upper;
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < kCloudChunks; c++) {
        const int i = first + c * 64 + lane_id();
        mask[c] = __ballot(i < n && cloud_pass(mp.select, mp.rec[i].update_times));
        cnt += __popcll(mask[c]);
    }
    return cnt;
}

__global__ __launch_bounds__(256) void k_cloud_count(const MapPart mp) {
    __shared__ int s_cnt[4];
    unsigned long long mask[kCloudChunks];
    const int cnt = map_wave_masks(mp, map_wave_first(), mask);
    if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) mp.tile_cnt[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// Called by every thread of a workgroup of 256 whose tile is blockIdx.x, after launch_map_offsets.  chunk(m, at, i), once per chunk
// and wave (wave-uniform): m = the lanes whose record i passes, at = the sequence number of the first of them when the map part
// starts at `base`; the lane's own number is at + rank_below(m).  `at` is an int: check_sequence keeps every sequence below 2^31
// records.  A BYTE offset made of it (the mesh's at * 144) does pass 2^31: that product is the caller's to widen first.
template <typename F> __device__ __forceinline__ void map_tile_walk(const MapPart &mp, int base, F chunk) {
    __shared__ int s_cnt[4];
    const int lane = lane_id(), wv = threadIdx.x >> 6, first = map_wave_first();
    unsigned long long mask[kCloudChunks];
    const int cnt = map_wave_masks(mp, first, mask);
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    int at = base + mp.tile_cnt[blockIdx.x];
    for (int k = 0; k < wv; k++) at += s_cnt[k];
#pragma unroll
    for (int c = 0; c < kCloudChunks; c++) {
        chunk(mask[c], at, first + c * 64 + lane);
        at += __popcll(mask[c]);
    }
}

// ONE array of n_seq records as two lists: `small` lanes take slots from the front (counts[0]), `big` lanes from the back
// (counts[1]), by a wave ballot and one atomic add per wave and list; they cannot meet while the array is as long as the sequence.
// Called by whole waves; the slot of a lane in neither list means nothing.
__device__ __forceinline__ int two_ended_slot(bool small, bool big, int32_t *__restrict__ counts, int n_seq) {
    const unsigned long long m_small = __ballot(small), m_big = __ballot(big);
    int base_small = 0, base_big = 0;
    if (lane_id() == 0) {
        if (m_small) base_small = atomicAdd(&counts[0], __popcll(m_small));
        if (m_big) base_big = atomicAdd(&counts[1], __popcll(m_big));
    }
    base_small = __shfl(base_small, 0, 64);
    base_big = __shfl(base_big, 0, 64);
    return small ? base_small + rank_below(m_small) : n_seq - 1 - (base_big + rank_below(m_big));
}

// ---- host side
__global__ void k_cloud_scan(int32_t *__restrict__ tile_cnt, int n_tiles, int32_t *__restrict__ total); // dsm_k_cloud.h

inline int map_tiles(const MapPart &mp) { return (mp.n_upper + kCloudTile - 1) / kCloudTile; } // the grid of a map_tile_walk kernel
inline int run_blocks(int total) { return launch_blocks(total, 256, 4096); } // the grid of a kernel over the runs

// mp.tile_cnt = the tile offsets and mp.total[0] = the count that a map_tile_walk kernel launched behind this finds
inline hipError_t launch_map_offsets(const MapPart &mp, hipStream_t st) {
    const int tiles = map_tiles(mp);
    if (tiles == 0) return hipMemsetAsync(mp.total, 0, sizeof(int32_t), st);
    hipLaunchKernelGGL(k_cloud_count, dim3(tiles), dim3(256), 0, st, mp);
    hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(1024), 0, st, mp.tile_cnt, tiles, mp.total);
    return hipGetLastError();
}

} // namespace dsm
