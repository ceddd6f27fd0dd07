// dsm_k_cloud.h -- the node's point-cloud publications (SM.cpp = surfel_fusion/src/surfel_map.cpp of the reference):
//   k_cloud_count / k_cloud_scan / k_cloud_scatter   order-preserving filtered compaction of the resident map into XYZI
//                    (publish_active_pointcloud SM.cpp:1398-1417: update_times >= 5; publish_neighbor_pointcloud
//                    SM.cpp:1292-1303: update_times != 0)
//   k_cloud_gather   runs of the inactive store's XYZI shadow behind it (publish_inactive / all / neighbor_pointcloud,
//                    SM.cpp:1305-1319, 1385-1454)
//   k_cloud_raw      the fused frame back-projected to world points, column-major (publish_raw_pointcloud SM.cpp:1115-1151)
// Included by dsm_kernels.hip.
//
// The compaction has no inter-workgroup waiting: a count pass (one tile of kCloudTile records per workgroup, wave ballots),
// a one-workgroup exclusive scan of the tile counts, and a scatter pass that recomputes the ballots and places every
// passing record at its tile offset + wave prefix + mbcnt rank.  update_times is read twice (once per pass); a look-back
// scan would read it once but spins on other workgroups.
#pragma once
#include "dsm_k_common.h"

namespace dsm {

constexpr int kRawTileW = 64, kRawTileH = 32;            // pixels of a k_cloud_raw tile (columns x rows)

__device__ __forceinline__ bool cloud_pass(int select, int32_t update_times) {
    return select == kCloudMature ? update_times >= 5 : update_times != 0;
}

// records below min(*n_ptr, n_upper) are the map: the grid covers n_upper, the running bound of the handle
__device__ __forceinline__ int cloud_map_size(const int32_t *__restrict__ n_ptr, int n_upper) {
    const int n = n_ptr[0];
    return n < n_upper ? n : n_upper;
}

__global__ __launch_bounds__(256) void k_cloud_count(const dsm_surfel *__restrict__ rec, const int32_t *__restrict__ n_ptr, int n_upper,
                                                     int select, int32_t *__restrict__ tile_cnt) {
    __shared__ int s_cnt[4];
    const int n = cloud_map_size(n_ptr, n_upper);
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int first = blockIdx.x * kCloudTile + wv * 64 * kCloudChunks;
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < kCloudChunks; c++) {
        const int i = first + c * 64 + lane;
        const bool pass = i < n && cloud_pass(select, rec[i].update_times);
        cnt += __popcll(__ballot(pass));
    }
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) tile_cnt[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// in place: tile_cnt[0 .. n_tiles) -> exclusive prefix; total[0] = the sum.  One workgroup of 1024 threads.
__global__ __launch_bounds__(1024) void k_cloud_scan(int32_t *__restrict__ tile_cnt, int n_tiles, int32_t *__restrict__ total) {
    __shared__ int s_wave[16];
    __shared__ int s_carry;
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < n_tiles; base += 1024) {
        const int t = base + (int)threadIdx.x;
        const int v = t < n_tiles ? tile_cnt[t] : 0;
        int incl = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_wave[wv] = incl;
        __syncthreads();
        if (wv == 0) {
            int w = lane < 16 ? s_wave[lane] : 0;
#pragma unroll
            for (int d = 1; d < 16; d <<= 1) {
                const int o = __shfl_up(w, d, 64);
                if (lane >= d) w += o;
            }
            if (lane < 16) s_wave[lane] = w; // inclusive over waves
        }
        __syncthreads();
        const int carry = s_carry;
        const int wave_excl = wv ? s_wave[wv - 1] : 0;
        if (t < n_tiles) tile_cnt[t] = carry + wave_excl + (incl - v);
        __syncthreads();
        if (threadIdx.x == 0) s_carry = carry + s_wave[15];
        __syncthreads();
    }
    if (threadIdx.x == 0) total[0] = s_carry;
}

__global__ __launch_bounds__(256) void k_cloud_scatter(const dsm_surfel *__restrict__ rec, const int32_t *__restrict__ n_ptr, int n_upper,
                                                       int select, const int32_t *__restrict__ tile_off, float4 *__restrict__ out, int cap) {
    __shared__ int s_cnt[4];
    const int n = cloud_map_size(n_ptr, n_upper);
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int first = blockIdx.x * kCloudTile + wv * 64 * kCloudChunks;
    unsigned long long mask[kCloudChunks];
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < kCloudChunks; c++) {
        const int i = first + c * 64 + lane;
        mask[c] = __ballot(i < n && cloud_pass(select, rec[i].update_times));
        cnt += __popcll(mask[c]);
    }
    if (lane == 0) s_cnt[wv] = cnt;
    __syncthreads();
    int at = tile_off[blockIdx.x];
    for (int k = 0; k < wv; k++) at += s_cnt[k];
#pragma unroll
    for (int c = 0; c < kCloudChunks; c++) {
        const unsigned long long m = mask[c];
        if ((m >> lane) & 1ull) {
            const int idx = at + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (idx < cap) {
                const dsm_surfel *r = rec + first + c * 64 + lane;
                out[idx] = make_float4(r->px, r->py, r->pz, r->color); // SM.cpp:1404-1409
            }
        }
        at += __popcll(m);
    }
}

// seg[3 s + 0 .. 2] = (begin in the store, count, exclusive output offset) of the non-empty runs; output j of the runs goes to
// out[base + j], base = *base_ptr (the map part's count, on the device)
__global__ __launch_bounds__(256) void k_cloud_gather(const float4 *__restrict__ src, const int32_t *__restrict__ seg, int n_seg, int total,
                                                      const int32_t *__restrict__ base_ptr, float4 *__restrict__ out, int cap) {
    const int base = base_ptr[0];
    for (int j = blockIdx.x * 256 + threadIdx.x; j < total; j += gridDim.x * 256) {
        int lo = 0, hi = n_seg; // last run whose offset is <= j
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (seg[3 * mid + 2] <= j) lo = mid; else hi = mid;
        }
        const int dst = base + j;
        if (dst < cap) out[dst] = src[seg[3 * lo] + (j - seg[3 * lo + 2])];
    }
}

// SM.cpp:1117-1150.  One tile of kRawTileW columns x kRawTileH rows per workgroup: pixels are read along rows (coalesced),
// the points go through LDS and leave along columns (output index i * h + j: runs of kRawTileH points, 16-byte stores).
// E33: rotation_R * cam_point in Eigen >= 3.3's order (DSM_FLAG_EIGEN33_PRODUCTS).
template <bool E33 = false> __global__ __launch_bounds__(256) void k_cloud_raw(const uint8_t *__restrict__ img, const float *__restrict__ depth, int pitch, int w, int h,
                                                   const RawCloudParams p, float4 *__restrict__ out) {
    __shared__ float4 s_pt[kRawTileW * (kRawTileH + 1)];
    const int i0 = blockIdx.x * kRawTileW, j0 = blockIdx.y * kRawTileH;
    {
        const int il = threadIdx.x & (kRawTileW - 1), i = i0 + il;
#pragma unroll
        for (int k = 0; k < kRawTileH / 4; k++) {
            const int jl = (threadIdx.x >> 6) + 4 * k, j = j0 + jl;
            if (i < w && j < h) {
                const float d = depth[(int64_t)j * pitch + i];
                const float cam[3] = {((float)i - p.cx) * d / p.fx, ((float)j - p.cy) * d / p.fy, d};
                float o[3];
                xform_dir_as<E33>(p.rot, cam, o); // rotation_R * cam_point
                s_pt[il * (kRawTileH + 1) + jl] = make_float4(o[0] + p.t[0], o[1] + p.t[1], o[2] + p.t[2], (float)img[(int64_t)j * pitch + i]);
            }
        }
    }
    __syncthreads();
    const int jl = threadIdx.x & (kRawTileH - 1), j = j0 + jl;
#pragma unroll
    for (int k = 0; k < kRawTileW / 8; k++) {
        const int il = (threadIdx.x >> 5) + 8 * k, i = i0 + il;
        if (i < w && j < h) out[(int64_t)i * h + j] = s_pt[il * (kRawTileH + 1) + jl];
    }
}

hipError_t launch_cloud_map(const dsm_surfel *rec, const int32_t *n_ptr, int n_upper, int select, int32_t *tile_cnt, int32_t *total,
                            float4 *out, int cap, hipStream_t st) {
    const int tiles = (n_upper + kCloudTile - 1) / kCloudTile;
    if (tiles == 0) return hipMemsetAsync(total, 0, sizeof(int32_t), st);
    hipLaunchKernelGGL(k_cloud_count, dim3(tiles), dim3(256), 0, st, rec, n_ptr, n_upper, select, tile_cnt);
    hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(1024), 0, st, tile_cnt, tiles, total);
    hipLaunchKernelGGL(k_cloud_scatter, dim3(tiles), dim3(256), 0, st, rec, n_ptr, n_upper, select, (const int32_t *)tile_cnt, out, cap);
    return hipGetLastError();
}

hipError_t launch_cloud_gather(const float4 *src, const int32_t *seg, int n_seg, int total, const int32_t *base_ptr, float4 *out, int cap,
                               hipStream_t st) {
    if (n_seg == 0 || total == 0) return hipSuccess;
    int blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_cloud_gather, dim3(blocks), dim3(256), 0, st, src, seg, n_seg, total, base_ptr, out, cap);
    return hipGetLastError();
}

hipError_t launch_cloud_raw(const uint8_t *img, const float *depth, int pitch, int w, int h, const RawCloudParams &p, bool eigen33, float4 *out,
                            hipStream_t st) {
    const dim3 grid((w + kRawTileW - 1) / kRawTileW, (h + kRawTileH - 1) / kRawTileH);
    if (eigen33) hipLaunchKernelGGL(k_cloud_raw<true>, grid, dim3(256), 0, st, img, depth, pitch, w, h, p, out);
    else hipLaunchKernelGGL(k_cloud_raw<false>, grid, dim3(256), 0, st, img, depth, pitch, w, h, p, out);
    return hipGetLastError();
}

} // namespace dsm
