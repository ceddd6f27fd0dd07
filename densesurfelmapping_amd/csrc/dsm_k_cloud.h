// dsm_k_cloud.h -- the node's point-cloud publications (SM.cpp = surfel_fusion/src/surfel_map.cpp of the reference):
//   k_cloud_scan / k_cloud_scatter   behind k_cloud_count: order-preserving filtered compaction of the resident map into
//                    XYZI (publish_active_pointcloud SM.cpp:1398-1417: update_times >= 5; publish_neighbor_pointcloud
//                    SM.cpp:1292-1303: update_times != 0)
//   k_cloud_gather   runs of the inactive store's XYZI shadow behind it (publish_inactive / all / neighbor_pointcloud,
//                    SM.cpp:1305-1319, 1385-1454)
//   k_cloud_raw      the fused frame back-projected to world points, column-major (publish_raw_pointcloud SM.cpp:1115-1151)
// Included by dsm_kernels.hip.
//
// The compaction is the walk of dsm_k_sequence.h: k_cloud_count, k_cloud_scan, and a scatter pass that places every passing
// record at its sequence number.
#pragma once
#include "dsm_k_sequence.h"

namespace dsm {

constexpr int kRawTileW = 64, kRawTileH = 32;            // pixels of a k_cloud_raw tile (columns x rows)

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

__global__ __launch_bounds__(256) void k_cloud_scatter(const MapPart mp, float4 *__restrict__ out, int cap) {
    map_tile_walk(mp, 0, [&](unsigned long long m, int at, int i) {
        const int idx = at + rank_below(m);
        if (((m >> lane_id()) & 1ull) && idx < cap) {
            const dsm_surfel *r = mp.rec + i;
            out[idx] = make_float4(r->px, r->py, r->pz, r->color); // SM.cpp:1404-1409
        }
    });
}

// output j of the runs goes to out[base + j], base = *base_ptr (the map part's count, on the device)
__global__ __launch_bounds__(256) void k_cloud_gather(const float4 *__restrict__ src, const RunTable rt, const int32_t *__restrict__ base_ptr,
                                                      float4 *__restrict__ out, int cap) {
    const int base = base_ptr[0];
    for (int j = blockIdx.x * 256 + threadIdx.x; j < rt.total; j += gridDim.x * 256) {
        const int dst = base + j;
        if (dst < cap) out[dst] = src[run_source(rt, j)];
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

hipError_t launch_cloud_map(const MapPart &mp, float4 *out, int cap, hipStream_t st) {
    const hipError_t e = launch_map_offsets(mp, st);
    if (e != hipSuccess || map_tiles(mp) == 0) return e;
    hipLaunchKernelGGL(k_cloud_scatter, dim3(map_tiles(mp)), dim3(256), 0, st, mp, out, cap);
    return hipGetLastError();
}

hipError_t launch_cloud_gather(const float4 *src, const RunTable &rt, const int32_t *base_ptr, float4 *out, int cap, hipStream_t st) {
    if (rt.n_seg == 0 || rt.total == 0) return hipSuccess;
    hipLaunchKernelGGL(k_cloud_gather, dim3(run_blocks(rt.total)), dim3(256), 0, st, src, rt, base_ptr, out, cap);
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
