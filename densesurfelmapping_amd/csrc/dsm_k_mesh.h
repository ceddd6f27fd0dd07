// dsm_k_mesh.h -- the hexagon mesh of SurfelMap::save_mesh (SM.cpp = surfel_fusion/src/surfel_map.cpp of the reference,
// :1176-1280) as vertex and index buffers:
//   k_mesh_scatter   the map part of the surfel sequence (dsm_k_sequence.h: map_tile_walk)
//   k_mesh_gather    its runs, of the inactive store's surfel RECORDS (not the XYZI shadow; run_source)
//   k_mesh_indices   12 indices per surfel, the four faces of :1274-1277
// Included by dsm_kernels.hip.
//
// The store path.  A surfel becomes D = 36 (REF6) or 24 (XYZ_RGBA8) dwords.  A lane storing its own 144 bytes at a
// 144-byte stride would touch 64 separate lines per instruction; but the passing records of one 64-record chunk land
// back to back in the output (at + rank), so each wave stages its chunk in LDS as the output image itself and then
// writes it as one contiguous run, lane q storing the q-th 16 bytes (1 KiB per wave instruction).
// LDS layout: record `rank` at float4 slots [rank * D/4, +D/4), written with ds_write_b128.  A b128 write is served in
// groups of 8 contiguous lanes over 32 banks (8 slots): D/4 = 9 slots is odd, so 8 lanes hit 8 different slots (no
// conflict); D/4 = 6 puts them on 4 slots (2-way: 16 LDS-array cycles against the 13 the instruction takes to issue).
// As plain dword writes both strides conflict (36 l mod 32 = 4 l: 4-way; 24 l: 8-way).  The image is read back linearly
// (ds_read_b128, lane q slot q: conflict-free).  D * 4 is a multiple of 16, so with a 16-byte aligned destination every
// run starts and ends on a 16-byte boundary; a destination that is only 4-byte aligned gets a head and a tail of dword
// stores around the 16-byte body (its LDS reads are then four dwords each: the slow path, same bytes).
// All offsets into the output are 64-bit: record index * 144 passes 2^31 at 14.9 M surfels.  No workgroup waits on another.
#pragma once
#include "dsm_k_cloud.h"

namespace dsm {

// 16 bytes as one value: a store of it is one ds_write_b128 / global_store_dwordx4 (a float4 is a struct, whose store the
// compiler may take apart into its members)
typedef float mesh_f4 __attribute__((ext_vector_type(4)));

template <int LAYOUT> struct MeshLayout;
template <> struct MeshLayout<kMeshRef6> { static constexpr int kSlots = 9; };     // 6 x (x y z c c c)
template <> struct MeshLayout<kMeshXyzRgba8> { static constexpr int kSlots = 6; }; // 6 x (x y z rgba)

// the vertices of one surfel into its slots of the wave's image
template <int LAYOUT> __device__ __forceinline__ void mesh_stage(mesh_f4 *__restrict__ img, int rank, const dsm_surfel &r) {
    float pt[6][3];
    int ic;
    surfel_hexagon(r, pt, ic);
    mesh_f4 *o = img + rank * MeshLayout<LAYOUT>::kSlots;
    if constexpr (LAYOUT == kMeshRef6) {
        const float c = (float)ic; // SM.cpp:1212-1214
        float v[36];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            v[6 * k + 0] = pt[k][0]; v[6 * k + 1] = pt[k][1]; v[6 * k + 2] = pt[k][2];
            v[6 * k + 3] = c; v[6 * k + 4] = c; v[6 * k + 5] = c;
        }
#pragma unroll
        for (int q = 0; q < 9; q++) o[q] = mesh_f4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
    } else {
        const uint32_t b = surfel_color_byte(ic);
        const float rgba = __uint_as_float(b | (b << 8) | (b << 16) | 0xff000000u); // bytes r g b 255
#pragma unroll
        for (int k = 0; k < 6; k++) o[k] = mesh_f4{pt[k][0], pt[k][1], pt[k][2], rgba};
    }
}

// the first n_rec records of the wave's image to g (the output address of the run's first record), as one contiguous run
template <int LAYOUT> __device__ __forceinline__ void mesh_flush(const mesh_f4 *__restrict__ img, int n_rec, float *__restrict__ g, int lane) {
    const int total = n_rec * MeshLayout<LAYOUT>::kSlots * 4; // dwords
    const int s = (int)(((uintptr_t)g >> 2) & 3);             // dwords of the run's start past a 16-byte boundary
    if (s == 0) {
        mesh_f4 *g4 = reinterpret_cast<mesh_f4 *>(g);
        for (int q = lane; q < total / 4; q += 64) g4[q] = img[q];
        return;
    }
    // 16-byte piece q of the destination holds the run's dwords [4 q - s, +4): piece 0 starts s dwords before the run (a
    // head of 4 - s dwords), the last piece ends 4 - s dwords after it (a tail of s), the total / 4 - 1 between are whole
    const float *f = reinterpret_cast<const float *>(img);
    const int pieces = total / 4 + 1;
    for (int q = lane; q < pieces; q += 64) {
        const int j = 4 * q - s;
        if (j >= 0 && j + 4 <= total) {
            *reinterpret_cast<mesh_f4 *>(g + j) = mesh_f4{f[j], f[j + 1], f[j + 2], f[j + 3]};
        } else {
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (j + c >= 0 && j + c < total) g[j + c] = f[j + c];
        }
    }
}

// out: the destination's first byte; the map part starts at record `base` (the runs of the store come first); records at
// or beyond `cap` are not written
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_mesh_scatter(const MapPart mp, float *__restrict__ out, int base, int cap) {
    constexpr int kSlots = MeshLayout<LAYOUT>::kSlots;
    __shared__ mesh_f4 s_img[4][64 * kSlots];
    const int lane = lane_id();
    mesh_f4 *img = s_img[threadIdx.x >> 6];
    map_tile_walk(mp, base, [&](unsigned long long m, int at, int i) {
        const int passed = __popcll(m), room = cap - at; // records of this run that fit below cap
        const int n_rec = room <= 0 ? 0 : room < passed ? room : passed;
        if (n_rec > 0) { // (wave-uniform)
            if ((m >> lane) & 1ull) {
                const int rank = rank_below(m);
                if (rank < n_rec) mesh_stage<LAYOUT>(img, rank, mp.rec[i]);
            }
            wave_lds_sync();
            mesh_flush<LAYOUT>(img, n_rec, out + (int64_t)at * (kSlots * 4), lane);
            wave_lds_sync(); // the next chunk overwrites the image
        }
    });
}

// output j of the runs is record j of the destination.  A wave takes 64 consecutive outputs at a time.
template <int LAYOUT>
__global__ __launch_bounds__(256) void k_mesh_gather(const dsm_surfel *__restrict__ src, const RunTable rt, float *__restrict__ out, int cap) {
    constexpr int kSlots = MeshLayout<LAYOUT>::kSlots;
    __shared__ mesh_f4 s_img[4][64 * kSlots];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int lim = rt.total < cap ? rt.total : cap;
    mesh_f4 *img = s_img[wv];
    for (int64_t j0 = ((int64_t)blockIdx.x * 4 + wv) * 64; j0 < lim; j0 += (int64_t)gridDim.x * 256) {
        const int n_rec = lim - j0 < 64 ? (int)(lim - j0) : 64;
        if (lane < n_rec) mesh_stage<LAYOUT>(img, lane, src[run_source(rt, (int)j0 + lane)]);
        wave_lds_sync();
        mesh_flush<LAYOUT>(img, n_rec, out + j0 * (int64_t)(kSlots * 4), lane);
        wave_lds_sync();
    }
}

// SM.cpp:1270-1278: faces (p1 p2 p3) (p2 p4 p3) (p3 p4 p5) (p5 p4 p6) of surfel i, p1 = 6 i.  WIDE: a thread per 16 bytes
// (three per surfel; the destination is 16-byte aligned), else a thread per index.
template <bool WIDE> __global__ __launch_bounds__(256) void k_mesh_indices(uint32_t *__restrict__ out, int n) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    if constexpr (WIDE) {
        for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < (int64_t)n * 3; t += stride) {
            const uint32_t i = (uint32_t)(t / 3), part = (uint32_t)(t - (int64_t)i * 3), p = 6u * i;
            const uint4 v = part == 0 ? make_uint4(p, p + 1, p + 2, p + 1) : part == 1 ? make_uint4(p + 3, p + 2, p + 2, p + 3) : make_uint4(p + 4, p + 4, p + 3, p + 5);
            reinterpret_cast<uint4 *>(out)[t] = v;
        }
    } else {
        for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < (int64_t)n * 12; t += stride) {
            const uint32_t i = (uint32_t)(t / 12), k = (uint32_t)(t - (int64_t)i * 12);
            // 0 1 2  1 3 2  2 3 4  4 3 5, three bits each
            const uint32_t lo = 0u | 1u << 3 | 2u << 6 | 1u << 9 | 3u << 12 | 2u << 15, hi = 2u | 3u << 3 | 4u << 6 | 4u << 9 | 3u << 12 | 5u << 15;
            out[t] = 6u * i + (((k < 6 ? lo : hi) >> (3 * (k < 6 ? k : k - 6))) & 7u);
        }
    }
}

hipError_t launch_mesh_map(const MapPart &mp, int layout, void *out, int base, int cap, hipStream_t st) {
    const hipError_t e = launch_map_offsets(mp, st);
    if (e != hipSuccess || map_tiles(mp) == 0) return e;
    if (layout == kMeshRef6) hipLaunchKernelGGL(k_mesh_scatter<kMeshRef6>, dim3(map_tiles(mp)), dim3(256), 0, st, mp, (float *)out, base, cap);
    else hipLaunchKernelGGL(k_mesh_scatter<kMeshXyzRgba8>, dim3(map_tiles(mp)), dim3(256), 0, st, mp, (float *)out, base, cap);
    return hipGetLastError();
}

hipError_t launch_mesh_gather(const dsm_surfel *src, const RunTable &rt, int layout, void *out, int cap, hipStream_t st) {
    const int lim = rt.total < cap ? rt.total : cap;
    if (rt.n_seg == 0 || lim <= 0) return hipSuccess;
    if (layout == kMeshRef6) hipLaunchKernelGGL(k_mesh_gather<kMeshRef6>, dim3(run_blocks(lim)), dim3(256), 0, st, src, rt, (float *)out, cap);
    else hipLaunchKernelGGL(k_mesh_gather<kMeshXyzRgba8>, dim3(run_blocks(lim)), dim3(256), 0, st, src, rt, (float *)out, cap);
    return hipGetLastError();
}

hipError_t launch_mesh_indices(uint32_t *out, int n, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    const bool wide = ((uintptr_t)out & 15) == 0;
    int64_t blocks = ((int64_t)n * (wide ? 3 : 12) + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (wide) hipLaunchKernelGGL(k_mesh_indices<true>, dim3((unsigned)blocks), dim3(256), 0, st, out, n);
    else hipLaunchKernelGGL(k_mesh_indices<false>, dim3((unsigned)blocks), dim3(256), 0, st, out, n);
    return hipGetLastError();
}

} // namespace dsm
