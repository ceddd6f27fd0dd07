// dsm_k_align.h -- one evaluation of the frame-to-map alignment (dsm_align_equations, dsm_align_frame): the 29 fixed-point sums
// of align_pixel over the sampled pixels of a frame slot.  The definition (align_pixel, the scale) is in dsm_align.h and shared
// with the host checker tests/align_host.cpp; this file is how it is evaluated:
//   k_align   a grid-stride pass over the sampled pixels, at most kAlignMaxBlocks workgroups of 256; 29 int64 accumulators per
//             thread, summed over the wave by shuffles, over the workgroup's four waves through LDS, then one 64-bit integer
//             atomicAdd per workgroup and sum (none for a sum that is zero) -- at most 1024 x 29 = 29 696 atomics an evaluation.
// The sums are integers, so neither the grid nor the order of the atomics changes a bit of them.  The atomic is atomicAdd on
// unsigned long long (global_atomic_add_x2), plain C++; two's complement makes the unsigned sum the signed one.  What has been
// measured on this chip (MI355X_MICROARCH.md, global float atomics) is the no-return fp32 add, and it says that every adder on
// one row is the slow shape: that is the shape here (29 words, 232 bytes, for every workgroup), chosen because there are so few
// of them.  The 64-bit integer add is NOT measured there.  The caller clears the 29 words on the stream before every launch.
// Reads are bounded by the sampled grid (u < w, v < h) on the frame side and by align_pixel's inside-the-image test on the model
// side; no workgroup waits on another.
#pragma once
#include "dsm_k_common.h"

namespace dsm {

constexpr int kAlignMaxBlocks = 1024;

struct AlignArgs {
    AlignConst c;
    const float *depth;     // the slot's depth plane [h][pitch]
    const float *zm, *nm;   // the model planes [mh][mw], [mh][mw][3]
    unsigned long long *sums; // [29]
};

__global__ __launch_bounds__(256) void k_align(const AlignArgs a) {
    __shared__ long long s_part[4][kAlignSums];
    int64_t acc[kAlignSums];
#pragma unroll
    for (int k = 0; k < kAlignSums; k++) acc[k] = 0;
    const int64_t total = align_sampled(a.c.f.w, a.c.f.h, a.c.stride);
    const int n_sx = align_sampled_side(a.c.f.w, a.c.stride);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int sv = (int)(i / n_sx), su = (int)(i - (int64_t)sv * n_sx);
        align_pixel(a.c, a.depth, a.zm, a.nm, su * a.c.stride, sv * a.c.stride, acc);
    }
    const int lane = lane_id(), wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kAlignSums; k++) {
        long long v = acc[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
        if (lane == 0) s_part[wv][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < kAlignSums) {
        const long long v = (s_part[0][threadIdx.x] + s_part[1][threadIdx.x]) + (s_part[2][threadIdx.x] + s_part[3][threadIdx.x]);
        if (v != 0) atomicAdd(a.sums + threadIdx.x, (unsigned long long)v);
    }
}

hipError_t launch_align(const AlignConst &c, const float *depth, const float *zm, const float *nm, unsigned long long *sums, hipStream_t st) {
    AlignArgs a;
    a.c = c;
    a.depth = depth;
    a.zm = zm;
    a.nm = nm;
    a.sums = sums;
    const int64_t total = align_sampled(c.f.w, c.f.h, c.stride);
    int blocks = (int)((total + 255) / 256 < kAlignMaxBlocks ? (total + 255) / 256 : kAlignMaxBlocks);
    if (blocks < 1) blocks = 1;
    const hipError_t e = hipMemsetAsync(sums, 0, kAlignSums * sizeof(unsigned long long), st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_align, dim3(blocks), dim3(256), 0, st, a);
    return hipGetLastError();
}

} // namespace dsm
