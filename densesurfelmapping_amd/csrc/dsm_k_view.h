// dsm_k_view.h -- viewpoint gain: candidate camera poses scored against the voxel grid (dsm_grid_view).  The definitions
// (view_in_view, the line, view_blocker) are in dsm_view.h and shared with the host checker tests/view_host.cpp; this file is how
// they are evaluated:
//   k_view   k_carve's shape: a wave per 64 voxels of a row, a lane per voxel, the poses in the second grid dimension (both
//            dimensions capped and strided over).  A lane whose voxel is in view walks its line with ViewWalk (integer error
//            terms, proven equal to the closed form where it is defined) and tests one bit of the blocker word per step.  A
//            ballot packs the 64 lanes into two words; each word has exactly one owning lane (0 and 32), which stores it whole:
//            plain stores, no atomics on the plane, pad bits 0.  The six counts are ballot popcounts, summed per wave over its
//            trips and added once per wave per counter (int32 atomicAdd: order-free).
// Two arrangements that the definition decides:
//   - The line is walked FROM THE VOXEL towards the camera (the same points, dsm_view.h), and "some interior point is a blocker"
//     does not depend on the order, so the walk ends at the first blocker.
//   - The walk also ends at the first point OUTSIDE the grid.  Every axis of the line is monotone in k and the grid is a product of
//     intervals, so the k whose points lie inside the grid are the intersection of three intervals of k: one interval.  It
//     contains k = n (the voxel itself), so once a point walking down from n - 1 lies outside, every further one does, and
//     outside the grid nothing blocks.  This bounds a lane's walk by the grid's largest dimension, whatever the reach.
// No frustum or range rejection of a wave or a tile is taken: carve_project decides every voxel on its own.
// LDS is not used: the 64 lines of a wave fan out towards the camera through rows all over the grid, so a tile of the sets staged
// per workgroup would serve the first few steps only; the sets (512 KB for 4 M voxels) stay in L2, and the words near the voxels
// of one wave are shared through L1 by its lanes.  Every loop is bounded by the grid or the pose count; no workgroup waits on
// another; no inline assembly.
#pragma once
#include "dsm_k_grid.h"

namespace dsm {

struct ViewArgs {
    CarveConst c; // origin, voxel, the view camera; inv is the pose's
    GridDims g;
    int n_poses;
    uint32_t flags;
};
static_assert(offsetof(ViewArgs, g) == sizeof(CarveConst) && offsetof(ViewArgs, n_poses) == sizeof(CarveConst) + 16 && offsetof(ViewArgs, flags) == sizeof(CarveConst) + 20 &&
                  sizeof(ViewArgs) == sizeof(CarveConst) + 24,
              "as the kernel was built for");

constexpr int kViewBlocksX = 1024, kViewBlocksY = 64; // the launch caps: units of 4 waves, poses

__global__ __launch_bounds__(256) void k_view(const ViewPose *__restrict__ poses, const uint32_t *__restrict__ occ, const uint32_t *__restrict__ fre,
                                              const uint32_t *__restrict__ target, ViewCounts *__restrict__ scores, uint32_t *__restrict__ visible,
                                              const ViewArgs a) {
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int per_row = (a.g.nx + 63) >> 6;
    const int64_t units = (int64_t)a.g.ny * a.g.nz * per_row, n_words = (int64_t)a.g.ny * a.g.nz * a.g.wx;
    const bool unknown_blocks = (a.flags & kViewUnknownBlocks) != 0;
    for (int pose = blockIdx.y; pose < a.n_poses; pose += gridDim.y) {
        CarveConst c = a.c;
        for (int k = 0; k < 16; k++) c.inv[k] = poses[pose].inv[k];
        const int32_t cam[3] = {poses[pose].a[0], poses[pose].a[1], poses[pose].a[2]};
        int n_in = 0, n_vis = 0, n_unk = 0, n_free = 0, n_occ = 0, n_tgt = 0; // (wave-uniform)
        for (int64_t u = (int64_t)blockIdx.x * 4 + wv; u < units; u += (int64_t)gridDim.x * 4) {
            const int64_t row = u / per_row;
            const int x = (int)(u % per_row) * 64 + lane, y = (int)(row % a.g.ny), z = (int)(row / a.g.ny);
            const int w = x >> 5;
            const bool inside = x < a.g.nx; // (then w < wx)
            const bool in_view = inside && view_in_view(c, x, y, z);
            bool vis = in_view;
            if (in_view) {
                const int32_t v[3] = {x, y, z};
                const int32_t n = (int32_t)view_line_n(cam, v);
                if (n > 1) {
                    ViewWalk wk;
                    view_walk_init(wk, v, cam, n);
                    for (int32_t j = 1; j < n; j++) {
                        view_walk_step(wk);
                        const int px = wk.p[0], py = wk.p[1], pz = wk.p[2];
                        if (px < 0 || px >= a.g.nx || py < 0 || py >= a.g.ny || pz < 0 || pz >= a.g.nz) break; // (outside from here on)
                        const int64_t wi = ((int64_t)pz * a.g.ny + py) * a.g.wx + (px >> 5);
                        const uint32_t o = occ[wi];
                        const uint32_t blockers = unknown_blocks ? (o | ~fre[wi]) : o;
                        if ((blockers >> (px & 31)) & 1u) {
                            vis = false;
                            break;
                        }
                    }
                }
            }
            uint32_t o_bit = 0, f_bit = 0, t_bit = 0;
            if (vis) {
                const int64_t wi = row * a.g.wx + w;
                o_bit = (occ[wi] >> (x & 31)) & 1u;
                f_bit = (fre[wi] >> (x & 31)) & 1u;
                if (target) t_bit = (target[wi] >> (x & 31)) & 1u;
            }
            const uint8_t state = space_state(o_bit != 0, f_bit != 0);
            const unsigned long long m = __ballot(vis);
            if (visible && (lane & 31) == 0 && w < a.g.wx) visible[(int64_t)pose * n_words + row * a.g.wx + w] = (uint32_t)(m >> (lane & 32));
            n_in += __popcll(__ballot(in_view));
            n_vis += __popcll(m);
            n_unk += __popcll(__ballot(vis && state == kSpaceUnknown));
            n_free += __popcll(__ballot(vis && state == kSpaceFree));
            n_occ += __popcll(__ballot(vis && state == kSpaceOccupied));
            n_tgt += __popcll(__ballot(t_bit != 0));
        }
        if (lane == 0) {
            ViewCounts *s = scores + pose;
            if (n_in) atomicAdd(&s->in_view, n_in);
            if (n_vis) atomicAdd(&s->visible, n_vis);
            if (n_unk) atomicAdd(&s->unknown, n_unk);
            if (n_free) atomicAdd(&s->free_, n_free);
            if (n_occ) atomicAdd(&s->occupied, n_occ);
            if (n_tgt) atomicAdd(&s->target, n_tgt);
        }
    }
}

// scores: [n_poses], cleared on `st` first; visible: [n_poses][nz][ny][wx] or null; target may be null.  c: everything but inv.
hipError_t launch_view(const ViewPose *poses, int n_poses, const CarveConst &c, uint32_t flags, const GridDims &d, const uint32_t *occ,
                       const uint32_t *fre, const uint32_t *target, ViewCounts *scores, uint32_t *visible, hipStream_t st) {
    const hipError_t e0 = hipMemsetAsync(scores, 0, sizeof(ViewCounts) * (size_t)n_poses, st);
    if (e0 != hipSuccess) return e0;
    ViewArgs a;
    a.c = c;
    a.g = d;
    a.n_poses = n_poses;
    a.flags = flags;
    const int bx = launch_blocks(d.units64(), 4, kViewBlocksX);
    const int by = n_poses < kViewBlocksY ? n_poses : kViewBlocksY;
    hipLaunchKernelGGL(k_view, dim3(bx, by), dim3(256), 0, st, poses, occ, fre, target, scores, visible, a);
    return hipGetLastError();
}

} // namespace dsm
