// dsm_view.h -- viewpoint gain: what a camera at a candidate pose would see of the voxel grid (dsm_grid_view): the definitions,
// shared by the kernel of dsm_k_view.h, the engine call and the host checker tests/view_host.cpp.  Included at the end of
// dsm_math.h, behind dsm_carve.h (it uses carve_project and space_state).
//
// The outcome is defined PER POSE AND PER VOXEL, so no order of execution can matter.  A voxel is IN VIEW when its centre passes
// steps 1-4 of the carve's definition (carve_project) with the view camera.  It is BLOCKED when some interior point of the line
// from the camera's voxel a to the voxel v that lies inside the grid is a blocker; VISIBLE = in view and not blocked.
//   the line     d = v - a, n = max |d_i|; p_k = a + floor((2 k d + n) / (2 n)) per axis for k = 1 .. n - 1 (view_line_point:
//                the mathematical floor, in int64).  Both ends are excluded; with n <= 1 there is no interior.  This is k d / n
//                rounded half up, so the line walked from v towards a is the same set of points:
//                  a + floor((2 (n - j) d + n) / (2 n)) = a + d + floor((-2 j d + n) / (2 n)) = v + floor((2 j (-d) + n) / (2 n)),
//                consecutive points are 26-adjacent (each axis moves by |d_i| / n <= 1 a step, rounded monotonically), and
//                every axis is monotone in k.
//   a blocker    a voxel of `occupied`; with kViewUnknownBlocks any voxel that is not known free (free & ~occupied).  Outside
//                the grid nothing blocks.
// ViewWalk is the same line by integer error terms, for the kernel; the proof that it equals the closed form stands with it.
#pragma once

namespace dsm {

constexpr int kViewMaxReach = 4096;          // DSM_VIEW_MAX_REACH
constexpr int kViewMaxPoses = 4096;          // DSM_VIEW_MAX_POSES
constexpr uint32_t kViewUnknownBlocks = 1u;  // DSM_VIEW_UNKNOWN_BLOCKS

struct ViewPose {   // 80 bytes, in device memory: one per pose of the call
    float inv[16];  // world -> camera, column-major
    int32_t a[3];   // the camera's voxel (comp_from_voxel of the pose's translation); it may lie outside the grid
    int32_t reserved;
};

struct ViewCounts { // dsm_view_score, field for field
    int32_t in_view, visible, unknown, free_, occupied, target, reserved[2];
};

// may a camera stand in voxel a along an axis of n voxels?  (what bounds the length of every line)
DSM_HD bool view_reach_ok(int32_t a, int32_t n) { return a >= -kViewMaxReach && (int64_t)a < (int64_t)n + kViewMaxReach; }

// floor(num / den) for den > 0
DSM_HD int64_t view_floor_div(int64_t num, int64_t den) {
    const int64_t q = num / den;
    return (num % den != 0 && num < 0) ? q - 1 : q;
}

// n of the line from a to v
DSM_HD int64_t view_line_n(const int32_t *a, const int32_t *v) {
    int64_t n = 0;
    for (int i = 0; i < 3; i++) {
        const int64_t d = (int64_t)v[i] - a[i], m = d < 0 ? -d : d;
        n = m > n ? m : n;
    }
    return n;
}

// coordinate of point k of the line along one axis: the closed form
DSM_HD int64_t view_line_point(int32_t a, int32_t v, int64_t n, int64_t k) {
    const int64_t d = (int64_t)v - a;
    return a + view_floor_div(2 * k * d + n, 2 * n);
}

// is the voxel with these bits a blocker?
DSM_HD bool view_blocker(bool occupied, bool free_, uint32_t flags) { return occupied || ((flags & kViewUnknownBlocks) && !free_); }

// in view: steps 1-4 of the carve with the view camera (c.pitch, c.margin and c.flags are not read)
DSM_HD bool view_in_view(const CarveConst &c, int x, int y, int z) {
    float qz;
    int u, v;
    return carve_project(c, x, y, z, qz, u, v) == kCarveFree;
}

// The line from `from` to `to` by integer error terms: after k calls of step(), p[i] = point k of the line.
//   Per axis let N_k = 2 k d + n.  The closed form is q_k = floor(N_k / (2 n)), that is the one integer with
//   N_k = 2 n q_k + r_k and 0 <= r_k < 2 n.  The walk keeps (q, r) with exactly that invariant:
//     k = 0:   N_0 = n = 2 n * 0 + n, and 0 <= n < 2 n because n >= 1 (the walk is not started with n = 0).
//     a step:  N_{k+1} = N_k + 2 d = 2 n q + (r + 2 d).  |d| <= n, so r + 2 d lies in [-2 n, 4 n): at most one correction by
//              2 n brings it back into [0, 2 n) -- r >= 2 n: (q + 1, r - 2 n); r < 0: (q - 1, r + 2 n) -- and the sum is unchanged.
//   The quotient with a remainder in [0, 2 n) is unique, so q = q_k after every step, ties (r_k = 0) and negative d included:
//   nothing here truncates.  |d| < 2^28 + 4096 (a grid has at most 2^28 voxels along an axis, the reach is 4096), so r + 2 d stays
//   below 2^31 in absolute value: int32 holds it.
struct ViewWalk {
    int32_t p[3];  // the current point
    int32_t r[3];  // the remainders
    int32_t d2[3]; // 2 d per axis
    int32_t n2;    // 2 n
};

DSM_HD void view_walk_init(ViewWalk &w, const int32_t *from, const int32_t *to, int32_t n) {
    for (int i = 0; i < 3; i++) {
        w.p[i] = from[i];
        w.r[i] = n;
        w.d2[i] = 2 * (to[i] - from[i]);
    }
    w.n2 = 2 * n;
}

DSM_HD void view_walk_step(ViewWalk &w) {
    for (int i = 0; i < 3; i++) {
        int32_t r = w.r[i] + w.d2[i];
        if (r >= w.n2) {
            r -= w.n2;
            w.p[i]++;
        } else if (r < 0) {
            r += w.n2;
            w.p[i]--;
        }
        w.r[i] = r;
    }
}

} // namespace dsm
