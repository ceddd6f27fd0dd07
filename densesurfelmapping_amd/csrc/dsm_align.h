// dsm_align.h -- a depth frame against the map as an image: projective association and the normal equations of one
// point-to-plane Gauss-Newton step (dsm_k_align.h, tests/align_host.cpp).  Included by dsm_math.h (never on its own: it uses that header's DSM_HD, ray_coeff, RenderCam), written once for the kernel
// and for the serial checker; every parenthesis is part of the definition.  No reference counterpart.
//
// One evaluation: a frame depth plane [h][pitch] (metres) with the frame camera's intrinsics and distances, a model camera
// with its depth plane and camera-frame normal plane as dsm_render_compose writes them, a rigid transform T (frame camera ->
// model camera, column-major) and the parameters below.  align_pixel is the rule of one sampled frame pixel; what passes it
// adds 28 fixed-point terms and a count to the 29 sums.  The host part further down (the 6x6 solve, the update of T, the loop)
// is double precision, plain host functions.
#pragma once

namespace dsm {

constexpr int kAlignSums = 29;     // 21 upper-triangle entries of w J J^T, row by row | 6 of w J r | w r^2 | the count
constexpr int kAlignCost = 27, kAlignCount = 28;
constexpr int kAlignMaxScale = 40; // cap of the fixed-point scale 2^k
constexpr int kAlignMinScale = 10; // a camera that leaves less is refused

// the exits of align_pixel, in the order of the rule (the census of tests/test_cpu_align.py)
enum AlignExit {
    kAlignPass = 0, kAlignDepth, kAlignRangeZ, kAlignRangeQ, kAlignOutside, kAlignModelDepth, kAlignNormal, kAlignDistance, kAlignViewCos,
    kAlignExits
};

struct AlignFrame { // the frame side: the handle's image, intrinsics and fuse distances
    int w, h, pitch;
    float fx, fy, cx, cy, near_d, far_d;
};

struct AlignConst {
    AlignFrame f;
    RenderCam m;        // the model camera
    int stride;
    float qmax2;        // align_qmax(m) squared, as a float product
    float dist_max2;    // dist_max * dist_max
    float view_cos2;    // min_view_cos * min_view_cos
    double huber;       // 0 = every weight is 1
    int scale_log2;     // k: a term t enters its sum as llrint(t * 2^k)
    float T[16];        // frame camera -> model camera
};

// The longest camera-frame vector the rule lets through: far_dist times the length of the most oblique ray one pixel outside
// the model image (columns -1 and w, rows -1 and h).
DSM_HD float align_qmax(const RenderCam &cam) {
    const double xa = fabs((double)ray_coeff(-1, cam.cx, cam.fx)), xb = fabs((double)ray_coeff(cam.w, cam.cx, cam.fx));
    const double ya = fabs((double)ray_coeff(-1, cam.cy, cam.fy)), yb = fabs((double)ray_coeff(cam.h, cam.cy, cam.fy));
    const double rx = xa > xb ? xa : xb, ry = ya > yb ? ya : yb;
    return (float)((double)cam.far_d * sqrt((rx * rx + ry * ry) + 1.0));
}

// The scale 2^k of the fixed-point sums.  Every term that enters a sum is at most M = 2 max(1, qmax)^2 in magnitude:
//   |n_i| <= sqrt 2 (the gate |n|^2 <= 2), |(q x n)_i| <= |q| |n| <= sqrt 2 qmax (the gate |q|^2 <= qmax^2), so |J_i J_j| <= 2 max(1, qmax)^2;
//   |r| = |n . e| <= sqrt 2 dist_max <= sqrt 2 qmax (dist_max <= qmax is an argument check), so |J_i r| <= 2 max(1, qmax) qmax and r^2 <= 2 qmax^2;
//   the weight is <= 1.
// A rounded term is at most M 2^k + 1/2, and n_sampled of them at most n_sampled (M 2^k + 1/2).  k is the largest value, at
// most kAlignMaxScale, that keeps this <= 2^62: int64 holds 2^63 - 1, and the factor of two covers the float roundings of the
// gates themselves (|n|^2 and |q|^2 are computed in fp32: relative 2e-7) many times over.  Negative: not even k = 0 fits.
DSM_HD int align_scale_log2(const RenderCam &cam, int64_t n_sampled) {
    const double qmax = (double)align_qmax(cam);
    const double q1 = qmax > 1.0 ? qmax : 1.0;
    const double M = 2.0 * q1 * q1;
    const double room = 4611686018427387904.0 / (double)(n_sampled > 0 ? n_sampled : 1); // 2^62 / n
    for (int k = kAlignMaxScale; k >= 0; k--)
        if (ldexp(M, k) + 0.5 <= room) return k;
    return -1;
}

// sampled pixels along a side of n >= 1 pixels: ceil(n / stride), written so that no stride up to INT_MAX overflows
DSM_HD int align_sampled_side(int n, int stride) { return (n - 1) / stride + 1; }

DSM_HD int64_t align_sampled(int w, int h, int stride) { return (int64_t)align_sampled_side(w, stride) * align_sampled_side(h, stride); }

DSM_HD int64_t align_fixed(double term, int k) { return (int64_t)llrint(ldexp(term, k)); }

// One sampled frame pixel (u, v): u % stride == 0, v % stride == 0, u < w, v < h (never a pad column).  Adds to acc[29] when it
// passes; returns the exit taken.  Acc = int64_t (the checker's overflow test also runs it with a wider type).
template <typename Acc>
DSM_HD AlignExit align_pixel(const AlignConst &c, const float *__restrict__ depth, const float *__restrict__ zm_plane, const float *__restrict__ nm_plane,
                             int u, int v, Acc *acc) {
    // 1. the frame's depth
    const float d = depth[(int64_t)v * c.f.pitch + u];
    if (!(d > c.f.near_d && d < c.f.far_d)) return kAlignDepth; // (a NaN fails both, an infinity one)
    // 2. 3. the point in the frame camera, then in the model camera
    const float p[3] = {ray_coeff(u, c.f.cx, c.f.fx) * d, ray_coeff(v, c.f.cy, c.f.fy) * d, d};
    float q[3];
    for (int i = 0; i < 3; i++) q[i] = ((c.T[i] * p[0] + c.T[4 + i] * p[1]) + c.T[8 + i] * p[2]) + c.T[12 + i];
    // 4.
    if (!(q[2] > c.m.near_d && q[2] < c.m.far_d)) return kAlignRangeZ;
    const float q2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2];
    if (!(q2 <= c.qmax2)) return kAlignRangeQ;
    // 5. the model pixel, rounded as fuse_project rounds
    const int um = round_to_pixel((q[0] * c.m.fx) / q[2] + c.m.cx), vm = round_to_pixel((q[1] * c.m.fy) / q[2] + c.m.cy);
    if (um < 0 || um >= c.m.w || vm < 0 || vm >= c.m.h) return kAlignOutside;
    // 6. 7. what the map shows there
    const int64_t at = (int64_t)vm * c.m.w + um;
    const float zm = zm_plane[at];
    if (!(zm > 0.0f)) return kAlignModelDepth;
    const float n[3] = {nm_plane[3 * at], nm_plane[3 * at + 1], nm_plane[3 * at + 2]};
    const float n2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
    if (!(n2 >= 0.5f && n2 <= 2.0f)) return kAlignNormal; // zero, NaN and arbitrary-bit normals
    // 8. the model point and the distance to it
    const float e[3] = {q[0] - ray_coeff(um, c.m.cx, c.m.fx) * zm, q[1] - ray_coeff(vm, c.m.cy, c.m.fy) * zm, q[2] - zm};
    const float e2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
    if (!(e2 <= c.dist_max2)) return kAlignDistance;
    // 9. |n . q| >= min_view_cos |q|, squared
    const float nq = (n[0] * q[0] + n[1] * q[1]) + n[2] * q[2];
    if (!(nq * nq >= c.view_cos2 * q2)) return kAlignViewCos;
    // 10. residual, Jacobian (translation part first) and weight in double, from the float values
    const double nd[3] = {(double)n[0], (double)n[1], (double)n[2]}, qd[3] = {(double)q[0], (double)q[1], (double)q[2]};
    const double r = (nd[0] * (double)e[0] + nd[1] * (double)e[1]) + nd[2] * (double)e[2];
    const double J[6] = {nd[0], nd[1], nd[2], qd[1] * nd[2] - qd[2] * nd[1], qd[2] * nd[0] - qd[0] * nd[2], qd[0] * nd[1] - qd[1] * nd[0]};
    double w = 1.0;
    if (c.huber > 0.0) {
        const double ar = fabs(r);
        w = ar <= c.huber ? 1.0 : c.huber / ar;
    }
    const int k = c.scale_log2;
    int s = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double wj = w * J[i];
#pragma unroll
        for (int j = i; j < 6; j++) acc[s++] += align_fixed(wj * J[j], k);
        acc[21 + i] += align_fixed(wj * r, k);
    }
    acc[kAlignCost] += align_fixed((w * r) * r, k);
    acc[kAlignCount] += 1;
    return kAlignPass;
}

// sampled pixel number i (row-major over the sampled grid) -> (u, v)
DSM_HD void align_sample(const AlignConst &c, int64_t i, int &u, int &v) {
    const int n_sx = align_sampled_side(c.f.w, c.stride);
    v = (int)(i / n_sx) * c.stride;
    u = (int)(i % n_sx) * c.stride;
}

// ------------------------------------------------------------------ the host step and the loop (double precision)

enum AlignStatus { kAlignConverged = 0, kAlignMaxIterations = 1, kAlignTooFew = 2, kAlignSingular = 3 }; // DSM_ALIGN_* of include/dsm.h

// The constants of an evaluation from its arguments (T is set per evaluation).  Returns what is wrong with them, or nullptr.
static inline const char *align_prepare(const AlignFrame &f, const RenderCam &m, int stride, float dist_max, float min_view_cos, float huber, AlignConst &c) {
    if (m.w < 1 || m.w > kRenderMaxSide || m.h < 1 || m.h > kRenderMaxSide) return "model image size outside 1..8192";
    if (!(m.fx > 0.0f && m.fy > 0.0f) || !(fabsf(m.fx) < __builtin_inff()) || !(fabsf(m.fy) < __builtin_inff()) || !(fabsf(m.cx) < __builtin_inff()) ||
        !(fabsf(m.cy) < __builtin_inff()))
        return "model camera intrinsics";
    if (!(m.near_d > 0.0f) || !(m.near_d < m.far_d) || !(m.far_d < __builtin_inff())) return "model depth range";
    if (stride < 1) return "stride < 1";
    const float qmax = align_qmax(m);
    if (!(qmax < __builtin_inff())) return "model camera: qmax is not finite";
    if (!(dist_max > 0.0f && dist_max <= qmax)) return "dist_max not in (0, qmax]";
    if (!(min_view_cos >= 0.0f && min_view_cos <= 1.0f)) return "min_view_cos outside [0, 1]";
    if (!(huber >= 0.0f && huber < __builtin_inff())) return "huber negative or not finite";
    c.f = f;
    c.m = m;
    c.stride = stride;
    c.qmax2 = qmax * qmax;
    c.dist_max2 = dist_max * dist_max;
    c.view_cos2 = min_view_cos * min_view_cos;
    c.huber = (double)huber;
    c.scale_log2 = align_scale_log2(m, align_sampled(f.w, f.h, stride));
    if (c.scale_log2 < kAlignMinScale) return "model camera leaves a fixed-point scale below 2^10";
    for (int k = 0; k < 16; k++) c.T[k] = (k % 5 == 0) ? 1.0f : 0.0f;
    return nullptr;
}

struct AlignLoop {
    int max_iterations;
    int64_t min_pixels;
    double stop_translation, stop_rotation;
    int scale_log2;
};

struct AlignOutcome {
    int status, iterations;
    int64_t n_pixels;
    double rms;
    double T[16]; // frame camera -> corrected frame camera, column-major
    int64_t sums[kAlignSums]; // of the last evaluation
};

// A xi = -b from the 29 sums, by LDL^T without pivoting, column by column; false (SINGULAR) when a pivot is not > 1e-9 trace(A).
// xi = (v, omega).
static inline bool align_solve(const int64_t *sums, int k, double xi[6]) {
    double A[6][6], b[6], L[6][6], D[6];
    int s = 0;
    for (int i = 0; i < 6; i++)
        for (int j = i; j < 6; j++) A[i][j] = A[j][i] = ldexp((double)sums[s++], -k);
    for (int i = 0; i < 6; i++) b[i] = -ldexp((double)sums[21 + i], -k);
    double trace = 0.0;
    for (int i = 0; i < 6; i++) trace += A[i][i];
    const double floor_d = 1e-9 * trace;
    for (int j = 0; j < 6; j++) {
        double dj = A[j][j];
        for (int m = 0; m < j; m++) dj -= (L[j][m] * L[j][m]) * D[m];
        if (!(dj > floor_d)) return false;
        D[j] = dj;
        L[j][j] = 1.0;
        for (int i = j + 1; i < 6; i++) {
            double l = A[i][j];
            for (int m = 0; m < j; m++) l -= (L[i][m] * L[j][m]) * D[m];
            L[i][j] = l / dj;
        }
    }
    double y[6];
    for (int i = 0; i < 6; i++) { // L y = b
        double t = b[i];
        for (int m = 0; m < i; m++) t -= L[i][m] * y[m];
        y[i] = t;
    }
    for (int i = 5; i >= 0; i--) { // L^T xi = D^-1 y
        double t = y[i] / D[i];
        for (int m = i + 1; m < 6; m++) t -= L[m][i] * xi[m];
        xi[i] = t;
    }
    return true;
}

// R (row-major 3x3) of the rotation vector om: I + sin(th)/th K + (1 - cos(th))/th^2 K^2, K = [om]x; first order below 1e-12
static inline void align_rodrigues(const double om[3], double R[9]) {
    const double th2 = (om[0] * om[0] + om[1] * om[1]) + om[2] * om[2], th = sqrt(th2);
    double a = 1.0, b = 0.5;
    if (th > 1e-12) {
        a = sin(th) / th;
        b = (1.0 - cos(th)) / th2;
    }
    const double K[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double kk = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
            R[3 * i + j] = ((i == j ? 1.0 : 0.0) + a * K[3 * i + j]) + b * kk;
        }
}

// T <- [Rodrigues(omega) R, Rodrigues(omega) t + v], T column-major 4x4
static inline void align_apply(const double xi[6], double T[16]) {
    double Rw[9], N[16];
    align_rodrigues(xi + 3, Rw);
    for (int c = 0; c < 4; c++) {
        for (int i = 0; i < 3; i++) N[4 * c + i] = (Rw[3 * i] * T[4 * c] + Rw[3 * i + 1] * T[4 * c + 1]) + Rw[3 * i + 2] * T[4 * c + 2];
        N[4 * c + 3] = c == 3 ? 1.0 : 0.0;
    }
    for (int i = 0; i < 3; i++) N[12 + i] += xi[i];
    for (int k = 0; k < 16; k++) T[k] = N[k];
}

// pose16 = pose_guess16 . T as a double product cast to float (both column-major)
static inline void align_refined_pose(const float *guess16, const double *T, float *pose16) {
    for (int c = 0; c < 4; c++)
        for (int i = 0; i < 4; i++) {
            double s = 0.0;
            for (int m = 0; m < 4; m++) s += (double)guess16[4 * m + i] * T[4 * c + m];
            pose16[4 * c + i] = (float)s;
        }
}

// The loop round an evaluator: eval(const float T16[16], int64_t sums[29]) -> 0, or an error code that ends the loop and is
// returned.  Every estimate is evaluated exactly once; the last evaluation is at the final estimate.
template <typename Eval> int align_loop(const AlignLoop &p, Eval &&eval, AlignOutcome &o) {
    for (int k = 0; k < 16; k++) o.T[k] = (k % 5 == 0) ? 1.0 : 0.0;
    o.iterations = 0;
    o.status = -1;
    for (;;) {
        float Tf[16];
        for (int k = 0; k < 16; k++) Tf[k] = (float)o.T[k];
        if (const int rc = eval((const float *)Tf, o.sums)) return rc;
        if (o.status >= 0) break;
        if (o.sums[kAlignCount] < p.min_pixels) {
            o.status = kAlignTooFew;
            break;
        }
        double xi[6];
        if (!align_solve(o.sums, p.scale_log2, xi)) {
            o.status = kAlignSingular;
            break;
        }
        align_apply(xi, o.T);
        o.iterations++;
        const double dv = sqrt((xi[0] * xi[0] + xi[1] * xi[1]) + xi[2] * xi[2]), dw = sqrt((xi[3] * xi[3] + xi[4] * xi[4]) + xi[5] * xi[5]);
        if (dv < p.stop_translation && dw < p.stop_rotation) o.status = kAlignConverged;
        else if (o.iterations >= p.max_iterations) o.status = kAlignMaxIterations;
    }
    o.n_pixels = o.sums[kAlignCount];
    o.rms = o.n_pixels > 0 ? sqrt(ldexp((double)o.sums[kAlignCost], -p.scale_log2) / (double)o.n_pixels) : 0.0;
    return 0;
}
} // namespace dsm
