// view_host.cpp -- viewpoint gain on the host (tests/test_cpu_view.py, tests/test_gpu_view.py): the definitions of
// csrc/dsm_view.h evaluated directly, with none of the arrangements of csrc/dsm_k_view.h.
//   score      a brute-force loop over every pose, every voxel and every interior point of its line, from the camera's end, by the
//              closed form view_line_point (an explicit floor division): no early exit, no stop where the line leaves the grid,
//              no integer error terms.  The exit of every (pose, voxel) pair and the facts of its line can be had, for the census
//              of the tests; then the line is evaluated for every voxel, in view or not.
//   walk       the points of one line by ViewWalk, the kernel's error terms, for the tests to hold against the closed form
// Build: g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC.  With -DVIEW_HOST_MAIN the file is a program: for every case file named
// on the command line (tests/view_cases.py's write_case) it scores the poses, checks the scores and the planes against one another,
// walks every line from both ends by the closed form and from the voxel by ViewWalk and compares the points; exit status 0 iff
// everything agrees (run under the sanitizers by the tests).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../densesurfelmapping_amd/csrc/dsm_components.h"
#include "../densesurfelmapping_amd/csrc/dsm_math.h"
#include "../include/dsm.h"

extern "C" {

struct ViewHostGrid { // the scalars of a call: tests/view_cases.py's _Grid
    float origin[3];
    float voxel;
    int32_t nx, ny, nz;
    int32_t w, h;
    float fx, fy, cx, cy;
    float near_d, far_d;
    uint32_t flags;
};

// the exit of a (pose, voxel) pair, in the order the definition decides it
enum ViewExit { kViewVisible = 0, kViewNear = 1, kViewFar = 2, kViewLeft = 3, kViewRight = 4, kViewAbove = 5, kViewBelow = 6, kViewBlocked = 7 };

struct ViewHostLine { // the facts of one pair's line, whether the voxel is in view or not
    int32_t n;        // max |d_i|
    int32_t blockers; // interior points inside the grid that are blockers
    int32_t k_first;  // the lowest k of one, 0 without
    int32_t outside;  // interior points outside the grid
};

} // extern "C"

namespace {

dsm::CarveConst view_const(const ViewHostGrid &g, const float *inv16) {
    dsm::CarveConst c;
    memset(&c, 0, sizeof c);
    for (int a = 0; a < 3; a++) c.origin[a] = g.origin[a];
    c.voxel = g.voxel;
    c.w = g.w; c.h = g.h; c.pitch = g.w;
    c.fx = g.fx; c.fy = g.fy; c.cx = g.cx; c.cy = g.cy;
    c.near_d = g.near_d; c.far_d = g.far_d;
    for (int k = 0; k < 16; k++) c.inv[k] = inv16[k];
    return c;
}

bool bit(const uint32_t *bits, int wx, int64_t row, int x) { return (bits[row * wx + (x >> 5)] >> (x & 31)) & 1u; }

// the line of one pair by the closed form, from the camera's end, every interior point
ViewHostLine line_of(const ViewHostGrid &g, const int32_t *a, const int32_t *v, const uint32_t *occ, const uint32_t *fre) {
    const int wx = (g.nx + 31) / 32;
    ViewHostLine l = {0, 0, 0, 0};
    const int64_t n = dsm::view_line_n(a, v);
    l.n = (int32_t)n;
    for (int64_t k = 1; k < n; k++) {
        const int64_t px = dsm::view_line_point(a[0], v[0], n, k), py = dsm::view_line_point(a[1], v[1], n, k), pz = dsm::view_line_point(a[2], v[2], n, k);
        if (px < 0 || px >= g.nx || py < 0 || py >= g.ny || pz < 0 || pz >= g.nz) {
            l.outside++;
            continue; // outside the grid nothing blocks
        }
        const int64_t row = pz * g.ny + py;
        if (dsm::view_blocker(bit(occ, wx, row, (int)px), bit(fre, wx, row, (int)px), g.flags)) {
            if (!l.blockers) l.k_first = (int32_t)k;
            l.blockers++;
        }
    }
    return l;
}

} // namespace

extern "C" {

// the closed-form inverse the library takes when the caller gives none
void view_host_inverse(const float *pose16, float *inv16) { dsm::inverse4<float>(pose16, inv16); }

// the camera's voxel of a pose in a grid; returns whether the reach rule admits it
int view_host_cam_voxel(const ViewHostGrid *g, const float *pose16, int32_t *a) {
    const int32_t dims[3] = {g->nx, g->ny, g->nz};
    bool ok = true;
    for (int i = 0; i < 3; i++) {
        a[i] = dsm::comp_from_voxel(pose16[12 + i], g->origin[i], g->voxel);
        ok = ok && dsm::view_reach_ok(a[i], dims[i]);
    }
    return ok ? 1 : 0;
}

// invs: [n_poses][16], cams: [n_poses][3] the cameras' voxels; occ / fre / target ([nz][ny][wx]; target may be null).  scores:
// [n_poses] dsm_view_score; visible (may be null): [n_poses][nz][ny][wx], pad bits written 0; exits (may be null): [n_poses][nz][ny][nx]
// ViewExit; lines (may be null): [n_poses][nz][ny][nx] -- with them every voxel's line is evaluated, else only those in view.
// Returns the number of interior points evaluated for the voxels in view: the line steps the definition asks for.
int64_t view_host_score(const ViewHostGrid *g, int n_poses, const float *invs, const int32_t *cams, const uint32_t *occ, const uint32_t *fre,
                        const uint32_t *target, dsm_view_score *scores, uint32_t *visible, uint8_t *exits, ViewHostLine *lines) {
    const int nx = g->nx, ny = g->ny, nz = g->nz, wx = (nx + 31) / 32;
    const size_t n_words = (size_t)wx * ny * nz, n_vox = (size_t)nx * ny * nz;
    int64_t steps = 0;
    if (visible) memset(visible, 0, n_words * sizeof(uint32_t) * (size_t)n_poses);
    for (int p = 0; p < n_poses; p++) {
        const dsm::CarveConst c = view_const(*g, invs + 16 * p);
        const int32_t *a = cams + 3 * p;
        dsm_view_score s;
        memset(&s, 0, sizeof s);
        for (int z = 0; z < nz; z++)
            for (int y = 0; y < ny; y++)
                for (int x = 0; x < nx; x++) {
                    const size_t i = ((size_t)z * ny + y) * nx + x;
                    const int64_t row = (int64_t)z * ny + y;
                    float qz = 0.0f;
                    int u = 0, v = 0;
                    const dsm::CarveExit e = dsm::carve_project(c, x, y, z, qz, u, v);
                    uint8_t exit_ = kViewVisible;
                    if (e == dsm::kCarveRange) exit_ = qz < c.far_d ? kViewNear : kViewFar; // (a NaN: neither side; counted with the far one)
                    else if (e == dsm::kCarveOutside) exit_ = u < 0 ? kViewLeft : u >= c.w ? kViewRight : v < 0 ? kViewAbove : kViewBelow;
                    const bool in_view = dsm::view_in_view(c, x, y, z);
                    if (in_view != (exit_ == kViewVisible)) return -1; // (the two readings of steps 1-4 cannot differ)
                    if (in_view || lines) {
                        const int32_t vox[3] = {x, y, z};
                        const ViewHostLine l = line_of(*g, a, vox, occ, fre);
                        if (lines) lines[n_vox * p + i] = l;
                        if (in_view) {
                            steps += l.n > 1 ? l.n - 1 : 0;
                            if (l.blockers) exit_ = kViewBlocked;
                        }
                    }
                    if (exits) exits[n_vox * p + i] = exit_;
                    if (in_view) s.in_view++;
                    if (exit_ != kViewVisible) continue;
                    s.visible++;
                    const uint8_t state = dsm::space_state(bit(occ, wx, row, x), bit(fre, wx, row, x));
                    if (state == DSM_SPACE_UNKNOWN) s.unknown++;
                    else if (state == DSM_SPACE_FREE) s.free++;
                    else s.occupied++;
                    if (target && bit(target, wx, row, x)) s.target++;
                    if (visible) visible[n_words * p + row * wx + (x >> 5)] |= 1u << (x & 31);
                }
        scores[p] = s;
    }
    return steps;
}

// the points k = skip + 1 .. skip + cap (below n) of the line from `from` towards `to` by ViewWalk (the kernel's error terms), every
// step from k = 1 taken: out [cap][3]; returns n
int32_t view_host_walk(const int32_t *from, const int32_t *to, int32_t *out, int32_t skip, int32_t cap) {
    const int32_t n = (int32_t)dsm::view_line_n(from, to);
    if (n < 1) return n;
    dsm::ViewWalk w;
    dsm::view_walk_init(w, from, to, n);
    for (int32_t k = 1; k < n; k++) {
        dsm::view_walk_step(w);
        if (k > skip && k - skip <= cap)
            for (int i = 0; i < 3; i++) out[3 * (k - skip - 1) + i] = w.p[i];
    }
    return n;
}

// the same points by the closed form: out [cap][3]; returns n
int32_t view_host_line(const int32_t *from, const int32_t *to, int32_t *out, int32_t skip, int32_t cap) {
    const int64_t n = dsm::view_line_n(from, to);
    for (int64_t k = (int64_t)skip + 1; k < n && k - skip <= cap; k++)
        for (int i = 0; i < 3; i++) out[3 * (k - skip - 1) + i] = (int32_t)dsm::view_line_point(from[i], to[i], n, k);
    return (int32_t)n;
}

} // extern "C"

#ifdef VIEW_HOST_MAIN
int main(int argc, char **argv) {
    bool ok = true;
    for (int a = 1; a < argc; a++) {
        std::FILE *f = std::fopen(argv[a], "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        ViewHostGrid g;
        int32_t n_poses = 0, has_target = 0;
        if (std::fread(&g, sizeof g, 1, f) != 1 || std::fread(&n_poses, sizeof n_poses, 1, f) != 1 || std::fread(&has_target, sizeof has_target, 1, f) != 1 ||
            g.nx < 1 || g.ny < 1 || g.nz < 1 || (int64_t)g.nx * g.ny * g.nz > (1 << 16) || g.w < 1 || g.h < 1 || n_poses < 1 || n_poses > DSM_VIEW_MAX_POSES) {
            std::fprintf(stderr, "%s: not a case file\n", argv[a]);
            std::fclose(f);
            return 2;
        }
        const int nx = g.nx, ny = g.ny, nz = g.nz, wx = (nx + 31) / 32;
        const size_t n_words = (size_t)wx * ny * nz, n_vox = (size_t)nx * ny * nz;
        std::vector<float> invs((size_t)16 * n_poses);
        std::vector<int32_t> cams((size_t)3 * n_poses);
        std::vector<uint32_t> occ(n_words), fre(n_words), target(n_words);
        bool whole = std::fread(invs.data(), sizeof(float), invs.size(), f) == invs.size() && std::fread(cams.data(), sizeof(int32_t), cams.size(), f) == cams.size() &&
                     std::fread(occ.data(), sizeof(uint32_t), n_words, f) == n_words && std::fread(fre.data(), sizeof(uint32_t), n_words, f) == n_words;
        if (whole && has_target) whole = std::fread(target.data(), sizeof(uint32_t), n_words, f) == n_words;
        std::fclose(f);
        const int32_t dims[3] = {nx, ny, nz};
        for (size_t i = 0; whole && i < cams.size(); i++) whole = dsm::view_reach_ok(cams[i], dims[i % 3]);
        if (!whole) {
            std::fprintf(stderr, "%s: short case file, or a camera beyond the reach\n", argv[a]);
            return 2;
        }
        std::vector<dsm_view_score> scores((size_t)n_poses), again((size_t)n_poses);
        std::vector<uint32_t> visible(n_words * n_poses);
        std::vector<uint8_t> exits(n_vox * n_poses);
        std::vector<ViewHostLine> lines(n_vox * n_poses);
        const int64_t steps = view_host_score(&g, n_poses, invs.data(), cams.data(), occ.data(), fre.data(), has_target ? target.data() : nullptr, scores.data(),
                                              visible.data(), exits.data(), lines.data());
        // only the lines of the voxels in view: the same scores
        const int64_t steps2 = view_host_score(&g, n_poses, invs.data(), cams.data(), occ.data(), fre.data(), has_target ? target.data() : nullptr, again.data(), nullptr,
                                               nullptr, nullptr);
        size_t bad = steps < 0 || steps != steps2 || memcmp(scores.data(), again.data(), sizeof(dsm_view_score) * (size_t)n_poses) != 0;
        const uint32_t pad = (nx & 31) ? ~((1u << (nx & 31)) - 1u) : 0u;
        int census[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        std::vector<int32_t> fwd, bwd, walk;
        for (int p = 0; p < n_poses; p++) {
            const dsm_view_score &s = scores[(size_t)p];
            int64_t pop = 0, seen = 0, blocked = 0;
            for (size_t i = 0; i < n_words; i++) {
                const uint32_t w = visible[n_words * p + i];
                pop += __builtin_popcount(w);
                bad += (i % wx == (size_t)wx - 1) && (w & pad);
            }
            for (size_t i = 0; i < n_vox; i++) {
                const uint8_t e = exits[n_vox * p + i];
                census[e < 8 ? e : 0]++;
                seen += e == kViewVisible;
                blocked += e == kViewBlocked;
            }
            bad += pop != s.visible || seen != s.visible || s.in_view != s.visible + blocked || s.unknown + s.free + s.occupied != s.visible || s.target > s.visible ||
                   (!has_target && s.target) || s.reserved[0] || s.reserved[1];
            // every line: the closed form from both ends and the error terms from the voxel give one set of points
            for (int z = 0; z < nz; z++)
                for (int y = 0; y < ny; y++)
                    for (int x = 0; x < nx; x++) {
                        const int32_t v[3] = {x, y, z}, *cam = cams.data() + 3 * p;
                        const int32_t n = (int32_t)dsm::view_line_n(cam, v);
                        bad += n != lines[n_vox * p + ((size_t)z * ny + y) * nx + x].n;
                        if (n < 2) continue;
                        const size_t m = (size_t)(n - 1);
                        fwd.assign(3 * m, 0); bwd.assign(3 * m, 0); walk.assign(3 * m, 0);
                        bad += view_host_line(cam, v, fwd.data(), 0, n - 1) != n || view_host_line(v, cam, bwd.data(), 0, n - 1) != n || view_host_walk(v, cam, walk.data(), 0, n - 1) != n;
                        for (size_t k = 0; k < m; k++)
                            for (int i = 0; i < 3; i++) {
                                bad += fwd[3 * k + i] != bwd[3 * (m - 1 - k) + i] || bwd[3 * k + i] != walk[3 * k + i];
                                const int32_t prev = k ? fwd[3 * (k - 1) + i] : cam[i];
                                bad += std::abs(fwd[3 * k + i] - prev) > 1; // (26-adjacent)
                            }
                    }
        }
        if (bad) std::fprintf(stderr, "%s: %zu disagreements\n", argv[a], bad);
        std::printf("%s: %dx%dx%d, %d poses of %dx%d, flags %u: %lld line steps; exits visible %d near %d far %d left %d right %d above %d below %d blocked %d\n", argv[a],
                    nx, ny, nz, n_poses, g.w, g.h, g.flags, (long long)steps, census[0], census[1], census[2], census[3], census[4], census[5], census[6], census[7]);
        ok = ok && bad == 0;
    }
    std::printf("%s\n", ok ? "view_host: consistent" : "view_host: MISMATCH");
    return ok ? 0 : 1;
}
#endif
