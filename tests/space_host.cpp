// space_host.cpp -- free space and the three-state map on the host (tests/test_cpu_space.py, tests/test_gpu_space.py): the
// definitions of csrc/dsm_carve.h evaluated directly, with none of the arrangements of csrc/dsm_k_carve.h.
//   carve      a brute-force loop of carve_voxel over every voxel and every frame -- no voxel is skipped because it is free
//              already, no frame because an earlier one freed the voxel -- OR-ed into the old set (or stored over it); the exit
//              of every (frame, voxel) pair can be had, for the census of the tests
//   project    the camera-frame depth and the pixel of every voxel centre for one frame, restated with the definition's expressions:
//              what the tests craft depths from (a depth set from the checker's own q.z puts a voxel on a margin)
//   classify   per voxel, neighbour by neighbour, bit by bit: it shares nothing with the word-parallel kernel
// Build: g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC.  With -DSPACE_HOST_MAIN the file is a program: for every case file
// named on the command line (tests/space_cases.py's write_case) it carves all frames in one call and frame by frame, in both
// orders, compares the three sets, classifies the result against the case's occupied set and checks the planes against one
// another; exit status 0 iff everything agrees (run under the sanitizers by the tests).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../densesurfelmapping_amd/csrc/dsm_math.h"
#include "../include/dsm.h"

extern "C" {

struct SpaceHostGrid { // the scalars of a carve: tests/space_cases.py's _Grid
    float origin[3];
    float voxel;
    int32_t nx, ny, nz;
    int32_t w, h, pitch;
    float fx, fy, cx, cy;
    float near_d, far_d, margin;
    uint32_t flags;
};

} // extern "C"

namespace {

dsm::CarveConst carve_const(const SpaceHostGrid &g, const float *inv16) {
    dsm::CarveConst c;
    memset(&c, 0, sizeof c);
    for (int a = 0; a < 3; a++) c.origin[a] = g.origin[a];
    c.voxel = g.voxel;
    c.w = g.w; c.h = g.h; c.pitch = g.pitch;
    c.fx = g.fx; c.fy = g.fy; c.cx = g.cx; c.cy = g.cy;
    c.near_d = g.near_d; c.far_d = g.far_d; c.margin = g.margin;
    c.flags = g.flags;
    for (int k = 0; k < 16; k++) c.inv[k] = inv16[k];
    return c;
}

bool bit(const uint32_t *bits, int wx, int64_t row, int x) { return (bits[row * wx + (x >> 5)] >> (x & 31)) & 1u; }

} // namespace

extern "C" {

// the closed-form inverse the library takes when the caller gives none
void space_host_inverse(const float *pose16, float *inv16) { dsm::inverse4<float>(pose16, inv16); }

// bits ([nz][ny][wx], read and written): |= the voxels some frame frees (DSM_CARVE_REPLACE in g->flags: = those voxels); pad bits
// written 0.  invs: [n_frames][16], depths: [n_frames][h * pitch].  exits (may be null): [n_frames][nz][ny][nx] CarveExit of every
// pair.  Returns the population count afterwards.
int64_t space_host_carve(const SpaceHostGrid *g, int n_frames, const float *invs, const float *depths, uint32_t *bits, uint8_t *exits) {
    const int nx = g->nx, ny = g->ny, nz = g->nz, wx = (nx + 31) / 32;
    const size_t plane = (size_t)g->h * g->pitch, n_vox = (size_t)nx * ny * nz;
    std::vector<uint8_t> freed(n_vox, 0);
    for (int f = 0; f < n_frames; f++) {
        const dsm::CarveConst c = carve_const(*g, invs + 16 * f);
        for (int z = 0; z < nz; z++)
            for (int y = 0; y < ny; y++)
                for (int x = 0; x < nx; x++) {
                    const size_t i = ((size_t)z * ny + y) * nx + x;
                    const dsm::CarveExit e = dsm::carve_voxel(c, depths + plane * f, x, y, z);
                    if (exits) exits[n_vox * f + i] = (uint8_t)e;
                    if (e == dsm::kCarveFree) freed[i] = 1;
                }
    }
    int64_t count = 0;
    for (int64_t row = 0; row < (int64_t)ny * nz; row++)
        for (int w = 0; w < wx; w++) {
            uint32_t word = 0;
            for (int b = 0; b < 32; b++) {
                const int x = w * 32 + b;
                if (x >= nx) break;
                const bool old = !(g->flags & DSM_CARVE_REPLACE) && bit(bits, wx, row, x);
                if (old || freed[(size_t)row * nx + x]) word |= 1u << b;
            }
            bits[row * wx + w] = word;
            count += __builtin_popcount(word);
        }
    return count;
}

// q.z, u, v of every voxel centre against one frame, [nz][ny][nx] each, with the definition's expressions (u, v: INT32_MIN where
// the rounding has no int)
void space_host_project(const SpaceHostGrid *g, const float *inv16, float *qz, int32_t *u, int32_t *v) {
    size_t i = 0;
    for (int z = 0; z < g->nz; z++)
        for (int y = 0; y < g->ny; y++)
            for (int x = 0; x < g->nx; x++, i++) {
                const float p[3] = {dsm::grid_centre(g->origin[0], g->voxel, x), dsm::grid_centre(g->origin[1], g->voxel, y), dsm::grid_centre(g->origin[2], g->voxel, z)};
                float q[3];
                dsm::xform_point(inv16, p, q);
                qz[i] = q[2];
                u[i] = dsm::round_to_pixel((q[0] * g->fx) / q[2] + g->cx);
                v[i] = dsm::round_to_pixel((q[1] * g->fy) / q[2] + g->cy);
            }
}

// the three states, the known-free set, the frontier and its ascending cell list of two bit sets; any output may be null; no cell
// is written at or beyond cap.  Returns the number of frontier voxels.
int32_t space_host_classify(const uint32_t *occ, const uint32_t *fre, int nx, int ny, int nz, uint8_t *state, uint32_t *known_free, uint32_t *frontier,
                            int32_t *cells, int32_t cap) {
    const int wx = (nx + 31) / 32;
    const size_t n_words = (size_t)wx * ny * nz;
    if (known_free) memset(known_free, 0, n_words * sizeof(uint32_t));
    if (frontier) memset(frontier, 0, n_words * sizeof(uint32_t));
    const auto state_of = [&](int x, int y, int z) {
        const int64_t row = (int64_t)z * ny + y;
        return dsm::space_state(bit(occ, wx, row, x), bit(fre, wx, row, x));
    };
    static const int kFace[6][3] = {{-1, 0, 0}, {1, 0, 0}, {0, -1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1}};
    int32_t count = 0;
    for (int z = 0; z < nz; z++)
        for (int y = 0; y < ny; y++)
            for (int x = 0; x < nx; x++) {
                const int64_t row = (int64_t)z * ny + y;
                const uint8_t s = state_of(x, y, z);
                if (state) state[row * nx + x] = s;
                if (s != DSM_SPACE_FREE) continue;
                if (known_free) known_free[row * wx + (x >> 5)] |= 1u << (x & 31);
                bool edge = false;
                for (const int *d : kFace) {
                    const int ax = x + d[0], ay = y + d[1], az = z + d[2];
                    if (ax < 0 || ax >= nx || ay < 0 || ay >= ny || az < 0 || az >= nz) continue; // outside the grid nothing is unknown
                    if (state_of(ax, ay, az) == DSM_SPACE_UNKNOWN) edge = true;
                }
                if (!edge) continue;
                if (frontier) frontier[row * wx + (x >> 5)] |= 1u << (x & 31);
                if (cells && count < cap) cells[count] = (int32_t)(row * nx + x);
                count++;
            }
    return count;
}

} // extern "C"

#ifdef SPACE_HOST_MAIN
int main(int argc, char **argv) {
    bool ok = true;
    for (int a = 1; a < argc; a++) {
        std::FILE *f = std::fopen(argv[a], "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        SpaceHostGrid g;
        int32_t n_frames = 0;
        if (std::fread(&g, sizeof g, 1, f) != 1 || std::fread(&n_frames, sizeof n_frames, 1, f) != 1 || g.nx < 1 || g.ny < 1 || g.nz < 1 ||
            (int64_t)g.nx * g.ny * g.nz > (1 << 16) || g.w < 1 || g.h < 1 || g.pitch < g.w || (int64_t)g.h * g.pitch > (1 << 16) || n_frames < 1 ||
            n_frames > DSM_CARVE_MAX_FRAMES) {
            std::fprintf(stderr, "%s: not a case file\n", argv[a]);
            std::fclose(f);
            return 2;
        }
        const int nx = g.nx, ny = g.ny, nz = g.nz, wx = (nx + 31) / 32;
        const size_t n_words = (size_t)wx * ny * nz, n_vox = (size_t)nx * ny * nz, plane = (size_t)g.h * g.pitch;
        std::vector<float> invs((size_t)16 * n_frames), depths(plane * n_frames);
        std::vector<uint32_t> old(n_words), occ(n_words);
        const bool whole = std::fread(invs.data(), sizeof(float), invs.size(), f) == invs.size() && std::fread(depths.data(), sizeof(float), depths.size(), f) == depths.size() &&
                           std::fread(old.data(), sizeof(uint32_t), n_words, f) == n_words && std::fread(occ.data(), sizeof(uint32_t), n_words, f) == n_words;
        std::fclose(f);
        if (!whole) {
            std::fprintf(stderr, "%s: short case file\n", argv[a]);
            return 2;
        }
        // all frames at once; frame by frame forwards; frame by frame backwards: one set
        std::vector<uint32_t> at_once = old, forwards = old, backwards = old;
        std::vector<uint8_t> exits(n_vox * n_frames);
        const int64_t n_free = space_host_carve(&g, n_frames, invs.data(), depths.data(), at_once.data(), exits.data());
        SpaceHostGrid or_in = g;
        int64_t n_fwd = 0, n_bwd = 0;
        for (int k = 0; k < n_frames; k++) {
            n_fwd = space_host_carve(&or_in, 1, invs.data() + 16 * k, depths.data() + plane * k, forwards.data(), nullptr);
            const int r = n_frames - 1 - k;
            n_bwd = space_host_carve(&or_in, 1, invs.data() + 16 * r, depths.data() + plane * r, backwards.data(), nullptr);
            or_in.flags &= ~(uint32_t)DSM_CARVE_REPLACE; // (a replacing carve replaces once)
        }
        size_t bad = 0;
        for (size_t i = 0; i < n_words; i++) bad += at_once[i] != forwards[i] || at_once[i] != backwards[i];
        bad += n_free != n_fwd || n_free != n_bwd;
        int census[6] = {0, 0, 0, 0, 0, 0};
        for (uint8_t e : exits) census[e < 6 ? e : 0]++;
        // the planes of the classification against one another
        std::vector<uint8_t> state(n_vox);
        std::vector<uint32_t> kf(n_words), fr(n_words);
        std::vector<int32_t> cells(n_vox + 1);
        const int32_t n_cells = space_host_classify(occ.data(), at_once.data(), nx, ny, nz, state.data(), kf.data(), fr.data(), cells.data(), (int32_t)n_vox);
        int64_t listed = 0;
        for (size_t i = 0; i < n_words; i++) {
            bad += (fr[i] & ~kf[i]) != 0 || (kf[i] & occ[i]) != 0;
            listed += __builtin_popcount(fr[i]);
        }
        bad += listed != n_cells;
        for (int32_t k = 0; k < n_cells; k++) {
            const int32_t c = cells[(size_t)k];
            bad += c < 0 || (size_t)c >= n_vox || state[(size_t)c] != DSM_SPACE_FREE || (k > 0 && cells[(size_t)k - 1] >= c);
        }
        if (bad) std::fprintf(stderr, "%s: %zu disagreements\n", argv[a], bad);
        std::printf("%s: %dx%dx%d, %d frames of %dx%d (pitch %d): %lld free, %d frontier; exits free %d range %d outside %d nodepth %d infinite %d notinfront %d\n",
                    argv[a], nx, ny, nz, n_frames, g.w, g.h, g.pitch, (long long)n_free, n_cells, census[0], census[1], census[2], census[3], census[4], census[5]);
        ok = ok && bad == 0;
    }
    std::printf("%s\n", ok ? "space_host: consistent" : "space_host: MISMATCH");
    return ok ? 0 : 1;
}
#endif
