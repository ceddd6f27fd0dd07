// grid_host.cpp -- the voxel grid's definition compiled for the host (tests/test_cpu_grid.py, tests/test_gpu_grid.py): serial
// evaluations of grid_setup / grid_covers / grid_centre of csrc/dsm_math.h, the functions the HIP kernels of csrc/dsm_k_grid.h call.
//   boxed   every surfel that grid_setup keeps visits the voxels of its box
//   brute   every surfel is tested against every voxel of the grid; of grid_setup only the constants of the test are used, its
//           box is ignored and its rejects are restated here
// boxed == brute says that the box loses no covered voxel.  Also: the brute-force inflation (every set voxel against every offset
// of the ball) and the cell list.  Build: g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC.
// With -DGRID_HOST_MAIN the file is a program: both forms over the case files named on the command line (the header of
// tests/grid_cases.py's write_case, then dsm_surfel records) and over random-bit records; exit status 0 iff they agree
// everywhere (run under the sanitizers by the tests).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../densesurfelmapping_amd/csrc/dsm_math.h"
#include "../include/dsm.h"

namespace {

dsm::GridSpec to_grid(const dsm_grid_spec &s) {
    dsm::GridSpec g;
    for (int a = 0; a < 3; a++) g.origin[a] = s.origin[a];
    g.voxel = s.voxel;
    g.n[0] = s.nx; g.n[1] = s.ny; g.n[2] = s.nz;
    return g;
}

// the rejects of the definition, restated
bool brute_keeps(const dsm_surfel &s) {
    if (!std::isfinite(s.px) || !std::isfinite(s.py) || !std::isfinite(s.pz)) return false;
    if (!(s.size >= 0.0f)) return false;
    const float nn = (s.nx * s.nx + s.ny * s.ny) + s.nz * s.nz;
    return std::isfinite(nn) && nn > 0.0f;
}

void voxelise(const dsm_surfel *s, int64_t n, const dsm::GridSpec &g, bool brute, std::vector<int32_t> &index) {
    index.assign((size_t)g.n[0] * g.n[1] * g.n[2], -1);
    std::vector<float> cx((size_t)g.n[0]), cy((size_t)g.n[1]), cz((size_t)g.n[2]);
    for (int i = 0; i < g.n[0]; i++) cx[(size_t)i] = dsm::grid_centre(g.origin[0], g.voxel, i);
    for (int i = 0; i < g.n[1]; i++) cy[(size_t)i] = dsm::grid_centre(g.origin[1], g.voxel, i);
    for (int i = 0; i < g.n[2]; i++) cz[(size_t)i] = dsm::grid_centre(g.origin[2], g.voxel, i);
    for (int64_t i = 0; i < n; i++) {
        dsm::GridSplat sp;
        const bool keep = dsm::grid_setup(g, s[i], (int)i, sp);
        int lo[3] = {0, 0, 0}, hi[3] = {g.n[0], g.n[1], g.n[2]};
        if (brute) {
            if (!brute_keeps(s[i])) continue;
        } else {
            if (!keep) continue;
            for (int a = 0; a < 3; a++) { lo[a] = sp.lo[a]; hi[a] = sp.hi[a]; }
        }
        for (int z = lo[2]; z < hi[2]; z++)
            for (int y = lo[1]; y < hi[1]; y++)
                for (int x = lo[0]; x < hi[0]; x++) {
                    int32_t &v = index[((size_t)z * g.n[1] + y) * g.n[0] + x];
                    if (v < 0 && dsm::grid_covers(sp, cx[(size_t)x], cy[(size_t)y], cz[(size_t)z])) v = (int32_t)i; // (ascending i: the first is the lowest)
                }
    }
}

} // namespace

extern "C" {

// index [nz][ny][nx] and / or the bit set [nz][ny][wx] of the sequence s[0 .. n) (already in order); either may be null
void grid_host(const dsm_surfel *s, int64_t n, const dsm_grid_spec *spec, int brute, int32_t *index, uint32_t *occupied) {
    const dsm::GridSpec g = to_grid(*spec);
    std::vector<int32_t> idx;
    voxelise(s, n, g, brute != 0, idx);
    const int wx = (g.n[0] + 31) / 32;
    if (index) memcpy(index, idx.data(), idx.size() * sizeof(int32_t));
    if (occupied) {
        memset(occupied, 0, (size_t)wx * g.n[1] * g.n[2] * sizeof(uint32_t));
        for (size_t row = 0; row < (size_t)g.n[1] * g.n[2]; row++)
            for (int x = 0; x < g.n[0]; x++)
                if (idx[row * g.n[0] + x] >= 0) occupied[row * wx + (x >> 5)] |= 1u << (x & 31);
    }
}

// every (surfel, voxel) pair on its own, no boxes: covered[i * voxels + linear index] = 0 / 1
void grid_host_pairs(const dsm_surfel *s, int64_t n, const dsm_grid_spec *spec, uint8_t *covered) {
    const dsm::GridSpec g = to_grid(*spec);
    const size_t vox = (size_t)g.n[0] * g.n[1] * g.n[2];
    for (int64_t i = 0; i < n; i++) {
        dsm::GridSplat sp;
        dsm::grid_setup(g, s[i], (int)i, sp);
        const bool keep = brute_keeps(s[i]);
        uint8_t *row = covered + (size_t)i * vox;
        for (int z = 0; z < g.n[2]; z++)
            for (int y = 0; y < g.n[1]; y++)
                for (int x = 0; x < g.n[0]; x++)
                    *row++ = keep && dsm::grid_covers(sp, dsm::grid_centre(g.origin[0], g.voxel, x), dsm::grid_centre(g.origin[1], g.voxel, y),
                                                      dsm::grid_centre(g.origin[2], g.voxel, z));
    }
}

// grid_setup's verdict and box of every record: box[6 i ..] = x0 y0 z0 x1 y1 z1, keep[i]
void grid_host_boxes(const dsm_surfel *s, int64_t n, const dsm_grid_spec *spec, int32_t *box, uint8_t *keep) {
    const dsm::GridSpec g = to_grid(*spec);
    for (int64_t i = 0; i < n; i++) {
        dsm::GridSplat sp;
        keep[i] = dsm::grid_setup(g, s[i], (int)i, sp);
        for (int a = 0; a < 3; a++) { box[6 * i + a] = sp.lo[a]; box[6 * i + 3 + a] = sp.hi[a]; }
    }
}

// brute force: every set voxel of src (pad bits ignored) sets every voxel of dst within the ball of radius r that is inside the grid
void grid_host_inflate(const uint32_t *src, uint32_t *dst, int nx, int ny, int nz, int r) {
    const int wx = (nx + 31) / 32;
    memset(dst, 0, (size_t)wx * ny * nz * sizeof(uint32_t));
    for (int z = 0; z < nz; z++)
        for (int y = 0; y < ny; y++)
            for (int x = 0; x < nx; x++) {
                if (!((src[((size_t)z * ny + y) * wx + (x >> 5)] >> (x & 31)) & 1u)) continue;
                for (int dz = -r; dz <= r; dz++)
                    for (int dy = -r; dy <= r; dy++)
                        for (int dx = -r; dx <= r; dx++) {
                            if (dx * dx + dy * dy + dz * dz > r * r) continue;
                            const int X = x + dx, Y = y + dy, Z = z + dz;
                            if (X < 0 || X >= nx || Y < 0 || Y >= ny || Z < 0 || Z >= nz) continue;
                            dst[((size_t)Z * ny + Y) * wx + (X >> 5)] |= 1u << (X & 31);
                        }
            }
}

// the linear indices of the set voxels (pad bits ignored), ascending, into cells[0 .. cap); returns how many there are
int64_t grid_host_cells(const uint32_t *bits, int nx, int ny, int nz, int32_t *cells, int64_t cap) {
    const int wx = (nx + 31) / 32;
    int64_t n = 0;
    for (int64_t row = 0; row < (int64_t)ny * nz; row++)
        for (int x = 0; x < nx; x++)
            if ((bits[row * wx + (x >> 5)] >> (x & 31)) & 1u) {
                if (n < cap) cells[n] = (int32_t)(row * nx + x);
                n++;
            }
    return n;
}

// the x-dilation width the inflation kernel's table holds for radius r at dy^2 + dz^2 = s (csrc/dsm_math.h)
int grid_host_inflate_width(int r, int s) { return dsm::grid_inflate_width(r, s); }

} // extern "C"

#ifdef GRID_HOST_MAIN
namespace {

bool agree(const std::vector<dsm_surfel> &s, const dsm_grid_spec &spec, const char *what) {
    const dsm::GridSpec g = to_grid(spec);
    std::vector<int32_t> a, b;
    voxelise(s.data(), (int64_t)s.size(), g, false, a);
    voxelise(s.data(), (int64_t)s.size(), g, true, b);
    size_t bad = 0, set = 0;
    for (size_t i = 0; i < a.size(); i++) {
        bad += a[i] != b[i];
        set += b[i] >= 0;
    }
    if (bad) std::fprintf(stderr, "%s %dx%dx%d voxel %g: %zu voxels differ\n", what, spec.nx, spec.ny, spec.nz, (double)spec.voxel, bad);
    // the inflation and the cell list run over the result, for the sanitizers' sake
    const int wx = (spec.nx + 31) / 32;
    std::vector<uint32_t> occ((size_t)wx * spec.ny * spec.nz), infl(occ.size());
    std::vector<int32_t> idx(a.size());
    grid_host(s.data(), (int64_t)s.size(), &spec, 0, idx.data(), occ.data());
    grid_host_inflate(occ.data(), infl.data(), spec.nx, spec.ny, spec.nz, spec.inflate);
    std::vector<int32_t> cells(set);
    if ((size_t)grid_host_cells(occ.data(), spec.nx, spec.ny, spec.nz, cells.data(), (int64_t)cells.size()) != set) {
        std::fprintf(stderr, "%s: the cell list does not count %zu\n", what, set);
        return false;
    }
    std::printf("%s: %zu records, %dx%dx%d, %zu voxels set\n", what, s.size(), spec.nx, spec.ny, spec.nz, set);
    return bad == 0;
}

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint32_t next_u32() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}

} // namespace

int main(int argc, char **argv) {
    bool ok = true;
    for (int a = 1; a < argc; a++) {
        std::FILE *f = std::fopen(argv[a], "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        dsm_grid_spec spec;
        if (std::fread(&spec, sizeof spec, 1, f) != 1 || spec.struct_size != sizeof spec || spec.nx < 1 || spec.ny < 1 || spec.nz < 1 ||
            (int64_t)spec.nx * spec.ny * spec.nz > (1 << 22) || spec.inflate < 0 || spec.inflate > 16) {
            std::fprintf(stderr, "%s: not a case file\n", argv[a]);
            std::fclose(f);
            return 2;
        }
        std::vector<dsm_surfel> s;
        dsm_surfel r;
        while (std::fread(&r, sizeof r, 1, f) == 1) s.push_back(r);
        std::fclose(f);
        ok = agree(s, spec, argv[a]) && ok;
    }
    std::vector<dsm_surfel> rnd(3000);
    for (dsm_surfel &r : rnd) {
        uint32_t w[11];
        for (uint32_t &v : w) v = next_u32();
        memcpy(&r, w, sizeof r);
        if (next_u32() & 1) { // half of them with a position and a size of ordinary magnitude: NaN patterns elsewhere
            r.px = (float)(int32_t)(next_u32() % 2001 - 1000) * 0.004f;
            r.py = (float)(int32_t)(next_u32() % 2001 - 1000) * 0.004f;
            r.pz = (float)(next_u32() % 4000) * 0.001f - 2.0f;
            if (next_u32() & 1) r.size = (float)(next_u32() % 1000) * 0.001f;
        }
    }
    const dsm_grid_spec specs[2] = {{(uint32_t)sizeof(dsm_grid_spec), {-4.0f, -4.0f, -2.0f}, 0.25f, 33, 32, 16, 2},
                                    {(uint32_t)sizeof(dsm_grid_spec), {100.3f, -250.7f, 3.2f}, 0.1f, 33, 9, 5, 1}};
    for (const dsm_grid_spec &spec : specs) ok = agree(rnd, spec, "random bits") && ok;
    std::printf("%s\n", ok ? "grid_host: boxed == brute" : "grid_host: MISMATCH");
    return ok ? 0 : 1;
}
#endif
