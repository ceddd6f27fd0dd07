// field_host.cpp -- the distance field's definition compiled for the host (tests/test_cpu_field.py, tests/test_gpu_field.py): for
// every voxel the minimum of field_key (csrc/dsm_math.h) over the set voxels within R, evaluated directly, with none of the
// passes of csrc/dsm_k_field.h.  Two brute-force forms of the same minimum:
//   list     every voxel against the list of all set voxels
//   window   every voxel against every position of its (2R + 1)^3 window clipped to the grid
// field_host takes whichever visits fewer pairs; the program below compares the two.  The `distance` plane goes through
// field_table_entry, the function the library builds its table with.  Build: g++ -std=c++17 -O2 -fopenmp -shared -fPIC (the
// voxels are independent: with OpenMP the rows are shared out among threads; without it the file is the same program, serial).
// With -DFIELD_HOST_MAIN the file is a program: both forms over the case files named on the command line (tests/field_cases.py's
// write_case: nx ny nz R as int32, the voxel edge as a float, then the words of the bit set); exit status 0 iff they agree everywhere
// (run under the sanitizers by the tests).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../densesurfelmapping_amd/csrc/dsm_math.h"
#include "../include/dsm.h"

namespace {

struct Field {
    std::vector<uint64_t> key; // per voxel: the minimum key, or ~0 when no set voxel lies within R
};

bool bit(const uint32_t *bits, int wx, int64_t row, int x) { return (bits[row * wx + (x >> 5)] >> (x & 31)) & 1u; }

uint64_t key_of(int x, int y, int z, int ox, int oy, int oz, int nx, int ny) {
    const int dx = ox - x, dy = oy - y, dz = oz - z;
    return dsm::field_key((uint32_t)((dx * dx + dy * dy) + dz * dz), (uint32_t)(((int64_t)oz * ny + oy) * nx + ox));
}

void field_list(const uint32_t *bits, int nx, int ny, int nz, int r, Field &f) {
    const int wx = (nx + 31) / 32;
    std::vector<int32_t> set; // x, y, z of every set voxel (pad bits never looked at)
    for (int z = 0; z < nz; z++)
        for (int y = 0; y < ny; y++)
            for (int x = 0; x < nx; x++)
                if (bit(bits, wx, (int64_t)z * ny + y, x)) { set.push_back(x); set.push_back(y); set.push_back(z); }
    f.key.assign((size_t)nx * ny * nz, ~0ull);
    const uint64_t limit = (uint64_t)(r * r);
#pragma omp parallel for schedule(static)
    for (int64_t row = 0; row < (int64_t)ny * nz; row++) // (every voxel on its own: with -fopenmp the rows are shared out)
        for (int x = 0; x < nx; x++) {
            const int y = (int)(row % ny), z = (int)(row / ny);
            uint64_t best = ~0ull;
            for (size_t k = 0; k < set.size(); k += 3) {
                const uint64_t key = key_of(x, y, z, set[k], set[k + 1], set[k + 2], nx, ny);
                if ((key >> 32) <= limit && key < best) best = key;
            }
            f.key[(size_t)row * nx + x] = best;
        }
}

void field_window(const uint32_t *bits, int nx, int ny, int nz, int r, Field &f) {
    const int wx = (nx + 31) / 32;
    f.key.assign((size_t)nx * ny * nz, ~0ull);
    const uint64_t limit = (uint64_t)(r * r);
#pragma omp parallel for schedule(static)
    for (int64_t row = 0; row < (int64_t)ny * nz; row++)
        for (int x = 0; x < nx; x++) {
            const int y = (int)(row % ny), z = (int)(row / ny);
            uint64_t best = ~0ull;
            for (int oz = z - r < 0 ? 0 : z - r; oz <= z + r && oz < nz; oz++)
                for (int oy = y - r < 0 ? 0 : y - r; oy <= y + r && oy < ny; oy++)
                    for (int ox = x - r < 0 ? 0 : x - r; ox <= x + r && ox < nx; ox++) {
                        if (!bit(bits, wx, (int64_t)oz * ny + oy, ox)) continue;
                        const uint64_t key = key_of(x, y, z, ox, oy, oz, nx, ny);
                        if ((key >> 32) <= limit && key < best) best = key;
                    }
            f.key[(size_t)row * nx + x] = best;
        }
}

int64_t count_set(const uint32_t *bits, int nx, int ny, int nz) {
    const int wx = (nx + 31) / 32;
    int64_t n = 0;
    for (int64_t row = 0; row < (int64_t)ny * nz; row++)
        for (int x = 0; x < nx; x++) n += bit(bits, wx, row, x);
    return n;
}

int64_t clipped(int n, int r) { return n < 2 * r + 1 ? n : 2 * r + 1; }

} // namespace

extern "C" {

// table[k], k = 0 .. r * r: the metres of squared distance k
void field_host_table(float voxel, int r, float *table) {
    for (int k = 0; k <= r * r; k++) table[k] = dsm::field_table_entry(voxel, k);
}

// the planes [nz][ny][nx] of the bit set [nz][ny][wx]; any plane may be null.  form: 0 = whichever is cheaper, 1 = list, 2 = window
void field_host(const uint32_t *bits, int nx, int ny, int nz, int r, float voxel, int form, uint16_t *dist2, int32_t *nearest, float *distance) {
    Field f;
    if (form == 0) form = count_set(bits, nx, ny, nz) <= clipped(nx, r) * clipped(ny, r) * clipped(nz, r) ? 1 : 2;
    if (form == 1) field_list(bits, nx, ny, nz, r, f); else field_window(bits, nx, ny, nz, r, f);
    std::vector<float> table((size_t)(r * r + 1));
    field_host_table(voxel, r, table.data());
    for (size_t i = 0; i < f.key.size(); i++) {
        const bool have = f.key[i] != ~0ull;
        if (dist2) dist2[i] = have ? (uint16_t)(f.key[i] >> 32) : (uint16_t)DSM_FIELD_FAR;
        if (nearest) nearest[i] = have ? (int32_t)(uint32_t)f.key[i] : -1;
        if (distance) distance[i] = table[have ? (size_t)(f.key[i] >> 32) : (size_t)(r * r)];
    }
}

} // extern "C"

#ifdef FIELD_HOST_MAIN
int main(int argc, char **argv) {
    bool ok = true;
    for (int a = 1; a < argc; a++) {
        std::FILE *f = std::fopen(argv[a], "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        int32_t hdr[4];
        float voxel;
        if (std::fread(hdr, sizeof hdr, 1, f) != 1 || std::fread(&voxel, sizeof voxel, 1, f) != 1 || hdr[0] < 1 || hdr[1] < 1 || hdr[2] < 1 ||
            (int64_t)hdr[0] * hdr[1] * hdr[2] > (1 << 16) || hdr[3] < 1 || hdr[3] > DSM_FIELD_MAX_DIST) {
            std::fprintf(stderr, "%s: not a case file\n", argv[a]);
            std::fclose(f);
            return 2;
        }
        const int nx = hdr[0], ny = hdr[1], nz = hdr[2], r = hdr[3];
        std::vector<uint32_t> bits((size_t)((nx + 31) / 32) * ny * nz);
        const bool whole = std::fread(bits.data(), sizeof(uint32_t), bits.size(), f) == bits.size();
        std::fclose(f);
        if (!whole) {
            std::fprintf(stderr, "%s: short bit set\n", argv[a]);
            return 2;
        }
        const size_t vox = (size_t)nx * ny * nz;
        std::vector<uint16_t> d2[2] = {std::vector<uint16_t>(vox), std::vector<uint16_t>(vox)};
        std::vector<int32_t> near[2] = {std::vector<int32_t>(vox), std::vector<int32_t>(vox)};
        std::vector<float> dist[2] = {std::vector<float>(vox), std::vector<float>(vox)};
        for (int form = 1; form <= 2; form++)
            field_host(bits.data(), nx, ny, nz, r, voxel, form, d2[form - 1].data(), near[form - 1].data(), dist[form - 1].data());
        size_t bad = 0, found = 0;
        for (size_t i = 0; i < vox; i++) {
            bad += d2[0][i] != d2[1][i] || near[0][i] != near[1][i] || memcmp(&dist[0][i], &dist[1][i], sizeof(float)) != 0;
            found += near[0][i] >= 0;
        }
        if (bad) std::fprintf(stderr, "%s: %zu voxels differ between the list and the window form\n", argv[a], bad);
        std::printf("%s: %dx%dx%d R %d, %lld set, %zu voxels with a set voxel in reach\n", argv[a], nx, ny, nz, r, (long long)count_set(bits.data(), nx, ny, nz), found);
        ok = ok && bad == 0;
    }
    std::printf("%s\n", ok ? "field_host: list == window" : "field_host: MISMATCH");
    return ok ? 0 : 1;
}
#endif
