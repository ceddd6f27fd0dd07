// grid_shape_host.cpp -- the vocabulary of csrc/dsm_grid_shape.h against its cases, on the host: the shape of a grid and of its bit
// sets, the limit on its dimensions, the layout of a call's scratch, the cap on a list, the cap on a launch.  The voxel-grid calls of
// the C API, the node and the launchers size everything with them.  A stand-alone program (tests/test_cpu_grid_shape.py builds and
// runs it, once plainly and once with the sanitizers); by hand, from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tests/grid_shape_host.cpp -o /tmp/grid_shape_host && /tmp/grid_shape_host
// It includes the header without HIP.
#include "../densesurfelmapping_amd/csrc/dsm_grid_shape.h"

#include <cstdio>
#include <initializer_list>

using namespace dsm;

static int failed = 0;
#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) {                                                               \
            fprintf(stderr, "grid_shape_host.cpp:%d: %s is false\n", __LINE__, #c); \
            failed++;                                                             \
        }                                                                         \
    } while (0)

// a grid of nx x 3 x 2: six rows
static bool dims_are(int nx, int wx, int64_t n_words, int64_t units64, uint32_t last_mask) {
    const GridDims d = grid_dims(nx, 3, 2);
    return d.nx == nx && d.ny == 3 && d.nz == 2 && d.wx == wx && d.rows() == 6 && d.n_vox() == 6 * (int64_t)nx && d.n_words() == n_words &&
           d.set_bytes() == (size_t)n_words * 4 && d.cell_tiles() == 1 && d.units64() == units64 && d.last_mask() == last_mask;
}

static void check_dims() {
    CHECK(dims_are(1, 1, 6, 6, 0x1u));
    CHECK(dims_are(31, 1, 6, 6, 0x7fffffffu));
    CHECK(dims_are(32, 1, 6, 6, 0xffffffffu));
    CHECK(dims_are(33, 2, 12, 6, 0x1u));
    CHECK(dims_are(63, 2, 12, 6, 0x7fffffffu));
    CHECK(dims_are(64, 2, 12, 6, 0xffffffffu));
    CHECK(dims_are(65, 3, 18, 12, 0x1u));
    // exactly 2^28 voxels: 2^14 x 2^14 x 1, 512 words a row
    const GridDims big = grid_dims(1 << 14, 1 << 14, 1);
    CHECK(big.wx == 512 && big.rows() == (1 << 14) && big.n_vox() == ((int64_t)1 << 28) && big.n_words() == ((int64_t)1 << 23));
    CHECK(big.set_bytes() == ((size_t)1 << 25) && big.cell_tiles() == (1 << 15) && big.units64() == ((int64_t)1 << 22) && big.last_mask() == 0xffffffffu);
    // one row of 2^28 voxels, and 2^28 rows of one
    const GridDims row = grid_dims(1 << 28, 1, 1), rows = grid_dims(1, 1 << 14, 1 << 14);
    CHECK(row.wx == (1 << 23) && row.n_words() == ((int64_t)1 << 23) && row.units64() == ((int64_t)1 << 22));
    CHECK(rows.wx == 1 && rows.n_words() == ((int64_t)1 << 28) && rows.set_bytes() == ((size_t)1 << 30) && rows.cell_tiles() == (1 << 20) &&
          rows.units64() == ((int64_t)1 << 28) && rows.last_mask() == 1u);
    // the tiles of the cell list: 256 words each
    CHECK(grid_dims(32, 256, 1).cell_tiles() == 1 && grid_dims(32, 257, 1).cell_tiles() == 2 && grid_dims(33, 128, 1).cell_tiles() == 1 &&
          grid_dims(33, 129, 1).cell_tiles() == 2);
}

static void check_limits() {
    const int64_t m28 = (int64_t)1 << 28, m26 = (int64_t)1 << 26;
    CHECK(kGridMaxVoxels == m28 && kFieldMaxVoxels == m26 && kGridMaxInflate == 16);
    // the default limit, from either side and through either product
    CHECK(grid_dims_ok(1 << 28, 1, 1) && !grid_dims_ok((1 << 28) + 1, 1, 1));
    CHECK(grid_dims_ok(1, 1, 1 << 28) && !grid_dims_ok(1, 1, (1 << 28) + 1));
    CHECK(grid_dims_ok(1 << 14, 1 << 14, 1) && !grid_dims_ok(1 << 14, (1 << 14) + 1, 1) && !grid_dims_ok(1 << 14, 1 << 14, 2));
    CHECK(grid_dims_ok((1 << 14) - 1, (1 << 14) + 1, 1)); // 2^28 - 1
    // the field's limit
    CHECK(grid_dims_ok(1 << 26, 1, 1, m26) && !grid_dims_ok((1 << 26) + 1, 1, 1, m26));
    CHECK(grid_dims_ok(1 << 13, 1 << 13, 1, m26) && !grid_dims_ok(1 << 13, 1 << 13, 2, m26) && !grid_dims_ok(1 << 13, (1 << 13) + 1, 1, m26));
    CHECK(grid_dims_ok(1 << 10, 1 << 10, 1 << 6, m26) && !grid_dims_ok(1 << 10, 1 << 10, (1 << 6) + 1, m26));
    // a dimension below 1
    CHECK(!grid_dims_ok(0, 8, 8) && !grid_dims_ok(8, 0, 8) && !grid_dims_ok(8, 8, 0) && !grid_dims_ok(-1, -1, 1) && !grid_dims_ok(8, 8, INT32_MIN));
    // 2^30 an axis: 2^60 for two, which is more than either limit before the third is multiplied in
    CHECK(!grid_dims_ok(1 << 30, 1 << 30, 1 << 30) && !grid_dims_ok(1 << 30, 1 << 30, 1 << 30, m26) && !grid_dims_ok(INT32_MAX, INT32_MAX, INT32_MAX));
    CHECK(!grid_dims_ok(1 << 30, 1, 1 << 30) && !grid_dims_ok(1, 1 << 30, 1 << 30));
}

// dsm_grid_compose's five parts at 33 x 3 x 2 with room for 5 cells, from 16-byte boundaries: 48 bytes a bit set; the index plane,
// 198 ints, 792 -> 800; the cells, 20 -> 32; one tile count, 4 -> 16
static bool compose_is(bool occ, bool infl, bool index, bool cells, bool tiles, size_t at_occ, size_t at_infl, size_t at_index, size_t at_cells, size_t at_tiles,
                       size_t bytes) {
    const GridDims d = grid_dims(33, 3, 2);
    ScratchPlan plan(16);
    const size_t a = plan.take(occ, d.set_bytes()), b = plan.take(infl, d.set_bytes()), c = plan.take(index, (size_t)d.n_vox() * 4);
    const size_t e = plan.take(cells, capped(5, d.n_vox()) * 4), f = plan.take(tiles, (size_t)d.cell_tiles() * 4);
    return a == at_occ && b == at_infl && c == at_index && e == at_cells && f == at_tiles && plan.bytes() == bytes;
}

static void check_plan() {
    CHECK(compose_is(true, true, true, true, true, 0, 48, 96, 896, 928, 944));     // every plane to the host
    CHECK(compose_is(true, false, false, false, false, 0, 48, 48, 48, 48, 48));    // the occupied set alone
    CHECK(compose_is(false, false, false, false, false, 0, 0, 0, 0, 0, 0));        // the occupied set in the caller's device memory
    CHECK(compose_is(false, true, false, false, true, 0, 0, 48, 48, 48, 64));      // device planes, the cells of the inflated set
    CHECK(compose_is(true, false, true, true, true, 0, 48, 48, 848, 880, 896));    // no inflated plane
    CHECK(compose_is(true, true, false, true, true, 0, 48, 96, 96, 128, 144));     // no index plane
    CHECK(compose_is(false, false, false, false, true, 0, 0, 0, 0, 0, 16));        // the tile counts alone
    // a part of no bytes takes none; one byte takes a whole pad
    ScratchPlan p16(16), p256(256);
    CHECK(p16.take(true, 0) == 0 && p16.take(true, 1) == 0 && p16.take(true, 16) == 16 && p16.take(true, 17) == 32 && p16.bytes() == 64);
    CHECK(p256.take(true, 0) == 0 && p256.take(true, 1) == 0 && p256.take(true, 256) == 256 && p256.take(true, 257) == 512 && p256.bytes() == 1024);
    // field_layout's seven parts at 33 x 3 x 2, from 256-byte boundaries, for every subset of the parts: the table of 64^2 + 1
    // floats, 16388 -> 16640; a byte a voxel, 198 -> 256; a word a voxel, 792 -> 1024; the bit set, 48 -> 256; dist2, 396 -> 512;
    // nearest and distance, 792 -> 1024 each
    const GridDims d = grid_dims(33, 3, 2);
    const size_t n = (size_t)d.n_vox();
    const size_t part[7] = {(64 * 64 + 1) * sizeof(float), n, n * 4, d.set_bytes(), n * 2, n * 4, n * 4};
    const size_t padded[7] = {16640, 256, 1024, 256, 512, 1024, 1024};
    for (unsigned here = 0; here < 128; here++) {
        ScratchPlan plan(256);
        size_t at = 0;
        bool same = true;
        for (int k = 0; k < 7; k++) {
            same = same && plan.take((here >> k) & 1u, part[k]) == at;
            if ((here >> k) & 1u) at += padded[k];
        }
        CHECK(same && plan.bytes() == at);
    }
    // as dsm_grid_distance has them (no bit set, device planes) and dsm_field_compose with host planes
    ScratchPlan dist(256), field(256);
    CHECK(dist.take(true, part[0]) == 0 && dist.take(true, part[1]) == 16640 && dist.take(true, part[2]) == 16896 && dist.take(false, part[3]) == 17920 &&
          dist.bytes() == 17920);
    CHECK(field.take(true, part[0]) == 0 && field.take(true, part[1]) == 16640 && field.take(true, part[2]) == 16896 && field.take(true, part[3]) == 17920 &&
          field.take(true, part[4]) == 18176 && field.take(true, part[5]) == 18688 && field.take(true, part[6]) == 19712 && field.bytes() == 20736);
}

// the clamp as the launchers spelled it before
static int spelled(int64_t n, int per, int cap) { return (int)((n + per - 1) / per < cap ? (n + per - 1) / per : cap); }

static void check_launch_and_cap() {
    const int cases[5][2] = {{256, 8192}, {256, 16384}, {256, 4096}, {4, 16384}, {16, 16384}};
    for (const auto &c : cases) {
        const int per = c[0], cap = c[1];
        const int64_t full = (int64_t)cap * per;
        CHECK(launch_blocks(0, per, cap) == 0 && launch_blocks(1, per, cap) == 1 && launch_blocks(per, per, cap) == 1 && launch_blocks(per + 1, per, cap) == 2);
        CHECK(launch_blocks(full - per, per, cap) == cap - 1 && launch_blocks(full - per + 1, per, cap) == cap);
        CHECK(launch_blocks(full - 1, per, cap) == cap && launch_blocks(full, per, cap) == cap && launch_blocks(full + 1, per, cap) == cap);
        CHECK(launch_blocks((int64_t)1 << 28, per, cap) == cap && launch_blocks(INT32_MAX, per, cap) == cap);
        for (const int64_t n : {(int64_t)0, (int64_t)1, full - 1, full, full + 1, (int64_t)12345}) CHECK(launch_blocks(n, per, cap) == spelled(n, per, cap));
    }
    // no more entries than voxels: 198 of them
    const int64_t n_vox = grid_dims(33, 3, 2).n_vox();
    CHECK(capped(0, n_vox) == 0 && capped(5, n_vox) == 5 && capped(197, n_vox) == 197 && capped(198, n_vox) == 198 && capped(199, n_vox) == 198);
    CHECK(capped(INT32_MAX, n_vox) == 198 && capped(INT32_MAX, (int64_t)1 << 28) == ((size_t)1 << 28));
    // the entries that come back: as many as were counted, no more than fit
    CHECK(capped(0, 5) == 0 && capped(3, 5) == 3 && capped(5, 5) == 5 && capped(143, 2) == 2 && capped(4, 0) == 0);
}

int main() {
    check_dims();
    check_limits();
    check_plan();
    check_launch_and_cap();
    if (failed) {
        fprintf(stderr, "grid_shape_host: %d checks failed\n", failed);
        return 1;
    }
    printf("grid_shape_host: ok\n");
    return 0;
}
