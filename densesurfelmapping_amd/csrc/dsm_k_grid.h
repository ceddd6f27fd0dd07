// dsm_k_grid.h -- the surfel map as a world-aligned occupancy voxel grid (dsm_grid_compose, dsm_grid_inflate): the lowest surfel
// number covering every voxel, the occupied bit set, its inflation by a sphere of voxels, and the list of set cells.  The
// definition (grid_setup / grid_covers / grid_centre) is in dsm_math.h and shared with the host checker tests/grid_host.cpp; this
// file is how it is evaluated:
//   k_grid_clear       the index plane to -1 or the bit set to 0 (whichever is splatted into), and the two list counts
//   k_grid_setup_map   the map part and the runs of the surfel sequence (dsm_k_sequence.h: map_tile_walk, run_source): a lane per
//   k_grid_setup_run   surfel does grid_setup; survivors are appended as GridSplat records to ONE array, small boxes from the
//                      front, large ones from the back (two_ended_slot)
//   k_grid_splat       the small list: 16 lanes per surfel, four surfels per wave.  The 16 lanes take 16 voxels along x from a
//                      multiple of 16, so they share one word of the bit set: the wave's ballot gives each group its 16 bits
//                      and one lane ORs them in -- or every lane does its atomicMin on 16 contiguous ints of the index plane
//   k_grid_splat_big   the large list: a workgroup per surfel in turn (grid-stride); a wave takes 64 voxels along x from a
//                      multiple of 64 (two words of a ballot), the four waves take rows
//   k_grid_bits        with an index plane: the bit set from index != -1, a wave per 64 voxels of a row (every word is written)
//   k_grid_inflate     bit-parallel dilation on 32-voxel words, a tile of row words with its y/z halo and one word of x halo
//                      each side in LDS; for each (dy, dz) inside the radius the source row dilated along x by the table's width
//   k_grid_cell_count / k_cloud_scan / k_grid_cell_scatter   popcount per word, scan, ordered scatter of the linear indices
//                      (launch_cell_list: also the frontier's list and the component counts)
// A voxel does a plain load first and skips the atomic when nothing would change: bits only get set and indices only decrease,
// so a stale value can cost an atomic, never a wrong skip.  The atomics are atomicOr / atomicMin / atomicAdd on 32-bit integers,
// plain C++.  What has been measured on this chip (MI355X_MICROARCH.md, global float atomics) is the no-return fp32 add; the
// rates of the 32-bit integer OR and min are NOT measured there -- the lanes of a surfel lie along x on the assumption that
// they coalesce like the adds.  Every loop is bounded by a clipped box or by the grid; the lists cannot overflow (the array
// is as long as the sequence); no workgroup waits on another.
#pragma once
#include "dsm_k_cloud.h"

namespace dsm {

__global__ __launch_bounds__(256) void k_grid_clear(uint32_t *__restrict__ plane, int64_t n, uint32_t value, int32_t *__restrict__ counts) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) plane[i] = value;
    if (blockIdx.x == 0 && threadIdx.x < 2) counts[threadIdx.x] = 0;
}

struct GridSetupArgs {
    GridSpec g;
    int32_t n_seq; // length of the splat array = an upper bound of the sequence's length
};

// called by whole waves; `valid` lanes hold record r with sequence number `number`
__device__ __forceinline__ void grid_emit(const GridSetupArgs &a, bool valid, const dsm_surfel *__restrict__ r, int number,
                                          GridSplat *__restrict__ splats, int32_t *__restrict__ counts) {
    GridSplat s = {};
    bool keep = false;
    if (valid) keep = grid_setup(a.g, *r, number, s);
    const int64_t rows = (int64_t)(s.hi[1] - s.lo[1]) * (s.hi[2] - s.lo[2]);
    const bool small = keep && s.hi[0] - s.lo[0] <= kGridSmallW && rows <= kGridSmallRows;
    const int slot = two_ended_slot(small, keep && !small, counts, a.n_seq);
    if (keep && slot >= 0 && slot < a.n_seq) splats[slot] = s; // (always: survivors <= sequence <= n_seq)
}

__global__ __launch_bounds__(256) void k_grid_setup_map(const MapPart mp, int base, const GridSetupArgs a, GridSplat *__restrict__ splats,
                                                        int32_t *__restrict__ counts) {
    map_tile_walk(mp, base, [&](unsigned long long m, int at, int i) {
        if (m) // (wave-uniform)
            grid_emit(a, (m >> lane_id()) & 1ull, mp.rec + i, at + rank_below(m), splats, counts);
    });
}

// output j of the runs is surfel j of the sequence.  A wave takes 64 consecutive outputs at a time.
__global__ __launch_bounds__(256) void k_grid_setup_run(const dsm_surfel *__restrict__ src, const RunTable rt, const GridSetupArgs a,
                                                        GridSplat *__restrict__ splats, int32_t *__restrict__ counts) {
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    for (int64_t j0 = ((int64_t)blockIdx.x * 4 + wv) * 64; j0 < rt.total; j0 += (int64_t)gridDim.x * 256) {
        const int j = (int)j0 + lane;
        const bool valid = j < rt.total;
        grid_emit(a, valid, valid ? src + run_source(rt, j) : src, j, splats, counts);
    }
}

struct GridTarget {
    GridSpec g;
    int wx;          // words per row of the bit set
    uint32_t *index; // [nz][ny][nx] as unsigned: -1 = 0xffffffff is the largest, so atomicMin keeps the lowest number; or null
    uint32_t *bits;  // [nz][ny][wx]: splatted into when index is null
};

// box inside the grid, whatever the record holds
__device__ __forceinline__ void grid_box(const GridSpec &g, const GridSplat &s, int lo[3], int hi[3]) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
        lo[a] = s.lo[a] > 0 ? s.lo[a] : 0;
        hi[a] = s.hi[a] < g.n[a] ? s.hi[a] : g.n[a];
    }
}

__device__ __forceinline__ void grid_index_min(const GridTarget &t, int x, int y, int z, uint32_t number) {
    uint32_t *p = t.index + (((int64_t)z * t.g.n[1] + y) * t.g.n[0] + x);
    if (*p > number) atomicMin(p, number);
}

__device__ __forceinline__ void grid_bits_or(const GridTarget &t, int xw, int y, int z, uint32_t bits) {
    uint32_t *p = t.bits + (((int64_t)z * t.g.n[1] + y) * t.wx + xw);
    if (bits & ~*p) atomicOr(p, bits);
}

// 16 lanes per surfel.  The wave's loop is uniform (the ballot needs every lane): a group that has run out of surfels or of
// rows goes along with nothing covered.
__global__ __launch_bounds__(256) void k_grid_splat(const GridSplat *__restrict__ splats, const int32_t *__restrict__ counts, int n_seq, const GridTarget t) {
    const int n = counts[0] < n_seq ? counts[0] : n_seq;
    const int sub = threadIdx.x >> 4, l = threadIdx.x & 15, grp = (threadIdx.x >> 4) & 3;
    for (int64_t i0 = (int64_t)blockIdx.x * 16; i0 < n; i0 += (int64_t)gridDim.x * 16) {
        const int64_t i = i0 + sub;
        const bool have = i < n;
        GridSplat s = {};
        if (have) s = splats[i];
        int lo[3], hi[3];
        grid_box(t.g, s, lo, hi);
        const int xa = lo[0] & ~15; // chunks of 16 voxels from a multiple of 16: inside one word
        const int chunks = have && hi[0] > lo[0] ? (hi[0] - xa + 15) >> 4 : 0;
        int c = 0, y = lo[1], z = lo[2];
        bool live = chunks > 0 && y < hi[1] && z < hi[2];
        while (__ballot(live)) {
            bool covered = false;
            const int x = xa + c * 16 + l;
            if (live && x >= lo[0] && x < hi[0])
                covered = grid_covers(s, grid_centre(t.g.origin[0], t.g.voxel, x), grid_centre(t.g.origin[1], t.g.voxel, y),
                                      grid_centre(t.g.origin[2], t.g.voxel, z));
            if (t.index) {
                if (covered) grid_index_min(t, x, y, z, (uint32_t)s.number);
            } else {
                const unsigned long long m = __ballot(covered);
                const uint32_t mine = (uint32_t)(m >> (grp * 16)) & 0xffffu;
                if (l == 0 && mine) grid_bits_or(t, x >> 5, y, z, mine << (x & 31));
            }
            if (live) { // the next chunk, row, slice of this group's box
                if (++c == chunks) {
                    c = 0;
                    if (++y == hi[1]) {
                        y = lo[1];
                        if (++z == hi[2]) live = false;
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_grid_splat_big(const GridSplat *__restrict__ splats, const int32_t *__restrict__ counts, int n_seq, const GridTarget t) {
    const int n = counts[1] < n_seq ? counts[1] : n_seq;
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const GridSplat s = splats[n_seq - 1 - i];
        int lo[3], hi[3];
        grid_box(t.g, s, lo, hi);
        if (lo[0] >= hi[0] || lo[1] >= hi[1] || lo[2] >= hi[2]) continue; // (block-uniform)
        const int xa = lo[0] & ~63;
        const int64_t rows = (int64_t)(hi[1] - lo[1]) * (hi[2] - lo[2]);
        for (int64_t row = wv; row < rows; row += 4) { // (wave-uniform)
            const int y = lo[1] + (int)(row % (hi[1] - lo[1])), z = lo[2] + (int)(row / (hi[1] - lo[1]));
            const float cy = grid_centre(t.g.origin[1], t.g.voxel, y), cz = grid_centre(t.g.origin[2], t.g.voxel, z);
            for (int xb = xa; xb < hi[0]; xb += 64) {
                const int x = xb + lane;
                const bool covered = x >= lo[0] && x < hi[0] && grid_covers(s, grid_centre(t.g.origin[0], t.g.voxel, x), cy, cz);
                if (t.index) {
                    if (covered) grid_index_min(t, x, y, z, (uint32_t)s.number);
                } else {
                    const unsigned long long m = __ballot(covered);
                    const uint32_t mine = (uint32_t)(m >> (lane & 32));
                    if ((lane & 31) == 0 && mine) grid_bits_or(t, x >> 5, y, z, mine);
                }
            }
        }
    }
}

// the bit set from the index plane: a wave per 64 voxels of a row, every word of the set written (pad bits 0)
__global__ __launch_bounds__(256) void k_grid_bits(const uint32_t *__restrict__ index, uint32_t *__restrict__ bits, int nx, int wx, int64_t rows) {
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    const int per_row = (nx + 63) >> 6;
    const int64_t units = rows * per_row;
    for (int64_t u = (int64_t)blockIdx.x * 4 + wv; u < units; u += (int64_t)gridDim.x * 4) {
        const int64_t row = u / per_row;
        const int x = (int)(u % per_row) * 64 + lane;
        const bool set = x < nx && index[row * nx + x] != 0xffffffffu;
        const unsigned long long m = __ballot(set);
        if ((lane & 31) == 0 && (x >> 5) < wx) bits[row * wx + (x >> 5)] = (uint32_t)(m >> (lane & 32));
    }
}

// ---- inflation
constexpr int kGridTileW = 8, kGridTileY = 8, kGridTileZ = 4; // output words per workgroup: 8 along x, 8 rows, 4 slices = 256
struct GridInflateArgs {
    GridDims g;
    int r;
    uint8_t width[kGridMaxInflate * kGridMaxInflate + 1]; // by dy^2 + dz^2: grid_inflate_width (host-built)
};
static_assert(sizeof(GridInflateArgs) == 280 && offsetof(GridInflateArgs, r) == 16 && offsetof(GridInflateArgs, width) == 20, "as the kernel was built for");

// OR of v << s for s = 0 .. k (k <= 16) by doubling: after the loop v holds the shifts 0 .. have - 1, and 2 have > k + 1
__device__ __forceinline__ unsigned long long grid_smear_up(unsigned long long v, int k) {
    int have = 1;
    while (2 * have <= k + 1) {
        v |= v << have;
        have *= 2;
    }
    return v | (v << (k + 1 - have));
}
__device__ __forceinline__ unsigned long long grid_smear_down(unsigned long long v, int k) {
    int have = 1;
    while (2 * have <= k + 1) {
        v |= v >> have;
        have *= 2;
    }
    return v | (v >> (k + 1 - have));
}

// LDS: [tz + 2r][ty + 2r][tw + 2] source words, pad bits and everything outside the grid 0
__global__ __launch_bounds__(256) void k_grid_inflate(const uint32_t *__restrict__ src, uint32_t *__restrict__ dst, const GridInflateArgs a) {
    extern __shared__ uint32_t s_tile[];
    const int r = a.r;
    const int lw = kGridTileW + 2, ly = kGridTileY + 2 * r, lz = kGridTileZ + 2 * r;
    const int tiles_x = (a.g.wx + kGridTileW - 1) / kGridTileW, tiles_y = (a.g.ny + kGridTileY - 1) / kGridTileY;
    const int bx = blockIdx.x % tiles_x, by = blockIdx.x / tiles_x % tiles_y, bz = blockIdx.x / tiles_x / tiles_y;
    const int w0 = bx * kGridTileW - 1, y0 = by * kGridTileY - r, z0 = bz * kGridTileZ - r;
    const uint32_t last_mask = (a.g.nx & 31) ? (1u << (a.g.nx & 31)) - 1u : 0xffffffffu;
    for (int i = threadIdx.x; i < lw * ly * lz; i += 256) {
        const int w = w0 + i % lw, y = y0 + i / lw % ly, z = z0 + i / lw / ly;
        uint32_t v = 0;
        if (w >= 0 && w < a.g.wx && y >= 0 && y < a.g.ny && z >= 0 && z < a.g.nz) {
            v = src[((int64_t)z * a.g.ny + y) * a.g.wx + w];
            if (w == a.g.wx - 1) v &= last_mask;
        }
        s_tile[i] = v;
    }
    __syncthreads();
    const int tw = threadIdx.x % kGridTileW, ty = threadIdx.x / kGridTileW % kGridTileY, tz = threadIdx.x / kGridTileW / kGridTileY;
    const int w = bx * kGridTileW + tw, y = by * kGridTileY + ty, z = bz * kGridTileZ + tz;
    if (w >= a.g.wx || y >= a.g.ny || z >= a.g.nz) return;
    uint32_t out = 0;
    for (int dz = -r; dz <= r; dz++)
        for (int dy = -r; dy <= r; dy++) {
            const int d2 = dy * dy + dz * dz;
            if (d2 > r * r) continue;
            const int k = a.width[d2];
            const uint32_t *row = s_tile + ((tz + r + dz) * ly + (ty + r + dy)) * lw + tw; // row[0] = the word below, [1] = this, [2] = above
            const unsigned long long below = ((unsigned long long)row[1] << 32) | row[0], above = ((unsigned long long)row[2] << 32) | row[1];
            out |= (uint32_t)(grid_smear_up(below, k) >> 32) | (uint32_t)grid_smear_down(above, k);
        }
    if (w == a.g.wx - 1) out &= last_mask;
    dst[((int64_t)z * a.g.ny + y) * a.g.wx + w] = out;
}

// ---- the cell list: 256 words per workgroup
__global__ __launch_bounds__(256) void k_grid_cell_count(const uint32_t *__restrict__ bits, int64_t n_words, int32_t *__restrict__ tile_cnt) {
    __shared__ int s_cnt[4];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile * 256 < n_words; tile += gridDim.x) {
        const int64_t i = tile * 256 + threadIdx.x;
        const int c = wave_sum(i < n_words ? __popc(bits[i]) : 0);
        if (lane == 0) s_cnt[wv] = c;
        __syncthreads();
        if (threadIdx.x == 0) tile_cnt[tile] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        __syncthreads();
    }
}

// tile_off: the exclusive prefix of the counts.  Linear indices (z ny + y) nx + x ascending, none at or beyond cap.
__global__ __launch_bounds__(256) void k_grid_cell_scatter(const uint32_t *__restrict__ bits, int64_t n_words, int nx, int wx,
                                                           const int32_t *__restrict__ tile_off, int32_t *__restrict__ cells, int cap) {
    __shared__ int s_cnt[4];
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile * 256 < n_words; tile += gridDim.x) {
        const int64_t i = tile * 256 + threadIdx.x;
        uint32_t v = i < n_words ? bits[i] : 0u;
        const int c = __popc(v);
        int incl = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_cnt[wv] = incl;
        __syncthreads();
        int at = tile_off[tile] + (incl - c);
        for (int k = 0; k < wv; k++) at += s_cnt[k];
        const int64_t row = i / wx;
        const int32_t first = (int32_t)(row * nx + (i % wx) * 32);
        while (v && at < cap) {
            cells[at++] = first + (__ffs((int)v) - 1);
            v &= v - 1;
        }
        __syncthreads();
    }
}

// *cells_total = the set bits of bits[0, n_words) (rows of wx words, nx voxels); with `cells`, their linear indices ascending, none
// at or beyond cells_cap.  cell_tiles: d.cell_tiles() ints of scratch (<= 2^20: at most 2^28 words)
inline void launch_cell_list(const uint32_t *bits, const GridDims &d, int32_t *cell_tiles, int32_t *cells_total, int32_t *cells, int cells_cap,
                             hipStream_t st) {
    const int64_t n_words = d.n_words(), tiles = d.cell_tiles();
    const int blocks = launch_blocks(n_words, 256, 8192);
    hipLaunchKernelGGL(k_grid_cell_count, dim3(blocks), dim3(256), 0, st, bits, n_words, cell_tiles);
    hipLaunchKernelGGL(k_cloud_scan, dim3(1), dim3(1024), 0, st, cell_tiles, (int)tiles, cells_total);
    if (cells && cells_cap > 0)
        hipLaunchKernelGGL(k_grid_cell_scatter, dim3(blocks), dim3(256), 0, st, bits, n_words, d.nx, d.wx, (const int32_t *)cell_tiles, cells, cells_cap);
}

hipError_t launch_grid_inflate(const uint32_t *src, uint32_t *dst, const GridDims &d, int r, hipStream_t st) {
    GridInflateArgs a;
    a.g = d;
    a.r = r;
    for (int s = 0; s <= kGridMaxInflate * kGridMaxInflate; s++) a.width[s] = (uint8_t)(s <= r * r ? grid_inflate_width(r, s) : 0);
    const int64_t tiles = (int64_t)((d.wx + kGridTileW - 1) / kGridTileW) * ((d.ny + kGridTileY - 1) / kGridTileY) * ((d.nz + kGridTileZ - 1) / kGridTileZ);
    if (tiles > INT32_MAX) return hipErrorInvalidValue; // (never: at most 2^28 voxels, a tile holds at least one)
    const size_t lds = (size_t)(kGridTileW + 2) * (kGridTileY + 2 * r) * (kGridTileZ + 2 * r) * sizeof(uint32_t); // <= 57600 bytes at r = 16
    hipLaunchKernelGGL(k_grid_inflate, dim3((unsigned)tiles), dim3(256), lds, st, src, dst, a);
    return hipGetLastError();
}

// the clear, then the lists, then the planes derived from them: launched in this order on one stream
hipError_t launch_grid(const dsm_surfel *store, const RunTable &rt, const MapPart &mp, const GridSpec &g, int inflate, const GridScratch &sc,
                       const GridOut &out, hipStream_t st) {
    const GridDims d = grid_dims(g.n[0], g.n[1], g.n[2]);
    {
        const int64_t n = out.index ? d.n_vox() : d.n_words(); // <= 2^28 each
        hipLaunchKernelGGL(k_grid_clear, dim3(launch_blocks(n, 256, 8192)), dim3(256), 0, st, out.index ? (uint32_t *)out.index : out.occupied, n,
                           out.index ? 0xffffffffu : 0u, sc.counts);
    }
    GridSetupArgs a;
    a.g = g;
    a.n_seq = sc.n_seq;
    if (rt.n_seg > 0 && rt.total > 0) hipLaunchKernelGGL(k_grid_setup_run, dim3(run_blocks(rt.total)), dim3(256), 0, st, store, rt, a, sc.splats, sc.counts);
    const hipError_t e = launch_map_offsets(mp, st);
    if (e != hipSuccess) return e;
    if (map_tiles(mp) > 0) hipLaunchKernelGGL(k_grid_setup_map, dim3(map_tiles(mp)), dim3(256), 0, st, mp, rt.total, a, sc.splats, sc.counts);
    GridTarget t;
    t.g = g;
    t.wx = d.wx;
    t.index = (uint32_t *)out.index;
    t.bits = out.occupied;
    if (sc.n_seq > 0) {
        int blocks = launch_blocks(sc.n_seq, 16, 16384);
        hipLaunchKernelGGL(k_grid_splat, dim3(blocks), dim3(256), 0, st, (const GridSplat *)sc.splats, (const int32_t *)sc.counts, sc.n_seq, t);
        blocks = sc.n_seq < 2048 ? sc.n_seq : 2048;
        hipLaunchKernelGGL(k_grid_splat_big, dim3(blocks), dim3(256), 0, st, (const GridSplat *)sc.splats, (const int32_t *)sc.counts, sc.n_seq, t);
    }
    if (out.index) {
        hipLaunchKernelGGL(k_grid_bits, dim3(launch_blocks(d.units64(), 4, 8192)), dim3(256), 0, st, (const uint32_t *)out.index, out.occupied, d.nx, d.wx,
                           d.rows());
    }
    if (out.inflated) {
        const hipError_t e = launch_grid_inflate(out.occupied, out.inflated, d, inflate, st);
        if (e != hipSuccess) return e;
    }
    if (out.cells_total)
        launch_cell_list(out.cells_of_inflated ? out.inflated : out.occupied, d, sc.cell_tiles, out.cells_total, out.cells, out.cells_cap, st);
    return hipGetLastError();
}

} // namespace dsm
