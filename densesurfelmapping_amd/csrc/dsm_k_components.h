// dsm_k_components.h -- connected components of a bit set in the grid layout (dsm_grid_components; the definition is in
// dsm_components.h).  Included by dsm_kernels.hip.
//
//   k_comp_init     per voxel: label = the first voxel of its run of set bits inside its 32-bit word, -1 for a voxel not in the set
//   k_comp_merge    per word: unions the runs with the runs before them in index order -- the word to the left, and the rows
//                   (y - 1, z), (y, z - 1) for faces, (y - 1 .. y + 1, z - 1) and the x +- 1 diagonals on top for all 26
//   k_comp_flatten  per voxel: label = the root of its tree = the lowest index of its component
//   k_comp_count    per word: voxels per root into the work plane (integer atomicAdd), the root bit plane
//   k_comp_keep     per word: the bit plane of the roots with count >= min_count
//   k_grid_cell_count / k_cloud_scan on both bit planes: n_all, n_components, the tile offsets of the kept roots
//   k_comp_rank     per word: the table entry of every kept root initialised in ascending order; the work plane then holds the
//                   entry's index at a kept root and -1 at every other root
//   k_comp_stats    per word: sums and bounding boxes by 64-bit add, min and max
// A fixed sequence of launches on one stream.  The label plane IS the parent plane of a union-find forest in which a parent is
// always a lower index than its child (or the voxel itself, a root): a path is a chain of strictly decreasing indices, so every
// find ends after at most as many steps as its start index and no cycle can form, whatever other workgroups do meanwhile.  No
// kernel waits for another workgroup: there is no flag, no barrier across workgroups and no cooperative launch.
//
// Tiles: the only unit that is labelled without merging is the run inside one word (kCompTileX voxels of one row); every word
// boundary along x and every row and slice boundary (kCompTileY = kCompTileZ = 1) is a seam that k_comp_merge closes.  A
// workgroup of the word passes takes kCompBlockWords consecutive words.
//
// Pad bits of the source are masked wherever a word is read (comp_word; k_comp_init looks at bits below its own only).  The
// per-voxel passes run along x; the word passes read the label of the first voxel of a run, along x as well.
#pragma once
#include "dsm_components.h"
#include "dsm_k_grid.h"

namespace dsm {

constexpr int kCompTileX = 32;       // voxels along x labelled without a merge: one word
constexpr int kCompTileY = 1;        // rows
constexpr int kCompTileZ = 1;        // slices
constexpr int kCompBlockWords = 256; // words per workgroup trip of the word passes: the tile of k_grid_cell_count

struct CompArgs {
    GridDims g;
    uint32_t last_mask; // the valid bits of the last word of a row
};
static_assert(sizeof(CompArgs) == 20 && offsetof(CompArgs, last_mask) == 16, "as the kernels were built for");

// word w of row (y, z), inside the grid; the pad bits 0
__device__ __forceinline__ uint32_t comp_word(const uint32_t *__restrict__ src, int w, int y, int z, const CompArgs &a) {
    const uint32_t v = src[((int64_t)z * a.g.ny + y) * a.g.wx + w];
    return w == a.g.wx - 1 ? v & a.last_mask : v;
}

// The parent plane is read with relaxed device-scope loads.  A value that is out of date is an EARLIER parent of the same voxel:
// a member of the same component that is no lower than the present parent, so a find that follows it still walks down inside the
// component and the union below corrects itself (its atomicMin returns the present value).
__device__ __forceinline__ int32_t comp_parent(const int32_t *label, int32_t v) {
    return __hip_atomic_load(label + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of v's tree as far as this thread can see.  Terminates: every step goes to a strictly lower index.
__device__ __forceinline__ int32_t comp_find(const int32_t *label, int32_t v) {
    for (;;) {
        const int32_t p = comp_parent(label, v);
        if (p == v) return v;
        v = p;
    }
}

// Union by minimum index.  a and b are set voxels of one component-to-be.  Both are taken to their roots; the larger root hangs
// itself below the smaller with atomicMin.  If the atomicMin finds that the larger root had been given a parent `old` meanwhile,
// parent(a) is now min(old, b) and what remains to be joined is the pair (old, b).  Terminates: every retry replaces a, the larger
// operand, by old < a, while a find can only lower an operand; the pair (max, min) decreases strictly in lexicographic order and
// both are >= 0.  The starting voxels are then pointed at the root found (atomicMin keeps the parent < child rule), which keeps
// the chains short for the finds that follow.
__device__ __forceinline__ void comp_union(int32_t *label, int32_t a0, int32_t b0) {
    int32_t a = a0, b = b0;
    for (;;) {
        a = comp_find(label, a);
        b = comp_find(label, b);
        if (a == b) break;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicMin(label + a, b);
        if (old == a) { a = b; break; } // a was a root and hangs below b now
        a = old;
    }
    // a == b: the lowest index this union has seen, an ancestor-to-be of both starts
    if (a < a0) atomicMin(label + a0, a);
    if (a < b0) atomicMin(label + b0, a);
}

__global__ __launch_bounds__(256) void k_comp_init(const uint32_t *__restrict__ src, int32_t *__restrict__ label, const CompArgs a) {
    const int64_t n_vox = (int64_t)a.g.nx * a.g.ny * a.g.nz;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_vox; i += (int64_t)gridDim.x * 256) {
        const int64_t row = i / a.g.nx;
        const int x = (int)(i - row * a.g.nx), b = x & 31;
        const uint32_t word = src[row * a.g.wx + (x >> 5)];
        int32_t l = -1;
        if ((word >> b) & 1u) {
            const uint32_t gaps_below = ~word & ((1u << b) - 1u); // the clear bits below mine: none of them a pad bit
            const int start = gaps_below ? 32 - __clz((int)gaps_below) : 0;
            l = (int32_t)i - b + start;
        }
        label[i] = l;
    }
}

// the first set bit of m and the length of the run of set bits that starts there; m != 0
__device__ __forceinline__ void comp_first_run(uint32_t m, int &start, int &len) {
    start = __ffs((int)m) - 1;
    const uint32_t rest = ~(m >> start); // 0: all 32 bits are set (start is 0 then)
    len = rest ? __ffs((int)rest) - 1 : 32;
}
__device__ __forceinline__ uint32_t comp_run_mask(int start, int len) { return (len >= 32 ? 0xffffffffu : (1u << len) - 1u) << start; }

// unions voxel base + b with voxel base + b + off for the first bit b of every run of m
__device__ __forceinline__ void comp_union_runs(int32_t *label, uint32_t m, int32_t base, int32_t off) {
    uint32_t starts = m & ~(m << 1);
    while (starts) {
        const int b = __ffs((int)starts) - 1;
        starts &= starts - 1;
        comp_union(label, base + b, base + b + off);
    }
}

template <int CONN>
__global__ __launch_bounds__(256) void k_comp_merge(const uint32_t *__restrict__ src, int32_t *label, const CompArgs a) {
    const int64_t n_words = (int64_t)a.g.wx * a.g.ny * a.g.nz;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * 256) {
        const int w = (int)(i % a.g.wx);
        const int64_t row = i / a.g.wx;
        const int y = (int)(row % a.g.ny), z = (int)(row / a.g.ny);
        const uint32_t mine = comp_word(src, w, y, z, a);
        if (!mine) continue;
        const int32_t base = (int32_t)(row * a.g.nx + w * 32);
        // the run that continues from the word to the left (never the last word of a row: no pad bits there)
        if ((mine & 1u) && w > 0 && (src[i - 1] >> 31)) comp_union(label, base, base - 1);
#pragma unroll
        for (int dz = -1; dz <= 0; dz++)
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
                if (dz == 0 && dy >= 0) continue; // the rows before this one in index order
                constexpr int conn = CONN;
                const bool straight = comp_adjacent(0, dy, dz, conn), diagonal = comp_adjacent(1, dy, dz, conn);
                if (!straight && !diagonal) continue;
                const int yy = y + dy, zz = z + dz;
                if (yy < 0 || yy >= a.g.ny || zz < 0) continue;
                const uint32_t n = comp_word(src, w, yy, zz, a);
                const int32_t off = (int32_t)(((int64_t)dz * a.g.ny + dy) * a.g.nx);
                if (straight) comp_union_runs(label, mine & n, base, off);
                if (diagonal) {
                    // bit b of `left` / `right`: the voxel at x - 1 / x + 1 of the other row.  Where the voxel at x of that row is
                    // set as well it has joined both already (it is in the neighbour's run): those bits are left out.
                    const uint32_t lo = w > 0 ? comp_word(src, w - 1, yy, zz, a) >> 31 : 0u;
                    const uint32_t hi = w + 1 < a.g.wx ? comp_word(src, w + 1, yy, zz, a) & 1u : 0u;
                    const uint32_t left = (n << 1) | lo, right = (n >> 1) | (hi << 31);
                    comp_union_runs(label, mine & left & ~n, base, off - 1);
                    comp_union_runs(label, mine & right & ~n, base, off + 1);
                }
            }
    }
}

__global__ __launch_bounds__(256) void k_comp_flatten(int32_t *label, int64_t n_vox) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_vox; i += (int64_t)gridDim.x * 256) {
        const int32_t l = comp_parent(label, (int32_t)i);
        // (a concurrent store of a root over a parent keeps the chain inside the component and decreasing)
        if (l >= 0 && l != (int32_t)i) label[i] = comp_find(label, l);
    }
}

// all 64 lanes: the sum over the lanes with `in`
__device__ __forceinline__ int64_t comp_wave_sum64(int64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ int comp_wave_min(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ int comp_wave_max(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

// per word: the voxels of every run are added to the count of the run's root.  Runs of one word that share a root are added up in
// the thread, and the lanes of a wave that end with the root of the wave's first such lane share one atomic.
__global__ __launch_bounds__(256) void k_comp_count(const uint32_t *__restrict__ src, const int32_t *__restrict__ label, int32_t *__restrict__ count,
                                                    uint32_t *__restrict__ root_bits, const CompArgs a) {
    const int64_t n_words = (int64_t)a.g.wx * a.g.ny * a.g.nz;
    const int lane = lane_id();
    for (int64_t tile = blockIdx.x; tile * kCompBlockWords < n_words; tile += gridDim.x) {
        const int64_t i = tile * kCompBlockWords + threadIdx.x;
        int32_t r = -1, n = 0;
        if (i < n_words) {
            const int w = (int)(i % a.g.wx);
            const int64_t row = i / a.g.wx;
            uint32_t m = src[i];
            if (w == a.g.wx - 1) m &= a.last_mask;
            const int32_t base = (int32_t)(row * a.g.nx + w * 32);
            uint32_t roots = 0u;
            while (m) {
                int s, len;
                comp_first_run(m, s, len);
                m &= ~comp_run_mask(s, len);
                const int32_t root = label[base + s];
                if (root == base + s) roots |= 1u << s;
                if (root != r && n) { atomicAdd(count + r, n); n = 0; }
                r = root;
                n += len;
            }
            root_bits[i] = roots;
        }
        const unsigned long long have = __ballot(n > 0);
        if (have) {
            const int32_t r0 = __shfl(r, __ffsll((long long)have) - 1, 64);
            const bool shared = n > 0 && r == r0;
            const int total = wave_sum(shared ? n : 0);
            if (shared ? lane == __ffsll((long long)have) - 1 : n > 0) atomicAdd(count + r, shared ? total : n);
        }
    }
}

__global__ __launch_bounds__(256) void k_comp_keep(const uint32_t *__restrict__ root_bits, const int32_t *__restrict__ count, uint32_t *__restrict__ keep_bits,
                                                   int min_count, const CompArgs a) {
    const int64_t n_words = (int64_t)a.g.wx * a.g.ny * a.g.nz;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_words; i += (int64_t)gridDim.x * 256) {
        const int32_t base = (int32_t)((i / a.g.wx) * a.g.nx + (i % a.g.wx) * 32);
        uint32_t v = root_bits[i], keep = 0u;
        while (v) {
            const int b = __ffs((int)v) - 1;
            v &= v - 1;
            if (count[base + b] >= min_count) keep |= 1u << b;
        }
        keep_bits[i] = keep;
    }
}

// tile_off: the exclusive prefix of the kept roots per kCompBlockWords words (k_grid_cell_count, k_cloud_scan).  The entry of
// kept root number k < cap is initialised; work[root] = k for those, -1 for every other root.
__global__ __launch_bounds__(256) void k_comp_rank(const uint32_t *__restrict__ root_bits, const uint32_t *__restrict__ keep_bits,
                                                   const int32_t *__restrict__ tile_off, int32_t *__restrict__ work, const int32_t *__restrict__ tag_src,
                                                   dsm_component *__restrict__ table, int cap, const CompArgs a) {
    __shared__ int s_cnt[4];
    const int64_t n_words = (int64_t)a.g.wx * a.g.ny * a.g.nz;
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    for (int64_t tile = blockIdx.x; tile * kCompBlockWords < n_words; tile += gridDim.x) {
        const int64_t i = tile * kCompBlockWords + threadIdx.x;
        uint32_t roots = i < n_words ? root_bits[i] : 0u;
        const uint32_t keep = i < n_words ? keep_bits[i] : 0u;
        const int c = __popc(keep);
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
        const int32_t base = i < n_words ? (int32_t)((i / a.g.wx) * a.g.nx + (i % a.g.wx) * 32) : 0;
        while (roots) {
            const int b = __ffs((int)roots) - 1;
            roots &= roots - 1;
            const int32_t lin = base + b;
            int32_t k = -1;
            if ((keep >> b) & 1u) {
                if (at < cap) {
                    k = at;
                    dsm_component e;
                    comp_init(e, lin, tag_src ? tag_src[lin] : 0);
                    e.count = work[lin];
                    table[k] = e;
                }
                at++;
            }
            work[lin] = k;
        }
        __syncthreads();
    }
}

struct CompPart { // what one thread has gathered for table entry k
    int32_t k;
    int64_t sum[3];
    int32_t lo[3], hi[3];
};
__device__ __forceinline__ void comp_part_flush(dsm_component *table, const CompPart &p) {
    dsm_component *e = table + p.k;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        atomicAdd((unsigned long long *)&e->sum[c], (unsigned long long)p.sum[c]);
        atomicMin(&e->lo[c], p.lo[c]);
        atomicMax(&e->hi[c], p.hi[c]);
    }
}

// per word, after k_comp_rank: the runs of the kept components into their table entries.  The same sharing as k_comp_count.
__global__ __launch_bounds__(256) void k_comp_stats(const uint32_t *__restrict__ src, const int32_t *__restrict__ label, const int32_t *__restrict__ work,
                                                    dsm_component *table, const CompArgs a) {
    const int64_t n_words = (int64_t)a.g.wx * a.g.ny * a.g.nz;
    const int lane = lane_id();
    for (int64_t tile = blockIdx.x; tile * kCompBlockWords < n_words; tile += gridDim.x) {
        const int64_t i = tile * kCompBlockWords + threadIdx.x;
        CompPart p;
        p.k = -1;
        if (i < n_words) {
            const int w = (int)(i % a.g.wx);
            const int64_t row = i / a.g.wx;
            const int y = (int)(row % a.g.ny), z = (int)(row / a.g.ny);
            uint32_t m = src[i];
            if (w == a.g.wx - 1) m &= a.last_mask;
            const int32_t base = (int32_t)(row * a.g.nx + w * 32);
            while (m) {
                int s, len;
                comp_first_run(m, s, len);
                m &= ~comp_run_mask(s, len);
                const int32_t k = work[label[base + s]];
                if (k < 0) continue;
                if (k != p.k) {
                    if (p.k >= 0) comp_part_flush(table, p);
                    p.k = k;
                    for (int c = 0; c < 3; c++) { p.sum[c] = 0; p.lo[c] = INT32_MAX; p.hi[c] = -1; }
                }
                const int x0 = w * 32 + s, x1 = x0 + len - 1;
                p.sum[0] += ((int64_t)(x0 + x1) * len) / 2; // x0 + .. + x1
                p.sum[1] += (int64_t)y * len;
                p.sum[2] += (int64_t)z * len;
                p.lo[0] = min(p.lo[0], x0); p.hi[0] = max(p.hi[0], x1);
                p.lo[1] = min(p.lo[1], y); p.hi[1] = max(p.hi[1], y);
                p.lo[2] = min(p.lo[2], z); p.hi[2] = max(p.hi[2], z);
            }
        }
        const unsigned long long have = __ballot(p.k >= 0);
        if (!have) continue;
        const int first = __ffsll((long long)have) - 1;
        const int32_t k0 = __shfl(p.k, first, 64);
        const bool shared = p.k >= 0 && p.k == k0;
        if (__popcll(__ballot(shared)) > 1) {
            CompPart t;
            t.k = k0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                t.sum[c] = comp_wave_sum64(shared ? p.sum[c] : 0);
                t.lo[c] = comp_wave_min(shared ? p.lo[c] : INT32_MAX);
                t.hi[c] = comp_wave_max(shared ? p.hi[c] : -1);
            }
            if (lane == first) comp_part_flush(table, t);
            if (p.k >= 0 && !shared) comp_part_flush(table, p);
        } else if (p.k >= 0) {
            comp_part_flush(table, p);
        }
    }
}

// label: [voxels] (the caller's plane or scratch), work: [voxels], root_bits / keep_bits: [words], root_tiles / keep_tiles:
// d.cell_tiles() ints each; *n_all / *n_kept: the counts.  table may be null (cap 0): no statistics are taken.
hipError_t launch_components(const uint32_t *src, const int32_t *tag_src, const GridDims &d, int connectivity, int min_count, int32_t *label,
                             int32_t *work, uint32_t *root_bits, uint32_t *keep_bits, int32_t *root_tiles, int32_t *keep_tiles, dsm_component *table,
                             int cap, int32_t *n_all, int32_t *n_kept, hipStream_t st) {
    const CompArgs a = {d, d.last_mask()};
    const int64_t n_vox = d.n_vox(); // <= 2^26, as the words
    const int vox_blocks = launch_blocks(n_vox, 256, 16384), word_blocks = launch_blocks(d.n_words(), 256, 8192);
    const hipError_t e0 = hipMemsetAsync(work, 0, (size_t)n_vox * sizeof(int32_t), st);
    if (e0 != hipSuccess) return e0;
    hipLaunchKernelGGL(k_comp_init, dim3(vox_blocks), dim3(256), 0, st, src, label, a);
    if (connectivity == kConnectFaces) hipLaunchKernelGGL(k_comp_merge<kConnectFaces>, dim3(word_blocks), dim3(256), 0, st, src, label, a);
    else hipLaunchKernelGGL(k_comp_merge<kConnectAll>, dim3(word_blocks), dim3(256), 0, st, src, label, a);
    hipLaunchKernelGGL(k_comp_flatten, dim3(vox_blocks), dim3(256), 0, st, label, n_vox);
    hipLaunchKernelGGL(k_comp_count, dim3(word_blocks), dim3(256), 0, st, src, (const int32_t *)label, work, root_bits, a);
    hipLaunchKernelGGL(k_comp_keep, dim3(word_blocks), dim3(256), 0, st, (const uint32_t *)root_bits, (const int32_t *)work, keep_bits, min_count, a);
    // the counts alone, no list: the tiles of the cell list are k_comp_rank's (kCompBlockWords)
    launch_cell_list(root_bits, d, root_tiles, n_all, nullptr, 0, st);
    launch_cell_list(keep_bits, d, keep_tiles, n_kept, nullptr, 0, st);
    if (table && cap > 0) {
        hipLaunchKernelGGL(k_comp_rank, dim3(word_blocks), dim3(256), 0, st, (const uint32_t *)root_bits, (const uint32_t *)keep_bits,
                           (const int32_t *)keep_tiles, work, tag_src, table, cap, a);
        hipLaunchKernelGGL(k_comp_stats, dim3(word_blocks), dim3(256), 0, st, src, (const int32_t *)label, (const int32_t *)work, table, a);
    }
    return hipGetLastError();
}

} // namespace dsm
