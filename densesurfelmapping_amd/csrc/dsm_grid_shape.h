// dsm_grid_shape.h -- the vocabulary the voxel-grid calls share: the shape of a grid and of its bit sets, the limit on its
// dimensions, the layout of a call's scratch, the cap on a list and the cap on a launch.  Plain C++ with no HIP include, so that
// the C API, the node, the launchers and a host program (tests/grid_shape_host.cpp) all hold the same text; GridDims also
// travels into the kernels inside their argument structs.
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define DSM_SHAPE_HD __host__ __device__
#else
#define DSM_SHAPE_HD
#endif

namespace dsm {

constexpr int64_t kGridMaxVoxels = (int64_t)1 << 28;  // of a grid
constexpr int64_t kFieldMaxVoxels = (int64_t)1 << 26; // of a grid with a distance field or with components
constexpr int kGridMaxInflate = 16;                   // the largest inflation radius, in voxels

// A grid of nx x ny x nz voxels, x fastest.  A bit set of it has wx words a row, bit x & 31 of word x >> 5, [nz][ny][wx]; the
// bits of a row's last word at and beyond nx are padding.  Sixteen bytes, four ints: kernels take it by value.
struct GridDims {
    int nx, ny, nz, wx;
    DSM_SHAPE_HD int64_t rows() const { return (int64_t)ny * nz; }
    DSM_SHAPE_HD int64_t n_vox() const { return rows() * nx; }
    DSM_SHAPE_HD int64_t n_words() const { return rows() * wx; }
    DSM_SHAPE_HD size_t set_bytes() const { return (size_t)n_words() * sizeof(uint32_t); }
    DSM_SHAPE_HD int64_t cell_tiles() const { return (n_words() + 255) / 256; } // the tiles of the cell list's scan (launch_cell_list)
    DSM_SHAPE_HD int64_t units64() const { return rows() * ((nx + 63) / 64); }  // the 64-voxel pieces of all rows: a wave each
    DSM_SHAPE_HD uint32_t last_mask() const { return (nx & 31) ? (1u << (nx & 31)) - 1u : 0xffffffffu; } // the valid bits of a row's last word
};
static_assert(sizeof(GridDims) == 16, "GridDims is four ints");

DSM_SHAPE_HD inline GridDims grid_dims(int nx, int ny, int nz) { return GridDims{nx, ny, nz, (nx + 31) / 32}; }

// a dimension < 1 or more than `limit` voxels: false.  Nothing of a GridDims is meaningful before this has said true.
DSM_SHAPE_HD inline bool grid_dims_ok(int32_t nx, int32_t ny, int32_t nz, int64_t limit = kGridMaxVoxels) {
    if (nx < 1 || ny < 1 || nz < 1) return false;
    const int64_t xy = (int64_t)nx * ny; // < 2^62
    return xy <= limit && xy * nz <= limit;
}

// The scratch of a call, part by part: take(here, bytes) is where the part lies, and the parts behind it lie `bytes` rounded up
// to `pad` further on if the part is `here`, else where it would have lain.  pad: 16 or 256.
class ScratchPlan {
public:
    explicit ScratchPlan(size_t pad) : pad_(pad) {}
    size_t take(bool here, size_t bytes) {
        const size_t at = bytes_;
        if (here) bytes_ += (bytes + pad_ - 1) & ~(pad_ - 1);
        return at;
    }
    size_t bytes() const { return bytes_; } // of all parts taken so far
private:
    size_t pad_, bytes_ = 0;
};

// no more than n: the room of a list of cells or components that cannot hold more entries than the grid has voxels, and the
// entries of such a list that come back when `cap` were counted and there is room for n
inline size_t capped(int64_t cap, int64_t n) { return (size_t)(cap < n ? cap : n); }

// the grid of a grid-stride kernel over n items, per_block to a workgroup, no more than cap workgroups
inline int launch_blocks(int64_t n, int per_block, int cap) {
    const int64_t blocks = (n + per_block - 1) / per_block;
    return (int)(blocks < cap ? blocks : cap);
}

} // namespace dsm
