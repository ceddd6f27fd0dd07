// dsm_device.h -- device-resident state of one handle, shared by dsm_kernels.hip and dsm_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dsm.h"
#include "dsm_grid_shape.h"
#include "dsm_math.h"

namespace dsm {

// per-wave phase stamps of the per-seed kernels (dsm_debug_wave_stamps): compiled in only by -DDSM_WAVE_STAMPS=1
#ifndef DSM_WAVE_STAMPS
#define DSM_WAVE_STAMPS 0
#endif
constexpr bool kWaveStamps = DSM_WAVE_STAMPS != 0;

constexpr int kIntMax = 0x7fffffff;
typedef uint16_t label_t;             // a pixel's superpixel index in the label planes
constexpr int kNoLabel = 0xffff;      // the reference's label -1 (pixels no cell reaches) in a label plane
constexpr int kMaxSeeds = 0xffff;     // superpixels a frame can have (dsm_create checks): every index fits a label_t below kNoLabel

// Per-frame inputs that change from frame to frame.  A ring of these lives in HBM; kernels pick
// entry (cursor % ring) so a captured hipGraph can be replayed without touching its arguments.
struct FrameParams {
    float pose[16]; // cam -> world, column-major
    float inv[16];  // world -> cam (host-computed with inverse4<float>, FF.cpp:59)
    int32_t ref_idx;
    int32_t slot;
    int32_t pad[2];
};

// The frame being processed: written to device memory by k_init_seeds (first kernel of a frame) from
// params[cursor % n_params], read by every later kernel of the frame.
struct FrameCur {
    FrameParams p;
    const uint8_t *img;
    const float *dep;
};

// Hand-off from k_seed_stats to k_seed_fit: the start of get_huber_norm (FF.cpp:104-120) for one seed; the fit gathers the
// centred inlier points itself.  A superpixel's pixels lie within 8 of its centre in both axes (FF.cpp:413-422): at most
// 15 x 15 = 225 members.
struct GnHeader {
    int32_t m_in;      // inliers handed to the fit; 0 = no fit, the seed keeps its defaults (FF.cpp:841, 862)
    float nx, ny, nz;  // normalised sum of the inliers' pixel normals (FF.cpp:852-871)
    float mx, my, mz;  // centroid (FF.cpp:111-120)
    float far2;        // squared superpixel radius (FF.cpp:820-824)
};
constexpr int kGnCap = 232;
constexpr int kRestListCap = 127; // = kLaneCap of k_update_seeds: rows of a queued list; a lane keeps 123 depths in LDS, the rows up to 127 are spare (a list of 124 or more gets a wave of its own)
constexpr int kFitSmallCap = 120; // longest list the short-column tier of k_seed_fit takes (batched launches)

// Everything a kernel needs.  Passed to every kernel BY VALUE (kernel-argument segment): the pointers and
// sizes never change after dsm_create, so a captured graph stays valid, and a kernel reaches its data
// without first loading a context from memory (one dependent round trip less per kernel).
struct DeviceCtx {
    // geometry
    int32_t w, h, pitch; // pitch = row stride in elements of every image-shaped plane (multiple of 64)
    int32_t gw, gh, n_seed;
    uint32_t gw_magic; // floor(2^32 / gw) + 1: s / gw == mulhi(s, gw_magic) for every seed index s < 65 536 (seed_cell)
    Intrinsics k;
    float far_d, near_d;
    double huber, baseline, disp_err, min_tol;
    const float *ray_x, *ray_y; // [w + 1], [h + 1]: (x - cx) / fx, (y - cy) / fy of back_project (dsm_math.h, ray_coeff)
    // frame slots (HBM-resident inputs)
    const uint8_t *img_base;
    const float *depth_base;
    int64_t slot_elems; // pitch * h
    int32_t n_slots;
    // superpixel state
    // 16 bits per pixel (label_t: a frame has at most kMaxSeeds = 65 535 superpixels, kNoLabel = the reference's -1): the label
    // image is read by every stage of a frame, by the window walks several times over -- a third of a frame's memory-side
    // traffic when it was 4 bytes per pixel
    label_t *label; // [h][pitch] superpixel index of every pixel: every sweep's image in turn (k_assign and k_resolve work in place), then the final one
    label_t *cand;  // [h][pitch] seed picked by this sweep, at the pixels on `worklist` only (whose old seed was stable at sweep start)
    float4 *core;   // [S] x, y, mean_intensity, mean_depth  (live seed state during the sweeps)
    double *inv_depth; // [S] 1.0 / mean_depth, FF.cpp:380
    float4 *core_stage; // [S] update_seeds output before the chunk-commit rule
    int32_t *stable_stage;
    // tmin[s]: -1 = seed unstable when the sweep started; INT_MAX = stable and never picked;
    // otherwise the first pixel key (row-major) at which an evaluated pixel picked the seed.
    int32_t *tmin;
    int32_t *first_empty; // [kSweeps][kWorkers] first unstable seed without pixels, per worker chunk
    int32_t *worklist;    // pixel keys whose old seed was stable at sweep start and which picked another one
    int32_t *work_count;
    int32_t fit_small_cap;  // kFitSmallCap, or less (dsm_debug_set_fit_small_cap: lets a test push ordinary groups through the other tier)
    int32_t *fit_big_count; // groups of seeds queued in `worklist` for the full-length tier of k_seed_fit (batched launches)
    int32_t *rest_count;    // [kSweeps][2] entries k_update_seeds queued in `worklist` for k_update_seeds_rest (batched launches):
                            // seeds that need more Huber passes | seeds whose depth list outgrew its LDS row
    float *rest_list;       // [ceil(S / 64)][kRestListCap][64] depth lists of the queued seeds, entry-major within a group of 64
    GnHeader *gn_hdr; // [S]
    // [ceil(S / 64)][16][64] which pixels of window row r are depth inliers of seed 64 g + l (bit j = window column j, window_pixel
    // of dsm_math.h): inl_mask[g][r][l], group-major so that a wave of k_seed_stats stores 128 contiguous bytes per row.  Written by
    // k_seed_stats for every seed of the frame, read by the k_seed_fit that follows it (sixteen lanes per seed, one row each) instead
    // of the labels.  Rows of seed s are valid iff gn_hdr[s].m_in > 0: a seed without a plane keeps whatever an earlier frame or its
    // own rejected walk left.  k_seed_points does not write it; the fit behind it derives its inliers itself.
    uint16_t *inl_mask;
    float4 *plane;    // [S] the plane k_seed_fit fitted (normal, offset: before plane_finish), for k_seed_finish
    float *normals;   // [h][pitch][3] forward-difference normal of every depth inlier of its own superpixel (k_pixel_normals); other entries stale, never read
    dsm_seed *seeds; // [S] final seed table, reference layout
    // what initialize_surfels (FF.cpp:315-361) would create from each seed, prepared by k_seed_planes (every
    // input but the `fused` flag is known there): the surfel, whether the seed qualifies, the flag itself
    dsm_surfel *spawn_rec; // [S]
    uint8_t *spawn_ok;     // [S]
    uint8_t *fused_flag;   // [S] set by k_fuse_surfels (besides the byte in `seeds`)
    float *seed_weight;    // [S] depth_weight(mean_depth) of the final seed, for k_fuse_surfels
    int32_t *spawn_idx;    // [S] seeds that do create a surfel, ascending
    // surfel map
    dsm_surfel *local;
    int32_t cap;
    dsm_surfel *fresh; // [S] surfels created by the current frame, seed order
    int32_t *n_local;
    int32_t *n_local_next;
    int32_t *n_new;
    // [cap/64 + 1] group g = records 64g .. 64g+63: a record of it was written since the flags were last cleared (k_fuse_surfels:
    // a wave stores its 64 records back only if one changed; k_frame_tail: refills, moves, appended surfels).  The drop-in call
    // downloads the flagged groups only (k_delta_pack clears them); flags left by other frames are cleared before it looks
    uint8_t *grp_dirty;
    uint64_t *hole_mask;  // [cap/64] bit i of word v: surfel 64v+i has update_times == 0
    int32_t *wave_prefix; // [cap/64] exclusive prefix of popcounts
    int32_t *holes;       // [cap] ascending indices of deleted slots
    int32_t *n_holes;
    // large maps (more than kTailFastWords * 64 surfels): holes per chunk of kTailChunkWords bitmap words, counted by
    // k_fuse_surfels, for the workgroups of k_frame_tail that list them; [n_hole_chunk] = their ticket counter,
    // [n_hole_chunk + 1] = the map size the frame started with.  All zero between frames (the tail's last workgroup resets them).
    int32_t *hole_chunk;
    int32_t n_hole_chunk;
    // sequencing
    const FrameParams *params;
    int32_t n_params;
    int32_t *cursor;      // frames this pipeline has finished; its next frame is params[cursor * cursor_mul + cursor_add]
    int32_t cursor_mul, cursor_add;
    int32_t *status; // sticky device-side error bits
    FrameCur *cur; // device memory, see FrameCur
    // optional per-wave phase stamps (shader clock) of the per-seed kernels; null unless DSM_FLAG_WAVE_STAMPS
    long long *stamps; // [5 kernels][n_seed][8]
};

// k_frame_tail: a thread owns kScanWords words of the hole bitmap per round, a workgroup kTailChunkWords; maps of up to
// kTailFastWords * 64 surfels take its one-workgroup fast path
constexpr int kScanWords = 8, kTailChunkWords = 1024 * kScanWords, kTailFastWords = 4096;
constexpr int kTailMaxBlocks = 33; // workgroups of k_frame_tail for a large map: one for the new surfels, the rest list holes

constexpr int kStatusCapacity = 1;
constexpr int kStatusBadPick = 2;
constexpr int kStatusBadLabels = 4; // a superpixel with more members than its 15 x 15 reach (injected label image)

// launch all kernels of one frame on `stream`.  with_compaction: SurfelMap::fuse_map semantics,
// otherwise FusionFunctions::fuse_initialize_map.  If ev != nullptr, an event is recorded before
// the first kernel and after every kernel (ev[0..n_stages]).
constexpr int kNumStages = 16;
constexpr int kLastSuperpixelStage = 13; // init_seeds .. seed_fit need the frame only; fuse_surfels + frame_tail need the map
extern const char *const kStageNames[kNumStages];
// map_upper_bound sizes the grid-stride pass of k_fuse_surfels (any bound does, the loop covers the map); tail_map_bound
// must be an upper bound of the map size whenever that exceeds kTailFastWords * 64 (it decides whether k_frame_tail gets
// the workgroups that list a large map's holes), and may be 0 while the map is known to be smaller.
// lanes_from: frames per launch from which the per-seed stages take their lane-per-seed forms (0 = the default for independent
// handles, kLaneBatch; the frame groups of one sequence pass 4: with other groups' kernels sharing the GPU the lane forms win
// from four frames on -- profiles/r06_wave_vs_lane.md)
// eigen33: the kernels that transform normals (k_seed_finish, k_fuse_surfels) in their Eigen >= 3.3 product-order instantiation
// (DSM_FLAG_EIGEN33_PRODUCTS of the handle; a captured graph holds the instantiation it was captured with)
hipError_t launch_frame(const DeviceCtx &ctx, bool eigen33, int map_upper_bound, int tail_map_bound, bool with_compaction,
                        hipStream_t stream, hipEvent_t *ev, int stage_lo = 0, int stage_hi = kNumStages - 1,
                        const DeviceCtx *d_batch = nullptr, int n_batch = 1, int lanes_from = 0);

struct WarpMat {
    float m[16]; // column-major 4x4
};
// d_mats: per-group matrices in device memory, or nullptr: `single16` (host pointer, copied into the kernel arguments)
hipError_t launch_warp(dsm_surfel *surfels, const int32_t *n_ptr, int n_fixed, const float *d_mats, const float *single16,
                       const int32_t *d_offsets, int n_groups, int n_upper, hipStream_t st,
                       const uint8_t *d_group_on = nullptr, float4 *d_cloud = nullptr);
hipError_t launch_mark(const DeviceCtx &ctx, int key, int n_upper, hipStream_t st);
hipError_t launch_repack_frames(uint8_t *d_img, float *d_depth, int pitch, int64_t slot_elems, const uint8_t *s_img, const float *s_depth, int w, int h,
                                int frames, hipStream_t st);
hipError_t launch_repack(uint8_t *d_img, float *d_depth, int pitch, const uint8_t *s_img, const float *s_depth, int w, int h,
                         hipStream_t st);
// uint16 depth of `frames` frames (rows src_row elements apart, frames src_frame apart) converted into the pitched depth planes
// d_depth + f * slot_elems: op = DSM_DEPTH_U16_DIVIDE (u / s) or DSM_DEPTH_U16_MULTIPLY (u * s), one launch, grid.y = frame
hipError_t launch_depth_u16(float *d_depth, int pitch, int64_t slot_elems, const uint16_t *src, int64_t src_row, int64_t src_frame, int w, int h,
                            int frames, float s, int op, hipStream_t st);
// packed colour pixels (`channels` = 3 or 4 bytes each, swap_rb: the first byte is B) of `frames` frames (rows src_row BYTES apart, frames
// src_frame bytes apart) converted into the pitched image planes d_img + f * slot_elems: grey = (R wr + G wg + B wb + (1 << (shift - 1)))
// >> shift (k_gray_u8), one launch, grid.y = frame.  The caller has checked the weights (dsm_frame_format's rules).
hipError_t launch_gray_u8(uint8_t *d_img, int pitch, int64_t slot_elems, const uint8_t *src, int64_t src_row, int64_t src_frame, int w, int h,
                          int frames, int channels, int swap_rb, int wr, int wg, int wb, int shift, hipStream_t st);
hipError_t launch_extract_marked(const DeviceCtx &ctx, dsm_surfel *out, int cap, float4 *cloud_out, hipStream_t st);
hipError_t launch_extract(const DeviceCtx &ctx, int key, dsm_surfel *out, int cap, int n_upper, hipStream_t st);
hipError_t launch_append_count(const DeviceCtx &ctx, int n, hipStream_t st);
// the flagged 64-record groups of the map (DeviceCtx::grp_dirty) packed into `buf` ([cap_groups][64] records) with their
// group numbers in `idx`; count[0] = how many there are (may exceed cap_groups: those are not packed), flags cleared
hipError_t launch_delta_pack(const DeviceCtx &ctx, dsm_surfel *buf, int32_t *idx, int32_t *count, int cap_groups, int n_upper, hipStream_t st);

// ---- point-cloud publications (dsm_k_cloud.h)
constexpr int kCloudNone = 0, kCloudMature = 1, kCloudNonzero = 2; // dsm_cloud_select of include/dsm.h
constexpr int kCloudChunks = 4;                   // 64-record chunks per wave of the compaction
constexpr int kCloudTile = 4 * 64 * kCloudChunks; // records per workgroup of its count / scatter passes (1024)
struct RawCloudParams {
    float rot[16]; // column-major 4x4, rotation in the upper 3x3 (xform_dir reads that part only)
    float t[3];
    float fx, fy, cx, cy;
};
// The surfel sequence that the cloud, the mesh, the render and the grid read (dsm_k_sequence.h walks it): first the runs of the
// inactive store, then the records of the resident map that pass `select`, in map order.
struct RunTable {       // the runs: output j of them is store record seg[3 s] + (j - seg[3 s + 2]) of the last run s with seg[3 s + 2] <= j
    const int32_t *seg; // device memory: n_seg triples (begin in the store, count > 0, exclusive offset in the sequence)
    int n_seg, total;   // total = the sum of the counts
};
struct MapPart {           // the map part: the records [0, min(*n_ptr, n_upper)) of rec that pass select (kCloudMature / kCloudNonzero)
    const dsm_surfel *rec;
    const int32_t *n_ptr;  // device memory: the map's size; n_upper = the handle's running bound of it, which sizes the grids
    int n_upper, select;
    int32_t *tile_cnt;     // ceil(n_upper / kCloudTile) ints of scratch: the tile counts, then their exclusive prefix
    int32_t *total;        // total[0] = how many records passed (also those a product's cap keeps out)
};
// XYZI of the map part, into out[0, cap)
hipError_t launch_cloud_map(const MapPart &mp, float4 *out, int cap, hipStream_t st);
// XYZI of the runs, read from the store's shadow src, to out[*base_ptr + ...] below cap: here the map part comes FIRST
hipError_t launch_cloud_gather(const float4 *src, const RunTable &rt, const int32_t *base_ptr, float4 *out, int cap, hipStream_t st);
// w * h world points of a pitched frame, column-major (index i * h + j for column i, row j)
// (eigen33: rotation_R * cam_point in Eigen >= 3.3's product order, DSM_FLAG_EIGEN33_PRODUCTS)
hipError_t launch_cloud_raw(const uint8_t *img, const float *depth, int pitch, int w, int h, const RawCloudParams &p, bool eigen33, float4 *out,
                            hipStream_t st);

// ---- the hexagon mesh (dsm_k_mesh.h)
constexpr int kMeshRef6 = 0, kMeshXyzRgba8 = 1; // dsm_mesh_vertex_layout of include/dsm.h
constexpr int mesh_surfel_bytes(int layout) { return layout == kMeshRef6 ? 144 : 96; }
// the six vertices of every record of the map part as records base, base + 1, ... of `out` (4-byte aligned; faster when 16-byte
// aligned), none at or beyond record cap
hipError_t launch_mesh_map(const MapPart &mp, int layout, void *out, int base, int cap, hipStream_t st);
// the runs of the store's records src as records 0, 1, ... of `out`, below cap
hipError_t launch_mesh_gather(const dsm_surfel *src, const RunTable &rt, int layout, void *out, int cap, hipStream_t st);
// 12 indices per surfel: 6 i + {0,1,2, 1,3,2, 2,3,4, 4,3,5}
hipError_t launch_mesh_indices(uint32_t *out, int n, hipStream_t st);

// ---- the map as an image (dsm_k_render.h; the definition is render_setup / render_hit / render_key of dsm_math.h)
constexpr int kRenderSmallW = 16, kRenderSmallArea = 256; // boxes up to this wide AND this large: 16 lanes per splat; others: a workgroup
struct RenderScratch {
    unsigned long long *keys; // [h][w]
    RenderSplat *splats;      // [n_seq]: small boxes from the front, large ones from the back
    int32_t *slot_of;         // [n_seq]: surfel number -> its splat record
    int32_t *counts;          // [2]: splats in the small list, in the large one
    int32_t n_seq;            // an upper bound of the sequence's length (the runs + the map's running bound)
};
// The surfel sequence (above): the runs of `store`, then the map part.  inv16: world -> cam.  ray_x [w] / ray_y [h]: ray_coeff
// of every column / row, in device memory.  Any plane may be null.
hipError_t launch_render(const dsm_surfel *store, const RunTable &rt, const MapPart &mp, const RenderCam &cam, const float *inv16, uint32_t flags,
                         bool eigen33, const RenderScratch &sc, const float *ray_x, const float *ray_y, float *depth, int32_t *index, float *normal,
                         uint8_t *intensity, hipStream_t st);

// ---- the map as a voxel grid (dsm_k_grid.h; the definition is grid_setup / grid_covers / grid_centre of dsm_math.h)
constexpr int kGridSmallW = 16, kGridSmallRows = 256; // boxes up to this wide along x AND of this many (y, z) rows: 16 lanes per surfel; others: a workgroup
struct GridScratch {
    GridSplat *splats;   // [n_seq]: small boxes from the front, large ones from the back
    int32_t *counts;     // [2]: surfels in the small list, in the large one
    int32_t n_seq;       // an upper bound of the sequence's length (the runs + the map's running bound)
    int32_t *cell_tiles; // [ceil(words / 256)]: scratch of the cell list's scan
};
struct GridOut {          // device memory; row-major [nz][ny][..]
    uint32_t *occupied;   // [nz][ny][wx], never null (the work plane of the others)
    uint32_t *inflated;   // [nz][ny][wx] or null
    int32_t *index;       // [nz][ny][nx] or null: then the bit set is splatted directly
    int32_t *cells;       // [cells_cap] or null
    int32_t cells_cap;
    int32_t *cells_total; // the number of set cells, or null: no cell list
    bool cells_of_inflated;
};
// The surfel sequence (above): the runs of `store`, then the map part.  inflate: the radius in voxels, 0 .. kGridMaxInflate.
hipError_t launch_grid(const dsm_surfel *store, const RunTable &rt, const MapPart &mp, const GridSpec &g, int inflate, const GridScratch &sc,
                       const GridOut &out, hipStream_t st);
// dst = src dilated by the voxels within radius r; pad bits of src ignored, of dst 0.  src != dst.
hipError_t launch_grid_inflate(const uint32_t *src, uint32_t *dst, const GridDims &d, int r, hipStream_t st);

// ---- the distance field of a bit set (dsm_k_field.h; the definition is field_key of dsm_math.h)
// bits: [nz][ny][wx] words, pad bits ignored.  1 <= r <= kFieldMaxDist, at most kFieldMaxVoxels voxels.  table: [r^2 + 1] metres by
// squared distance (field_table_entry).  ox: [voxels] bytes and mid: [voxels] words of scratch.  dist2 / nearest / distance: tight
// [nz][ny][nx] planes, any may be null.
hipError_t launch_field(const uint32_t *bits, const GridDims &d, int r, const float *table, int8_t *ox, uint32_t *mid, uint16_t *dist2,
                        int32_t *nearest, float *distance, hipStream_t st);

// ---- free space carved by depth frames, the three-state map and its frontier (dsm_k_carve.h; the definition is carve_voxel of dsm_carve.h)
struct CarveFrame {    // 72 bytes, in device memory: one per frame of the call
    float inv[16];     // world -> camera, column-major
    int64_t depth_off; // elements from the depth base to the frame's plane
};
// bits |= the voxels that carve_voxel frees against any of the n_frames frames (c.flags & kCarveReplace: bits = those voxels); pad bits
// are written 0.  c: everything but inv.  *count = the population of bits afterwards (cleared on `st` first).
hipError_t launch_carve(const float *depth_base, const CarveFrame *frames, int n_frames, const CarveConst &c, const GridDims &d, uint32_t *bits,
                        unsigned long long *count, hipStream_t st);
// occ / fre: [nz][ny][wx] words, pad bits ignored.  frontier ([nz][ny][wx]) is always written: the list and the count are taken from
// it; state ([nz][ny][nx] bytes), known_free and cells may be null.  cell_tiles: (words + 255) / 256 ints of scratch; *cells_total =
// the number of frontier voxels; no cell is written at or beyond cells_cap.
hipError_t launch_space(const uint32_t *occ, const uint32_t *fre, const GridDims &d, uint8_t *state, uint32_t *known_free, uint32_t *frontier,
                        int32_t *cells, int cells_cap, int32_t *cell_tiles, int32_t *cells_total, hipStream_t st);

// ---- candidate camera poses scored against the grid (dsm_k_view.h; the definition is in dsm_view.h)
// occ / fre / target: [nz][ny][wx] words, pad bits ignored; target may be null.  c: the grid's origin and voxel and the view camera,
// everything but inv, which is the pose's.  scores: [n_poses], cleared on `st` first; visible: [n_poses][nz][ny][wx] or null, pad
// bits written 0.
hipError_t launch_view(const ViewPose *poses, int n_poses, const CarveConst &c, uint32_t flags, const GridDims &d, const uint32_t *occ,
                       const uint32_t *fre, const uint32_t *target, ViewCounts *scores, uint32_t *visible, hipStream_t st);

// ---- connected components of a bit set (dsm_k_components.h; the definition is in dsm_components.h)
// src: [nz][ny][wx] words, pad bits ignored; at most kFieldMaxVoxels voxels.  label: [voxels], always written (the caller's plane or
// scratch); work: [voxels] of scratch; root_bits / keep_bits: [words]; root_tiles / keep_tiles: (words + 255) / 256 ints each.  table
// may be null: no statistics; no entry is written at or beyond cap.  *n_all = the components, *n_kept = those with count >= min_count.
hipError_t launch_components(const uint32_t *src, const int32_t *tag_src, const GridDims &d, int connectivity, int min_count, int32_t *label,
                             int32_t *work, uint32_t *root_bits, uint32_t *keep_bits, int32_t *root_tiles, int32_t *keep_tiles, dsm_component *table,
                             int cap, int32_t *n_all, int32_t *n_kept, hipStream_t st);

// ---- a depth frame against the rendered map (dsm_k_align.h; the definition is align_pixel of dsm_align.h)
// One evaluation: clears sums[29] on `st`, then adds the fixed-point terms of every sampled pixel of the frame plane `depth`
// ([h][pitch]) that passes align_pixel against the model planes zm [mh][mw] and nm [mh][mw][3].  c from align_prepare, with T set.
hipError_t launch_align(const AlignConst &c, const float *depth, const float *zm, const float *nm, unsigned long long *sums, hipStream_t st);

} // namespace dsm
