// dsm_k_render.h -- the surfel map as an image from any pose (dsm_render_compose): depth, surfel number, camera-frame normal
// and intensity of the nearest disc along every pixel's ray.  The definition (render_setup / render_hit / render_key) is in
// dsm_math.h and shared with the host checker tests/render_host.cpp; this file is how it is evaluated:
//   k_render_clear     the key plane u64 [h][w] to all ones (no hit)
//   k_render_setup_map the map part and the runs of the surfel sequence (dsm_k_sequence.h: map_tile_walk, run_source): a lane
//   k_render_setup_run per surfel does render_setup; survivors are appended as RenderSplat records to ONE array -- boxes of at
//                      most kRenderSmallW x kRenderSmallArea from the front, larger ones from the back (two_ended_slot).
//                      slot_of[number] = where the record went (k_render_resolve's way back).
//   k_render_splat     the small list: 16 lanes per splat, four splats per wave; the 16 lanes take one box row per trip, so a
//                      wave's atomic instruction touches up to four runs of 128 bytes instead of 64 scattered lines
//   k_render_splat_big the large list: a workgroup per splat in turn (grid-stride), 16 rows at a time, so a disc in front of the
//                      camera costs w h / 256 trips per thread and not w h trips in one lane
//   k_render_resolve   a thread per pixel: key -> the planes asked for
// A hit does a plain load of the pixel's key first and skips the atomic when that is already <= its own: keys only decrease,
// so a stale value can cost an atomic, never a wrong skip.  The atomic is atomicMin on unsigned long long (global_atomic_umin_x2),
// plain C++.  What has been measured on this chip (MI355X_MICROARCH.md, global float atomics) is the no-return fp32 add: full
// rate for 256 contiguous bytes or two 128-byte segments per wave instruction, about 17x slower with 64 lanes in 64 different
// rows -- hence the lanes of a splat side by side.  The 64-bit integer min is NOT measured there, nor are four segments.
// Every loop is bounded by a clipped box, i.e. by w * h; the lists cannot overflow; no workgroup waits on another.
#pragma once
#include "dsm_k_cloud.h"

namespace dsm {

__global__ __launch_bounds__(256) void k_render_clear(unsigned long long *__restrict__ keys, int n_px, int32_t *__restrict__ counts) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_px; i += gridDim.x * 256) keys[i] = kRenderEmpty;
    if (blockIdx.x == 0 && threadIdx.x < 2) counts[threadIdx.x] = 0;
}

struct RenderSetupArgs {
    RenderCam cam;
    float inv[16];
    uint32_t flags;
    int32_t n_seq; // length of the splat array = an upper bound of the sequence's length
};

// called by whole waves; `valid` lanes hold record r with sequence number `number`
template <bool E33>
__device__ __forceinline__ void render_emit(const RenderSetupArgs &a, bool valid, const dsm_surfel *__restrict__ r, int number,
                                            RenderSplat *__restrict__ splats, int32_t *__restrict__ slot_of, int32_t *__restrict__ counts) {
    RenderSplat s = {};
    bool keep = false;
    if (valid) keep = render_setup<E33>(a.cam, a.inv, a.flags, *r, number, s);
    const int bw = (int)s.x1 - (int)s.x0, bh = (int)s.y1 - (int)s.y0;
    const bool small = keep && bw <= kRenderSmallW && bw * bh <= kRenderSmallArea;
    const int slot = two_ended_slot(small, keep && !small, counts, a.n_seq);
    if (keep && slot >= 0 && slot < a.n_seq && number >= 0 && number < a.n_seq) { // (always: survivors <= sequence <= n_seq)
        splats[slot] = s;
        slot_of[number] = slot;
    }
}

template <bool E33>
__global__ __launch_bounds__(256) void k_render_setup_map(const MapPart mp, int base, const RenderSetupArgs a, RenderSplat *__restrict__ splats,
                                                          int32_t *__restrict__ slot_of, int32_t *__restrict__ counts) {
    map_tile_walk(mp, base, [&](unsigned long long m, int at, int i) {
        if (m) // (wave-uniform)
            render_emit<E33>(a, (m >> lane_id()) & 1ull, mp.rec + i, at + rank_below(m), splats, slot_of, counts);
    });
}

// output j of the runs is surfel j of the sequence.  A wave takes 64 consecutive outputs at a time.
template <bool E33>
__global__ __launch_bounds__(256) void k_render_setup_run(const dsm_surfel *__restrict__ src, const RunTable rt, const RenderSetupArgs a,
                                                          RenderSplat *__restrict__ splats, int32_t *__restrict__ slot_of, int32_t *__restrict__ counts) {
    const int lane = lane_id(), wv = threadIdx.x >> 6;
    for (int64_t j0 = ((int64_t)blockIdx.x * 4 + wv) * 64; j0 < rt.total; j0 += (int64_t)gridDim.x * 256) {
        const int j = (int)j0 + lane;
        const bool valid = j < rt.total;
        render_emit<E33>(a, valid, valid ? src + run_source(rt, j) : src, j, splats, slot_of, counts);
    }
}

struct RenderImage {
    unsigned long long *keys; // [h][w]
    const float *ray_x, *ray_y; // [w], [h]: ray_coeff of every column and row
    int w, h;
    float near_d, far_d;
};

__device__ __forceinline__ void render_pixel(const RenderImage &im, const RenderSplat &s, int x, int y) {
    float z;
    if (!render_hit(s, im.ray_x[x], im.ray_y[y], im.near_d, im.far_d, z)) return;
    const unsigned long long key = render_key(z, s.number);
    unsigned long long *p = im.keys + ((int64_t)y * im.w + x);
    if (*p > key) atomicMin(p, key);
}

// box inside the image, whatever the record holds
__device__ __forceinline__ void render_box(const RenderImage &im, const RenderSplat &s, int &x0, int &x1, int &y0, int &y1) {
    x0 = s.x0; y0 = s.y0;
    x1 = (int)s.x1 < im.w ? (int)s.x1 : im.w;
    y1 = (int)s.y1 < im.h ? (int)s.y1 : im.h;
}

__global__ __launch_bounds__(256) void k_render_splat(const RenderSplat *__restrict__ splats, const int32_t *__restrict__ counts, int n_seq, const RenderImage im) {
    const int n = counts[0] < n_seq ? counts[0] : n_seq;
    const int sub = threadIdx.x >> 4, l = threadIdx.x & 15;
    for (int64_t i = (int64_t)blockIdx.x * 16 + sub; i < n; i += (int64_t)gridDim.x * 16) {
        const RenderSplat s = splats[i];
        int x0, x1, y0, y1;
        render_box(im, s, x0, x1, y0, y1);
        for (int y = y0; y < y1; y++)
            for (int x = x0 + l; x < x1; x += 16) render_pixel(im, s, x, y);
    }
}

__global__ __launch_bounds__(256) void k_render_splat_big(const RenderSplat *__restrict__ splats, const int32_t *__restrict__ counts, int n_seq, const RenderImage im) {
    const int n = counts[1] < n_seq ? counts[1] : n_seq;
    const int row = threadIdx.x >> 4, l = threadIdx.x & 15;
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const RenderSplat s = splats[n_seq - 1 - i];
        int x0, x1, y0, y1;
        render_box(im, s, x0, x1, y0, y1);
        for (int y = y0 + row; y < y1; y += 16)
            for (int x = x0 + l; x < x1; x += 16) render_pixel(im, s, x, y);
    }
}

struct RenderPlanes {
    float *depth;
    int32_t *index;
    float *normal;
    uint8_t *intensity;
};

__global__ __launch_bounds__(256) void k_render_resolve(const unsigned long long *__restrict__ keys, int n_px, const RenderSplat *__restrict__ splats,
                                                        const int32_t *__restrict__ slot_of, int n_seq, const RenderPlanes out) {
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n_px; i += gridDim.x * 256) {
        const unsigned long long key = keys[i];
        const bool hit = key != kRenderEmpty;
        const int number = (int)(uint32_t)key;
        if (out.depth) out.depth[i] = hit ? __uint_as_float((uint32_t)(key >> 32)) : 0.0f;
        if (out.index) out.index[i] = hit ? number : -1;
        if (out.normal || out.intensity) {
            float nx = 0.0f, ny = 0.0f, nz = 0.0f;
            uint32_t c = 0;
            if (hit && number >= 0 && number < n_seq) {
                const int slot = slot_of[number];
                if (slot >= 0 && slot < n_seq) {
                    const RenderSplat *s = splats + slot;
                    nx = s->nc[0]; ny = s->nc[1]; nz = s->nc[2];
                    c = s->intensity;
                }
            }
            if (out.normal) {
                out.normal[3 * (int64_t)i] = nx; out.normal[3 * (int64_t)i + 1] = ny; out.normal[3 * (int64_t)i + 2] = nz;
            }
            if (out.intensity) out.intensity[i] = (uint8_t)c;
        }
    }
}

// keys, then the lists: launched in this order on one stream
hipError_t launch_render(const dsm_surfel *store, const RunTable &rt, const MapPart &mp, const RenderCam &cam, const float *inv16, uint32_t flags,
                         bool eigen33, const RenderScratch &sc, const float *ray_x, const float *ray_y, float *depth, int32_t *index, float *normal,
                         uint8_t *intensity, hipStream_t st) {
    const int n_px = cam.w * cam.h; // <= 8192 * 8192
    int px_blocks = (n_px + 255) / 256;
    if (px_blocks > 8192) px_blocks = 8192;
    hipLaunchKernelGGL(k_render_clear, dim3(px_blocks), dim3(256), 0, st, sc.keys, n_px, sc.counts);
    RenderSetupArgs a;
    a.cam = cam;
    for (int k = 0; k < 16; k++) a.inv[k] = inv16[k];
    a.flags = flags;
    a.n_seq = sc.n_seq;
    if (rt.n_seg > 0 && rt.total > 0) {
        if (eigen33) hipLaunchKernelGGL(k_render_setup_run<true>, dim3(run_blocks(rt.total)), dim3(256), 0, st, store, rt, a, sc.splats, sc.slot_of, sc.counts);
        else hipLaunchKernelGGL(k_render_setup_run<false>, dim3(run_blocks(rt.total)), dim3(256), 0, st, store, rt, a, sc.splats, sc.slot_of, sc.counts);
    }
    const hipError_t e = launch_map_offsets(mp, st);
    if (e != hipSuccess) return e;
    if (map_tiles(mp) > 0) {
        if (eigen33) hipLaunchKernelGGL(k_render_setup_map<true>, dim3(map_tiles(mp)), dim3(256), 0, st, mp, rt.total, a, sc.splats, sc.slot_of, sc.counts);
        else hipLaunchKernelGGL(k_render_setup_map<false>, dim3(map_tiles(mp)), dim3(256), 0, st, mp, rt.total, a, sc.splats, sc.slot_of, sc.counts);
    }
    RenderImage im;
    im.keys = sc.keys;
    im.ray_x = ray_x;
    im.ray_y = ray_y;
    im.w = cam.w;
    im.h = cam.h;
    im.near_d = cam.near_d;
    im.far_d = cam.far_d;
    if (sc.n_seq > 0) {
        int blocks = launch_blocks(sc.n_seq, 16, 16384);
        hipLaunchKernelGGL(k_render_splat, dim3(blocks), dim3(256), 0, st, (const RenderSplat *)sc.splats, (const int32_t *)sc.counts, sc.n_seq, im);
        blocks = sc.n_seq < 2048 ? sc.n_seq : 2048;
        hipLaunchKernelGGL(k_render_splat_big, dim3(blocks), dim3(256), 0, st, (const RenderSplat *)sc.splats, (const int32_t *)sc.counts, sc.n_seq, im);
    }
    RenderPlanes out;
    out.depth = depth;
    out.index = index;
    out.normal = normal;
    out.intensity = intensity;
    hipLaunchKernelGGL(k_render_resolve, dim3(px_blocks), dim3(256), 0, st, (const unsigned long long *)sc.keys, n_px, (const RenderSplat *)sc.splats,
                       (const int32_t *)sc.slot_of, sc.n_seq, out);
    return hipGetLastError();
}

} // namespace dsm
