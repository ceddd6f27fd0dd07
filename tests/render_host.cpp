// render_host.cpp -- the map renderer's definition compiled for the host (tests/test_cpu_render.py, tests/test_gpu_render.py):
// two serial renderers over render_setup / render_hit / render_key of csrc/dsm_math.h, the functions the HIP kernels of
// csrc/dsm_k_render.h call.
//   boxed   every surfel that render_setup keeps visits the pixels of its box
//   brute   every surfel is tested against every pixel of the image; of render_setup only the camera-frame quantities are
//           used, its verdict and its box are ignored (the back-face rule is restated here)
// boxed == brute says that the rejects and the box lose no hit.  Build: g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC.
// With -DRENDER_HOST_MAIN the file is a program: both renderers over the records of the files named on the command line and
// over random-bit records, at two image sizes; exit status 0 iff they agree everywhere (run under the sanitizers by the tests).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../densesurfelmapping_amd/csrc/dsm_math.h"
#include "../include/dsm.h"

namespace {

dsm::RenderCam to_cam(const dsm_render_camera &c) {
    dsm::RenderCam cam;
    cam.w = c.width; cam.h = c.height;
    cam.fx = c.fx; cam.fy = c.fy; cam.cx = c.cx; cam.cy = c.cy;
    cam.near_d = c.near_dist; cam.far_d = c.far_dist;
    return cam;
}

struct Image {
    int w, h;
    std::vector<uint64_t> key;
    std::vector<float> nrm;      // of the winner
    std::vector<uint8_t> intensity;
    std::vector<float> rx, ry;
    Image(const dsm::RenderCam &cam) : w(cam.w), h(cam.h), key((size_t)cam.w * cam.h, dsm::kRenderEmpty), nrm((size_t)cam.w * cam.h * 3, 0.f),
                                       intensity((size_t)cam.w * cam.h, 0), rx((size_t)cam.w), ry((size_t)cam.h) {
        for (int x = 0; x < w; x++) rx[(size_t)x] = dsm::ray_coeff(x, cam.cx, cam.fx);
        for (int y = 0; y < h; y++) ry[(size_t)y] = dsm::ray_coeff(y, cam.cy, cam.fy);
    }
    void test(const dsm::RenderCam &cam, const dsm::RenderSplat &s, int x, int y) {
        float z;
        if (!dsm::render_hit(s, rx[(size_t)x], ry[(size_t)y], cam.near_d, cam.far_d, z)) return;
        const uint64_t k = dsm::render_key(z, s.number);
        const size_t i = (size_t)y * w + x;
        if (k < key[i]) {
            key[i] = k;
            for (int d = 0; d < 3; d++) nrm[3 * i + d] = s.nc[d];
            intensity[i] = (uint8_t)s.intensity;
        }
    }
};

template <bool E33> void render(const dsm_surfel *s, int64_t n, const dsm::RenderCam &cam, const float *inv16, uint32_t flags, bool brute, Image &im) {
    for (int64_t i = 0; i < n; i++) {
        dsm::RenderSplat sp;
        const bool keep = dsm::render_setup<E33>(cam, inv16, flags, s[i], (int)i, sp);
        if (brute) {
            if ((flags & DSM_RENDER_CULL_BACKFACES) && sp.d >= 0.0f) continue;
            for (int y = 0; y < cam.h; y++)
                for (int x = 0; x < cam.w; x++) im.test(cam, sp, x, y);
        } else if (keep) {
            for (int y = sp.y0; y < sp.y1; y++)
                for (int x = sp.x0; x < sp.x1; x++) im.test(cam, sp, x, y);
        }
    }
}

void run(const dsm_surfel *s, int64_t n, const dsm::RenderCam &cam, const float *inv16, uint32_t flags, int eigen33, int brute, Image &im) {
    if (eigen33) render<true>(s, n, cam, inv16, flags, brute != 0, im);
    else render<false>(s, n, cam, inv16, flags, brute != 0, im);
}

} // namespace

extern "C" {

// the planes of the sequence s[0 .. n) (already in render order); any output may be null
void render_host(const dsm_surfel *s, int64_t n, const dsm_render_camera *camera, const float *inv16, uint32_t flags, int eigen33, int brute,
                 float *depth, int32_t *index, float *normal, uint8_t *intensity) {
    const dsm::RenderCam cam = to_cam(*camera);
    Image im(cam);
    run(s, n, cam, inv16, flags, eigen33, brute, im);
    const size_t px = (size_t)cam.w * cam.h;
    for (size_t i = 0; i < px; i++) {
        const bool hit = im.key[i] != dsm::kRenderEmpty;
        const uint32_t zb = (uint32_t)(im.key[i] >> 32);
        float z;
        memcpy(&z, &zb, 4);
        if (depth) depth[i] = hit ? z : 0.0f;
        if (index) index[i] = hit ? (int32_t)(uint32_t)im.key[i] : -1;
        if (normal)
            for (int d = 0; d < 3; d++) normal[3 * i + d] = im.nrm[3 * i + d];
        if (intensity) intensity[i] = im.intensity[i];
    }
}

// render_setup's verdict and box of every record: box[4 i ..] = x0 y0 x1 y1, keep[i]
void render_host_boxes(const dsm_surfel *s, int64_t n, const dsm_render_camera *camera, const float *inv16, uint32_t flags, int eigen33, int32_t *box,
                       uint8_t *keep) {
    const dsm::RenderCam cam = to_cam(*camera);
    for (int64_t i = 0; i < n; i++) {
        dsm::RenderSplat sp;
        keep[i] = eigen33 ? dsm::render_setup<true>(cam, inv16, flags, s[i], (int)i, sp) : dsm::render_setup<false>(cam, inv16, flags, s[i], (int)i, sp);
        box[4 * i] = sp.x0; box[4 * i + 1] = sp.y0; box[4 * i + 2] = sp.x1; box[4 * i + 3] = sp.y1;
    }
}

// the closed-form world -> cam matrix dsm_render_compose uses for a NULL inverse
void render_host_inverse(const float *pose16, float *inv16) { dsm::inverse4<float>(pose16, inv16); }

} // extern "C"

#ifdef RENDER_HOST_MAIN
namespace {

bool agree(const std::vector<dsm_surfel> &s, const dsm_render_camera &c, const float *inv16, uint32_t flags, int eigen33, const char *what) {
    const dsm::RenderCam cam = to_cam(c);
    Image a(cam), b(cam);
    run(s.data(), (int64_t)s.size(), cam, inv16, flags, eigen33, 0, a);
    run(s.data(), (int64_t)s.size(), cam, inv16, flags, eigen33, 1, b);
    size_t bad = 0;
    for (size_t i = 0; i < a.key.size(); i++) bad += a.key[i] != b.key[i];
    if (bad) std::fprintf(stderr, "%s %dx%d flags %u e33 %d: %zu pixels differ\n", what, c.width, c.height, flags, eigen33, bad);
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
    std::vector<std::vector<dsm_surfel>> sets;
    for (int a = 1; a < argc; a++) {
        std::FILE *f = std::fopen(argv[a], "rb");
        if (!f) {
            std::fprintf(stderr, "cannot open %s\n", argv[a]);
            return 2;
        }
        std::vector<dsm_surfel> s;
        dsm_surfel r;
        while (std::fread(&r, sizeof r, 1, f) == 1) s.push_back(r);
        std::fclose(f);
        sets.push_back(s);
    }
    std::vector<dsm_surfel> rnd(3000);
    for (dsm_surfel &r : rnd) {
        uint32_t w[11];
        for (uint32_t &v : w) v = next_u32();
        memcpy(&r, w, sizeof r);
        if (next_u32() & 1) { // half of them with a position and a size of ordinary magnitude: NaN patterns elsewhere
            r.px = (float)(int32_t)(next_u32() % 2001 - 1000) * 0.004f;
            r.py = (float)(int32_t)(next_u32() % 2001 - 1000) * 0.004f;
            r.pz = (float)(next_u32() % 4000) * 0.01f - 5.0f;
            if (next_u32() & 1) r.size = (float)(next_u32() % 1000) * 0.003f;
        }
    }
    sets.push_back(rnd);
    const dsm_render_camera cams[2] = {{48, 32, 40.5f, 38.25f, 23.3f, 15.6f, 0.3f, 30.0f}, {70, 37, 64.0f, 61.5f, 35.0f, 18.25f, 0.05f, 8.0f}};
    // identity, and a camera turned about y and moved (cam -> world; the renderers take its inverse)
    const float poses[2][16] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1},
                                {0.8f, 0, -0.6f, 0, 0, 1, 0, 0, 0.6f, 0, 0.8f, 0, 0.25f, -0.125f, 0.5f, 1}};
    bool ok = true;
    for (const std::vector<dsm_surfel> &s : sets)
        for (const dsm_render_camera &c : cams)
            for (const float *pose : poses) {
                float inv[16];
                render_host_inverse(pose, inv);
                for (uint32_t flags = 0; flags < 2; flags++)
                    for (int e33 = 0; e33 < 2; e33++) ok = agree(s, c, inv, flags, e33, "set") && ok;
            }
    std::printf("%s\n", ok ? "render_host: boxed == brute" : "render_host: MISMATCH");
    return ok ? 0 : 1;
}
#endif
