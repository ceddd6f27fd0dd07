// align_host.cpp -- the frame-to-map alignment's definition compiled for the host (tests/test_cpu_align.py, tests/test_gpu_align.py):
// the evaluation over the sampled pixels in a caller-given order, and the loop, over align_pixel / align_loop of
// csrc/dsm_align.h -- the functions the kernel of csrc/dsm_k_align.h and dsm_align_frame call.
// Build: g++ -std=c++17 -O2 -ffp-contract=off -shared -fPIC.  With -DALIGN_HOST_MAIN the file is a program: the evaluation and
// the loop over the planes of the files named on the command line and over random-bit planes; exit status 0 iff every order of
// the pixels gives the same sums (run under the sanitizers by the tests).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../densesurfelmapping_amd/csrc/dsm_math.h"
#include "../include/dsm.h"

extern "C" {

struct align_host_frame_desc { // the frame side: the handle's image size, row pitch in floats, intrinsics and fuse distances
    int32_t width, height, pitch;
    float fx, fy, cx, cy, near_dist, far_dist;
};

} // extern "C"

namespace {

dsm::RenderCam to_cam(const dsm_render_camera &c) {
    dsm::RenderCam cam;
    cam.w = c.width; cam.h = c.height;
    cam.fx = c.fx; cam.fy = c.fy; cam.cx = c.cx; cam.cy = c.cy;
    cam.near_d = c.near_dist; cam.far_d = c.far_dist;
    return cam;
}

const char *prepare(const align_host_frame_desc &f, const dsm_render_camera &cam, const dsm_align_params &p, dsm::AlignConst &c) {
    if (p.struct_size != sizeof(dsm_align_params)) return "struct_size";
    if (p.max_iterations < 1) return "max_iterations < 1";
    if (f.width < 1 || f.height < 1 || f.pitch < f.width) return "frame size";
    dsm::AlignFrame af;
    af.w = f.width; af.h = f.height; af.pitch = f.pitch;
    af.fx = f.fx; af.fy = f.fy; af.cx = f.cx; af.cy = f.cy;
    af.near_d = f.near_dist; af.far_d = f.far_dist;
    return dsm::align_prepare(af, to_cam(cam), p.stride, p.dist_max, p.min_view_cos, p.huber, c);
}

// order: n_order sampled-pixel numbers (row-major over the sampled grid), or null = all of them in row-major order
template <typename Acc>
void evaluate(const dsm::AlignConst &c, const float *depth, const float *zm, const float *nm, const int64_t *order, int64_t n_order, Acc *acc,
              int64_t *census, int8_t *exits) {
    const int64_t total = dsm::align_sampled(c.f.w, c.f.h, c.stride);
    const int64_t n = order ? n_order : total;
    for (int64_t j = 0; j < n; j++) {
        const int64_t i = order ? order[j] : j;
        if (i < 0 || i >= total) continue;
        int u, v;
        dsm::align_sample(c, i, u, v);
        const dsm::AlignExit x = dsm::align_pixel(c, depth, zm, nm, u, v, acc);
        if (census) census[x]++;
        if (exits) exits[i] = (int8_t)x;
    }
}

} // namespace

extern "C" {

float align_host_qmax(const dsm_render_camera *cam) { return dsm::align_qmax(to_cam(*cam)); }
int align_host_scale(const dsm_render_camera *cam, int64_t n_sampled) { return dsm::align_scale_log2(to_cam(*cam), n_sampled); }
int align_host_exits(void) { return dsm::kAlignExits; }

// One evaluation.  census: kAlignExits counters or null; exits: the exit of every sampled pixel or null.  -1: refused arguments.
int align_host_equations(const align_host_frame_desc *frame, const float *depth, const dsm_render_camera *cam, const float *zm, const float *nm,
                         const float *T16, const dsm_align_params *params, const int64_t *order, int64_t n_order, int64_t *sums, int32_t *scale_log2,
                         int64_t *census, int8_t *exits) {
    dsm::AlignConst c;
    if (prepare(*frame, *cam, *params, c)) return -1;
    for (int k = 0; k < 16; k++) {
        if (!(fabsf(T16[k]) < __builtin_inff())) return -1;
        c.T[k] = T16[k];
    }
    for (int k = 0; k < dsm::kAlignSums; k++) sums[k] = 0;
    if (census)
        for (int k = 0; k < dsm::kAlignExits; k++) census[k] = 0;
    evaluate<int64_t>(c, depth, zm, nm, order, n_order, sums, census, exits);
    if (scale_log2) *scale_log2 = c.scale_log2;
    return 0;
}

// The same evaluation accumulated in 128 bits beside the int64 one.  1: every sum agrees; *fill = the largest |sum| / 2^63.
int align_host_equations_wide(const align_host_frame_desc *frame, const float *depth, const dsm_render_camera *cam, const float *zm, const float *nm,
                              const float *T16, const dsm_align_params *params, int64_t *sums, double *fill) {
    dsm::AlignConst c;
    if (prepare(*frame, *cam, *params, c)) return -1;
    for (int k = 0; k < 16; k++) c.T[k] = T16[k];
    __int128 wide[dsm::kAlignSums];
    uint64_t narrow[dsm::kAlignSums]; // (unsigned: a wrap is then defined, and shows as a difference)
    for (int k = 0; k < dsm::kAlignSums; k++) wide[k] = 0, narrow[k] = 0;
    evaluate<__int128>(c, depth, zm, nm, nullptr, 0, wide, nullptr, nullptr);
    evaluate<uint64_t>(c, depth, zm, nm, nullptr, 0, narrow, nullptr, nullptr);
    int same = 1;
    double top = 0.0;
    for (int k = 0; k < dsm::kAlignSums; k++) {
        sums[k] = (int64_t)narrow[k];
        if ((__int128)sums[k] != wide[k]) same = 0;
        const double a = (double)(wide[k] < 0 ? -wide[k] : wide[k]) / 9223372036854775808.0;
        if (a > top) top = a;
    }
    *fill = top;
    return same;
}

// The loop against given model planes (what dsm_align_frame does behind its render).  -1: refused arguments.
int align_host_frame(const align_host_frame_desc *frame, const float *depth, const dsm_render_camera *cam, const float *zm, const float *nm,
                     const float *pose16_guess, const dsm_align_params *params, dsm_align_result *out) {
    dsm::AlignConst c;
    if (prepare(*frame, *cam, *params, c)) return -1;
    dsm::AlignLoop lp;
    lp.max_iterations = params->max_iterations;
    lp.min_pixels = params->min_pixels;
    lp.stop_translation = (double)params->stop_translation;
    lp.stop_rotation = (double)params->stop_rotation;
    lp.scale_log2 = c.scale_log2;
    dsm::AlignOutcome o;
    const int rc = dsm::align_loop(lp, [&](const float *T16, int64_t *sums) {
        for (int k = 0; k < 16; k++) c.T[k] = T16[k];
        for (int k = 0; k < dsm::kAlignSums; k++) sums[k] = 0;
        evaluate<int64_t>(c, depth, zm, nm, nullptr, 0, sums, nullptr, nullptr);
        return 0;
    }, o);
    if (rc) return rc;
    dsm::align_refined_pose(pose16_guess, o.T, out->pose16);
    for (int k = 0; k < 16; k++) out->T16[k] = (float)o.T[k];
    out->status = o.status;
    out->iterations = o.iterations;
    out->n_pixels = (int32_t)o.n_pixels;
    out->scale_log2 = c.scale_log2;
    out->rms = o.rms;
    for (int k = 0; k < dsm::kAlignSums; k++) out->sums[k] = o.sums[k];
    return 0;
}

} // extern "C"

#ifdef ALIGN_HOST_MAIN
namespace {

uint64_t g_state = 0x9e3779b97f4a7c15ull;
uint32_t next_u32() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 16);
}

struct Case {
    align_host_frame_desc f;
    dsm_render_camera cam;
    std::vector<float> depth, zm, nm;
};

// a case file: align_host_frame_desc, dsm_render_camera, then the three planes as floats
bool read_case(const char *path, Case &c) {
    std::FILE *fp = std::fopen(path, "rb");
    if (!fp) return false;
    bool ok = std::fread(&c.f, sizeof c.f, 1, fp) == 1 && std::fread(&c.cam, sizeof c.cam, 1, fp) == 1;
    ok = ok && c.f.width >= 1 && c.f.width <= 4096 && c.f.height >= 1 && c.f.height <= 4096 && c.f.pitch >= c.f.width && c.f.pitch <= 8192;
    ok = ok && c.cam.width >= 1 && c.cam.width <= 4096 && c.cam.height >= 1 && c.cam.height <= 4096;
    if (ok) {
        c.depth.resize((size_t)c.f.pitch * c.f.height);
        c.zm.resize((size_t)c.cam.width * c.cam.height);
        c.nm.resize(c.zm.size() * 3);
        ok = std::fread(c.depth.data(), 4, c.depth.size(), fp) == c.depth.size() && std::fread(c.zm.data(), 4, c.zm.size(), fp) == c.zm.size() &&
             std::fread(c.nm.data(), 4, c.nm.size(), fp) == c.nm.size();
    }
    std::fclose(fp);
    return ok;
}

bool run_case(const Case &c, const char *what) {
    static const float poses[2][16] = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1},
                                       {0.8f, 0, -0.6f, 0, 0, 1, 0, 0, 0.6f, 0, 0.8f, 0, 0.25f, -0.125f, 0.5f, 1}};
    bool ok = true;
    for (int stride = 1; stride <= 3; stride++)
        for (int hub = 0; hub < 2; hub++)
            for (const float *T : poses) {
                dsm_align_params p;
                p.struct_size = sizeof p;
                p.max_iterations = 4;
                p.stride = stride;
                p.dist_max = 0.5f;
                p.min_view_cos = 0.2f;
                p.huber = hub ? 0.02f : 0.0f;
                p.min_pixels = 6;
                p.stop_translation = 1e-4f;
                p.stop_rotation = 1e-4f;
                const int64_t total = dsm::align_sampled(c.f.width, c.f.height, stride);
                std::vector<int64_t> rev((size_t)total);
                for (int64_t i = 0; i < total; i++) rev[(size_t)i] = total - 1 - i;
                int64_t a[dsm::kAlignSums], b[dsm::kAlignSums];
                int32_t k = 0;
                if (align_host_equations(&c.f, c.depth.data(), &c.cam, c.zm.data(), c.nm.data(), T, &p, nullptr, 0, a, &k, nullptr, nullptr) ||
                    align_host_equations(&c.f, c.depth.data(), &c.cam, c.zm.data(), c.nm.data(), T, &p, rev.data(), total, b, &k, nullptr, nullptr)) {
                    std::fprintf(stderr, "%s: refused\n", what);
                    return false;
                }
                if (memcmp(a, b, sizeof a)) {
                    std::fprintf(stderr, "%s stride %d huber %d: the reversed order gives other sums\n", what, stride, hub);
                    ok = false;
                }
                dsm_align_result r;
                if (align_host_frame(&c.f, c.depth.data(), &c.cam, c.zm.data(), c.nm.data(), T, &p, &r)) ok = false;
            }
    return ok;
}

} // namespace

int main(int argc, char **argv) {
    bool ok = true;
    for (int a = 1; a < argc; a++) {
        Case c;
        if (!read_case(argv[a], c)) {
            std::fprintf(stderr, "cannot read %s\n", argv[a]);
            return 2;
        }
        ok = run_case(c, argv[a]) && ok;
    }
    // random bits in every plane; half of the values replaced by ones of ordinary magnitude, so that pixels get past the first gates
    Case r;
    r.f = {45, 23, 64, 40.5f, 38.25f, 22.3f, 11.6f, 0.3f, 30.0f};
    r.cam = {70, 37, 64.0f, 61.5f, 35.0f, 18.25f, 0.05f, 8.0f};
    r.depth.resize((size_t)r.f.pitch * r.f.height);
    r.zm.resize((size_t)r.cam.width * r.cam.height);
    r.nm.resize(r.zm.size() * 3);
    for (std::vector<float> *pl : {&r.depth, &r.zm, &r.nm})
        for (float &v : *pl) {
            const uint32_t bits = next_u32();
            memcpy(&v, &bits, 4);
            if (next_u32() & 1) v = pl == &r.nm ? (float)(int32_t)(next_u32() % 2001 - 1000) * 0.001f : (float)(next_u32() % 4000) * 0.001f + 0.1f;
        }
    ok = run_case(r, "random bits") && ok;
    std::printf("%s\n", ok ? "align_host: every order agrees" : "align_host: MISMATCH");
    return ok ? 0 : 1;
}
#endif
