// sanitize_frame_format.cpp -- the host code of the *_fmt family under AddressSanitizer + UBSan, as a stand-alone program on the
// CPU: dsm_frame_format's checks (csrc/dsm_frame_format.h) and dsm_host_pack_frames_fmt.  No device call is made.  Build and run
// from the repository root:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       tools/sanitize_frame_format.cpp densesurfelmapping_amd/csrc/dsm_api.hip densesurfelmapping_amd/csrc/dsm_kernels.hip \
//       -o /tmp/sanitize_frame_format && ASAN_OPTIONS=detect_leaks=0 /tmp/sanitize_frame_format
// (detect_leaks=0: the packing threads of the library are process-wide and live until exit)
#include "../densesurfelmapping_amd/csrc/dsm_frame_format.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) {                                                              \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c);       \
            return 1;                                                            \
        }                                                                        \
    } while (0)

int main() {
    dsm_frame_format f;
    dsm_frame_format_init(&f);
    dsm_fmt::Parsed p;
    CHECK(f.struct_size == sizeof f && dsm_fmt::parse(&f, &p) == nullptr && !p.color && !p.u16 && p.depth_elem == 4 && p.gray.ch == 1);
    // every rule of the descriptor
    CHECK(dsm_fmt::parse(nullptr, &p) != nullptr);
    for (int fmt = -2; fmt <= 6; fmt++) {
        dsm_frame_format g = f;
        g.image_format = fmt;
        const bool known = fmt >= 0 && fmt <= 4;
        CHECK((dsm_fmt::parse(&g, &p) == nullptr) == known);
        if (known) CHECK(p.gray.ch == dsm_fmt::image_channels(fmt) && p.color == (fmt != 0) && p.gray.swap == (fmt == DSM_IMAGE_BGR8 || fmt == DSM_IMAGE_BGRA8));
    }
    const int32_t presets[3][4] = {DSM_GRAY_OPENCV_14BIT, DSM_GRAY_OPENCV_15BIT, DSM_GRAY_PIL_L};
    for (const auto &w : presets) CHECK(!dsm_fmt::gray_weights_error(w[0], w[1], w[2], w[3]) && w[0] + w[1] + w[2] == 1 << w[3]);
    CHECK(dsm_fmt::gray_weights_error(-1, 1, 1, 8) && dsm_fmt::gray_weights_error(1, -1, 1, 8) && dsm_fmt::gray_weights_error(1, 1, -1, 8));
    CHECK(dsm_fmt::gray_weights_error(1, 1, 1, 0) && dsm_fmt::gray_weights_error(1, 1, 1, 23) && dsm_fmt::gray_weights_error(1, 1, 1, -5));
    CHECK(dsm_fmt::gray_weights_error(0x7fffffff, 0x7fffffff, 0x7fffffff, 22) && dsm_fmt::gray_weights_error(200, 50, 7, 8));
    CHECK(!dsm_fmt::gray_weights_error(1 << 22, 0, 0, 22) && !dsm_fmt::gray_weights_error(0, 0, 0, 1));
    {
        dsm_frame_format g = f;
        g.image_format = DSM_IMAGE_RGB8;
        g.struct_size = sizeof g - 4;
        CHECK(dsm_fmt::parse(&g, &p) != nullptr);
        g.struct_size = sizeof g;
        g.gray_shift = 23;
        CHECK(dsm_fmt::parse(&g, &p) != nullptr);
        g.gray_shift = 14;
        g.depth_format = 2;
        CHECK(dsm_fmt::parse(&g, &p) != nullptr);
        g.depth_format = DSM_DEPTH_U16;
        g.depth_scale = 0.0f;
        CHECK(dsm_fmt::parse(&g, &p) != nullptr);
        g.depth_scale = 5000.0f;
        g.depth_op = 2;
        CHECK(dsm_fmt::parse(&g, &p) != nullptr);
        g.depth_op = DSM_DEPTH_U16_MULTIPLY;
        CHECK(dsm_fmt::parse(&g, &p) == nullptr && p.color && p.u16 && p.depth_elem == 2 && p.depth_op == DSM_DEPTH_U16_MULTIPLY);
    }
    // dsm_host_pack_frames_fmt: every format, exact-size heap buffers (a byte read or written outside them is reported)
    const int n = 3, w = 37, h = 19, pitch = 64;
    for (int fmt = 0; fmt <= 4; fmt++)
        for (int u16 = 0; u16 <= 1; u16++) {
            dsm_frame_format g = f;
            g.image_format = fmt;
            g.depth_format = u16 ? DSM_DEPTH_U16 : DSM_DEPTH_F32;
            const size_t ch = (size_t)dsm_fmt::image_channels(fmt), de = u16 ? 2 : 4;
            std::vector<std::vector<uint8_t>> im((size_t)n), dp((size_t)n);
            std::vector<const void *> ip, dpp;
            std::vector<size_t> is, ds;
            for (int i = 0; i < n; i++) {
                const size_t si = (size_t)w * ch + (size_t)i, sd = (size_t)w * de + 2 * (size_t)i; // tight, then strided
                im[(size_t)i].resize(si * (h - 1) + (size_t)w * ch); // (the last row ends with its last pixel)
                dp[(size_t)i].resize(sd * (h - 1) + (size_t)w * de);
                for (size_t k = 0; k < im[(size_t)i].size(); k++) im[(size_t)i][k] = (uint8_t)(k * 7 + (size_t)i);
                for (size_t k = 0; k < dp[(size_t)i].size(); k++) dp[(size_t)i][k] = (uint8_t)(k * 13 + (size_t)i);
                ip.push_back(im[(size_t)i].data()); dpp.push_back(dp[(size_t)i].data());
                is.push_back(si); ds.push_back(sd);
            }
            const size_t ri = (size_t)pitch * ch, rd = (size_t)pitch * de;
            std::vector<uint8_t> di(ri * h * (n - 1) + ri * (h - 1) + (size_t)w * ch, 0xEE), dd(rd * h * (n - 1) + rd * (h - 1) + (size_t)w * de, 0xEE);
            CHECK(dsm_host_pack_frames_fmt(n, w, h, ip.data(), is.data(), dpp.data(), ds.data(), di.data(), ri, ri * h, dd.data(), rd, rd * h, &g) == DSM_OK);
            for (int i = 0; i < n; i++)
                for (int y = 0; y < h; y++) {
                    CHECK(!memcmp(di.data() + ri * h * (size_t)i + ri * (size_t)y, im[(size_t)i].data() + is[(size_t)i] * (size_t)y, (size_t)w * ch));
                    CHECK(!memcmp(dd.data() + rd * h * (size_t)i + rd * (size_t)y, dp[(size_t)i].data() + ds[(size_t)i] * (size_t)y, (size_t)w * de));
                    if (y + 1 < h || i + 1 < n) CHECK(di[ri * h * (size_t)i + ri * (size_t)y + (size_t)w * ch] == 0xEE && dd[rd * h * (size_t)i + rd * (size_t)y + (size_t)w * de] == 0xEE);
                }
            // refused before anything is copied
            CHECK(dsm_host_pack_frames_fmt(n, w, h, ip.data(), is.data(), dpp.data(), ds.data(), di.data(), (size_t)w * ch - 1, ri * h, dd.data(), rd, rd * h, &g) == DSM_E_INVALID);
            is[1] = (size_t)w * ch - 1;
            CHECK(dsm_host_pack_frames_fmt(n, w, h, ip.data(), is.data(), dpp.data(), ds.data(), di.data(), ri, ri * h, dd.data(), rd, rd * h, &g) == DSM_E_INVALID);
            CHECK(dsm_host_pack_frames_fmt(n, w, h, ip.data(), is.data(), dpp.data(), ds.data(), di.data(), ri, ri * h, dd.data(), rd, rd * h, nullptr) == DSM_E_INVALID);
        }
    dsm_frame_format bad = f;
    bad.image_format = 9;
    CHECK(dsm_host_pack_frames_fmt(1, w, h, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, 0, &bad) == DSM_E_INVALID);
    CHECK(dsm_host_pack_frames_fmt(1, w, h, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, 0, &f) == DSM_E_INVALID);
    dsm_frame_format_init(nullptr);
    puts("sanitize_frame_format: ok");
    return 0;
}
