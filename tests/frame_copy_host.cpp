// frame_copy_host.cpp -- every plan of csrc/dsm_frame_copy.h carried out with memcpy between buffers of EXACTLY the extents the
// geometry implies: a byte count that is one too large is a range error here, not a read past a caller's frame on the device.
// tests/test_cpu_frame_copy.py loads it as a library.  The same file is a stand-alone program for the sanitizers (never loaded
// into Python that way); from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -DFRAME_COPY_MAIN tests/frame_copy_host.cpp ...
//       ... -o /tmp/frame_copy_host && /tmp/frame_copy_host
#include "../densesurfelmapping_amd/csrc/dsm_frame_copy.h"

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#define CHECK(c)                  \
    do {                          \
        if (!(c)) return __LINE__; \
    } while (0)

// 0 and out = {transfers, two_d, packed, out_step, out_frame_step}, or the line of the check that failed
extern "C" int frame_copy_host_run(int n, size_t rows, size_t row_bytes, size_t step, size_t frame_step, size_t dst_step, size_t dst_frame_step,
                                   int pack_tight, int64_t *out) {
    const dsm_copy::Plan p = dsm_copy::plan({n, rows, row_bytes, step, frame_step, dst_step, dst_frame_step, pack_tight != 0});
    const size_t n1 = (size_t)(n - 1);
    const uint8_t kGap = 0xEE;
    std::vector<uint8_t> src(frame_step * n1 + step * (rows - 1) + row_bytes), dst(p.out_frame_step * n1 + p.out_step * (rows - 1) + row_bytes, kGap);
    for (size_t k = 0; k < src.size(); k++) src[k] = (uint8_t)(k * 131 + (k >> 8) * 7 + 1);
    CHECK(p.transfers == 1 || p.transfers == n);
    for (size_t i = 0; i < (size_t)p.transfers; i++) {
        const size_t s = i * p.src_advance, d = i * p.dst_advance;
        if (p.two_d) {
            CHECK(p.rows == rows && p.row_bytes == row_bytes);
            for (size_t r = 0; r < p.rows; r++) {
                CHECK(s + r * p.src_step + p.row_bytes <= src.size() && d + r * p.dst_step + p.row_bytes <= dst.size());
                memcpy(dst.data() + d + r * p.dst_step, src.data() + s + r * p.src_step, p.row_bytes);
            }
        } else {
            CHECK(p.bytes > 0 && s + p.bytes <= src.size() && d + p.bytes <= dst.size());
            memcpy(dst.data() + d, src.data() + s, p.bytes);
        }
    }
    // every payload row where the plan says it is, equal to its source row
    std::vector<uint8_t> payload(dst.size(), 0);
    for (size_t f = 0; f < (size_t)n; f++)
        for (size_t r = 0; r < rows; r++) {
            const size_t d = f * p.out_frame_step + r * p.out_step;
            CHECK(d + row_bytes <= dst.size());
            CHECK(!memcmp(dst.data() + d, src.data() + f * frame_step + r * step, row_bytes));
            memset(payload.data() + d, 1, row_bytes);
        }
    // row by row: nothing between the rows or between the frames was written; frame by frame in one piece each: nothing between
    // a frame's last payload byte and the next frame
    if (p.two_d)
        for (size_t k = 0; k < dst.size(); k++) CHECK(payload[k] || dst[k] == kGap);
    else if (p.transfers > 1)
        for (size_t f = 0; f + 1 < (size_t)n; f++)
            for (size_t k = f * p.out_frame_step + p.out_step * (rows - 1) + row_bytes; k < (f + 1) * p.out_frame_step; k++) CHECK(dst[k] == kGap);
    out[0] = p.transfers; out[1] = p.two_d; out[2] = p.packed; out[3] = (int64_t)p.out_step; out[4] = (int64_t)p.out_frame_step;
    return 0;
}

#ifdef FRAME_COPY_MAIN
int main() {
    int cases = 0;
    for (size_t w : {1, 25, 64, 250})
        for (size_t e = 1; e <= 4; e++)
            for (size_t rows : {1, 2, 19})
                for (int n : {1, 2, 5})
                    for (int pack = 0; pack <= 1; pack++) {
                        const size_t row_bytes = w * e, dst_step = (w + 63) / 64 * 64 * e;
                        for (size_t step : {dst_step, row_bytes, row_bytes + 1, dst_step + e})
                            for (size_t frame_step : {step * rows, dst_step * rows, step * rows + 3}) {
                                int64_t out[5];
                                const int line = frame_copy_host_run(n, rows, row_bytes, step, frame_step, dst_step, dst_step * rows, pack, out);
                                if (line) {
                                    fprintf(stderr, "frame_copy_host.cpp:%d failed: n %d rows %zu row_bytes %zu step %zu frame_step %zu dst_step %zu pack %d\n", line, n, rows,
                                            row_bytes, step, frame_step, dst_step, pack);
                                    return 1;
                                }
                                cases++;
                            }
                    }
    printf("frame_copy_host: %d plans ok\n", cases);
    return 0;
}
#endif
