// dsm_frame_copy.h -- how the planes of n frames get from a caller's layout into a destination's, as few transfers as the two
// layouts allow: plain host C++ with no device call, shared by every frame upload of the engine (dsm_api.hip, copy_planes) and
// by the host build that runs every plan with memcpy inside exact-size buffers (tests/frame_copy_host.cpp).
#ifndef DSM_FRAME_COPY_H
#define DSM_FRAME_COPY_H
#include <cstddef>

namespace dsm_copy {

// n planes of `rows` rows of `row_bytes` payload; all steps in bytes, the frame steps unused when n == 1
struct Planes {
    int n;
    size_t rows, row_bytes;
    size_t step, frame_step;         // the source's rows and frames
    size_t dst_step, dst_frame_step; // the destination's
    bool pack_tight; // whoever reads the destination takes any row and frame stride (the staging in front of a kernel)
};

struct Plan {
    int transfers;  // 1 or n
    bool two_d;     // a transfer is `rows` rows of `row_bytes`, src_step / dst_step apart; otherwise `bytes` in one piece
    size_t bytes, rows, row_bytes, src_step, dst_step;
    size_t src_advance, dst_advance; // from one transfer to the next
    bool packed;    // rule 2: the payload sits tight in the destination, not at the destination's own steps
    size_t out_step, out_frame_step; // where the rows and frames sit in the destination afterwards
};

// 1. rows at the destination's step and frames at its frame step: ONE transfer for all n (the bytes between rows and between
//    frames travel along; the last row ends with its payload);
// 2. (pack_tight) tight rows, frames back to back: one transfer, the payload stays tight;
// 3. anything else frame by frame: in one piece each if the rows are at the destination's step, else row by row (2-D).
inline Plan plan(const Planes &g) {
    const size_t plane = g.dst_step * (g.rows - 1) + g.row_bytes, tight = g.row_bytes * g.rows;
    Plan p = {1, false, 0, g.rows, g.row_bytes, g.step, g.dst_step, 0, 0, false, g.dst_step, g.dst_frame_step};
    if (g.step == g.dst_step && (g.n == 1 || g.frame_step == g.dst_frame_step)) {
        p.bytes = g.dst_frame_step * (size_t)(g.n - 1) + plane;
    } else if (g.pack_tight && g.step == g.row_bytes && (g.n == 1 || g.frame_step == tight)) {
        p.bytes = tight * (size_t)g.n;
        p.packed = true;
        p.out_step = g.row_bytes;
        p.out_frame_step = tight;
    } else {
        p.transfers = g.n;
        p.two_d = g.step != g.dst_step;
        p.bytes = p.two_d ? 0 : plane;
        p.src_advance = g.frame_step;
        p.dst_advance = g.dst_frame_step;
    }
    return p;
}

} // namespace dsm_copy
#endif /* DSM_FRAME_COPY_H */
