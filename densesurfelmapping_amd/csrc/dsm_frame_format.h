// dsm_frame_format.h -- dsm_frame_format (include/dsm.h) taken apart and checked: plain host C++ with no device call, shared by the
// engine's *_fmt entry points and by the stand-alone sanitizer program (tools/sanitize_frame_format.cpp).
#ifndef DSM_FRAME_FORMAT_H
#define DSM_FRAME_FORMAT_H
#include "../../include/dsm.h"

namespace dsm_fmt {

// a colour image format and its grey weights: grey = (R wr + G wg + B wb + (1 << (shift - 1))) >> shift
struct Gray {
    int ch;   // bytes per pixel, 3 or 4 (the fourth is alpha: ignored)
    int swap; // the first byte of a pixel is B
    int wr, wg, wb, shift;
};

// bytes per image pixel of a DSM_IMAGE_* format, 0 = unknown
inline int image_channels(int image_format) {
    switch (image_format) {
    case DSM_IMAGE_MONO8: return 1;
    case DSM_IMAGE_RGB8:
    case DSM_IMAGE_BGR8: return 3;
    case DSM_IMAGE_RGBA8:
    case DSM_IMAGE_BGRA8: return 4;
    default: return 0;
    }
}

// the rules of the weights (include/dsm.h): nullptr = fine, else what is wrong
inline const char *gray_weights_error(int wr, int wg, int wb, int shift) {
    if (wr < 0 || wg < 0 || wb < 0) return "negative grey weight";
    if (shift < 1 || shift > 22) return "gray_shift outside [1, 22]";
    if ((long long)wr + (long long)wg + (long long)wb > (1ll << shift)) return "grey weights add up to more than 1 << gray_shift";
    return nullptr;
}

inline bool depth_scale_ok(float scale, int op) {
    return scale > 0.0f && scale <= 3.402823466e38f && (op == DSM_DEPTH_U16_DIVIDE || op == DSM_DEPTH_U16_MULTIPLY); // (false for NaN)
}

struct Parsed {
    bool color = false, u16 = false;
    Gray gray = {1, 0, 0, 0, 0, 1};
    float depth_scale = 1.0f;
    int depth_op = DSM_DEPTH_U16_DIVIDE;
    int depth_elem = 4; // bytes per depth pixel
};

// nullptr = fine (out filled), else what is wrong with the descriptor
inline const char *parse(const dsm_frame_format *f, Parsed *out) {
    if (!f) return "null dsm_frame_format";
    if (f->struct_size != (uint32_t)sizeof(dsm_frame_format)) return "dsm_frame_format.struct_size is not sizeof(dsm_frame_format)";
    const int ch = image_channels(f->image_format);
    if (!ch) return "unknown image_format";
    if (f->depth_format != DSM_DEPTH_F32 && f->depth_format != DSM_DEPTH_U16) return "unknown depth_format";
    Parsed p;
    if (ch > 1) {
        if (const char *e = gray_weights_error(f->gray_wr, f->gray_wg, f->gray_wb, f->gray_shift)) return e;
        p.color = true;
        p.gray = {ch, f->image_format == DSM_IMAGE_BGR8 || f->image_format == DSM_IMAGE_BGRA8, f->gray_wr, f->gray_wg, f->gray_wb, f->gray_shift};
    }
    if (f->depth_format == DSM_DEPTH_U16) {
        if (!depth_scale_ok(f->depth_scale, f->depth_op))
            return "depth_scale must be finite and > 0, depth_op DSM_DEPTH_U16_DIVIDE or DSM_DEPTH_U16_MULTIPLY";
        p.u16 = true;
        p.depth_scale = f->depth_scale;
        p.depth_op = f->depth_op;
        p.depth_elem = 2;
    }
    *out = p;
    return nullptr;
}

} // namespace dsm_fmt
#endif /* DSM_FRAME_FORMAT_H */
