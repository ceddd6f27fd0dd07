// window_pixel of csrc/dsm_math.h compiled for the host: the one statement of the depth-inlier predicate that k_seed_stats publishes
// as row masks and that k_seed_points and the fit behind it evaluate themselves (tests/test_cpu_fit_masks.py).
#include "../densesurfelmapping_amd/csrc/dsm_math.h"

extern "C" {
// bit 0 = member, bit 1 = has depth, bit 2 = depth inlier; the Huber range as the kernels hand it over (flt_above of the double)
int fit_masks_window_pixel(int row_in, int col_in, int label_is_seed, float d, float mean_depth, double huber) {
    const dsm::WindowPixel p = dsm::window_pixel(row_in != 0, col_in != 0, label_is_seed != 0, d, mean_depth, dsm::flt_above(huber));
    return (p.member ? 1 : 0) | (p.has_depth ? 2 : 0) | (p.inlier ? 4 : 0);
}
float fit_masks_flt_below(double c) { return dsm::flt_below(c); }
float fit_masks_flt_above(double c) { return dsm::flt_above(c); }
}
