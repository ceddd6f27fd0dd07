"""window_pixel (csrc/dsm_math.h), the depth-inlier predicate behind the fit's row masks, on the host against the reference's
own statements spelled out (FF.cpp:816-818 member, 826-827 depth, 846-850 residual against HUBER_RANGE in double): all sixteen
combinations of (row in the image, column in the image, labelled with the seed, depth above 0.05), with the depths and the
residuals at the thresholds and the floats on either side of them."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_lib = None


def host_lib():
    global _lib
    if _lib is None:
        out = os.path.join(ROOT, "tests", "_build", "libfit_masks_host.so")
        src = os.path.join(ROOT, "tests", "fit_masks_host.cpp")
        deps = [src, os.path.join(ROOT, "densesurfelmapping_amd", "csrc", "dsm_math.h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            os.makedirs(os.path.dirname(out), exist_ok=True)
            subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", out + ".tmp"], check=True)
            os.replace(out + ".tmp", out)
        lib = C.CDLL(out)
        lib.fit_masks_window_pixel.argtypes = [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_double]
        lib.fit_masks_window_pixel.restype = C.c_int
        for f in (lib.fit_masks_flt_below, lib.fit_masks_flt_above):
            f.argtypes, f.restype = [C.c_double], C.c_float
        _lib = lib
    return _lib


def reference(row_in, col_in, label_is_seed, d, mean_depth, huber):
    """(member, has depth, inlier) as FF.cpp states them: a float against a double literal compares in double"""
    member = bool(row_in and col_in and label_is_seed)          # FF.cpp:816-818
    has_depth = member and float(np.float32(d)) > 0.05           # FF.cpp:826-827
    with np.errstate(invalid="ignore", over="ignore"):
        residual = float(np.float32(mean_depth) - np.float32(d))  # FF.cpp:849, a float
    inlier = has_depth and residual < huber and residual > -huber  # FF.cpp:850
    return member, has_depth, inlier


def neighbours(x):
    x = np.float32(x)
    return [np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))]


HUBERS = [0.4, 0.05, 0.5]  # the reference's HUBER_RANGE, its commented-out alternative, and a value that IS a float


def test_float_neighbours_of_the_thresholds():
    lib = host_lib()
    for c in [0.05] + HUBERS:
        lo, hi = np.float32(lib.fit_masks_flt_below(c)), np.float32(lib.fit_masks_flt_above(c))
        assert float(lo) <= c <= float(hi)
        assert hi == lo if float(np.float32(c)) == c else hi == np.nextafter(lo, np.float32(np.inf))


@pytest.mark.parametrize("huber", HUBERS)
def test_window_pixel_against_the_reference_statements(huber):
    lib = host_lib()
    below, above = lib.fit_masks_flt_below(0.05), lib.fit_masks_flt_above(0.05)
    # depths: at and around the 0.05 threshold (both sides of the double literal), zero, negative, ordinary, non-finite
    around = sorted({float(v) for b in (below, above) for v in neighbours(b)})
    assert float(below) <= 0.05 < float(above) and len(around) >= 4
    depth_lo = [v for v in around if not v > 0.05] + [0.0, -1.0, 0.01, float("-inf")]
    depth_hi = [v for v in around if v > 0.05] + [0.0625, 1.0, 4.0, 37.5, float("inf")]
    seen = set()
    n = 0
    for row_in, col_in, lab, deep in itertools.product((0, 1), repeat=4):
        for d in (depth_hi if deep else depth_lo) + [float("nan")]:
            # mean depths that put the residual at +-huber and one float to either side, besides ordinary ones
            mds = [0.0, 1.0, 4.0, float("nan"), float("inf")]
            if np.isfinite(d):
                for sign in (1.0, -1.0):
                    for hb in (lib.fit_masks_flt_below(huber), lib.fit_masks_flt_above(huber)):
                        mds += [float(v) for v in neighbours(np.float32(d) + np.float32(sign * hb))]
            for md in mds:
                want = reference(row_in, col_in, lab, d, md, huber)
                got = lib.fit_masks_window_pixel(row_in, col_in, lab, d, md, huber)
                assert got == want[0] | want[1] << 1 | want[2] << 2, (row_in, col_in, lab, d, md, huber, got, want)
                if not np.isnan(d):
                    assert want[1] == bool(row_in and col_in and lab and deep), (d, deep)
                seen.add((row_in, col_in, lab, deep, want[2]))
                n += 1
    # all sixteen combinations were walked, and the only one that can hold an inlier held inliers and non-inliers
    assert {s[:4] for s in seen} == set(itertools.product((0, 1), repeat=4))
    assert {s[4] for s in seen if s[:4] == (1, 1, 1, 1)} == {False, True}
    assert not any(s[4] for s in seen if s[:4] != (1, 1, 1, 1))
    assert n > 1000
