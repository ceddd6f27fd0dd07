"""Crafted frames for the plane path: depth images whose pixels sit ON the decision margins that k_pixel_normals,
k_seed_points / k_seed_stats, k_seed_fit, k_seed_finish, k_frame_tail and the robust mean of k_update_seeds restate from the
reference -- built from numpy and the ORACLE alone (oracle/bindings.py, PortOracle), never from the product.

The device.  Every 8x8 cell gets one of four grey levels in a 2x2 tiling (10, 95 / 180, 250).  A neighbour's intensity term
(85^2 / 100 at the least) outweighs every distance and depth term, so the label image after the three sweeps IS the cell grid
(on a ragged camera: the grid extended to the border pixels that have a candidate cell, -1 beyond), whatever the depths are.
Each superpixel is then its own pixels, and the depth of each is ours to choose.

Families (frames(ob, cam, family, huber) -> VARIANTS frames; a variant changes the pixel order inside the cells, the
assignment of cases to cells and the grey tiling's phase):

  valid    every depth the float just below 0.05 (FF.cpp:827 is `depth > 0.05`, a float against a double: float(0.05) > 0.05);
           k = 14..18 pixels per cell on a float above it.  valid_depth_num < 16 (FF.cpp:841) on both sides.
  ratio    m pixels at 4 m, n - m at 5.5 m, the rest 0, for RATIO_PAIRS: inlier_num / size < 0.8 (FF.cpp:862), a float quotient
           against a double -- 16/20, 32/40 and 48/60 are 0.8f > 0.8 and fitted.
  huber    per cell a wall at 4.00..4.06 m and eight pixels on consecutive floats centred on mean_depth + huber (even cells) or
           - huber (odd cells): |mean_depth - d| against HUBER_RANGE (FF.cpp:540, 850).  mean_depth is the seed's value after
           the sweeps, read from the oracle: the lattice is placed, the oracle run, the lattice placed again (HUBER_PASSES).
           With the wall and the lattice alone the estimator of FF.cpp:530-556 stops at its first iterate, where the lattice
           itself straddles the range: a pixel changing sides moves the mean by 3e-3, a thousand lattice widths, and only
           57..77 of 240 cells settled.  Four more pixels per cell at wall + 5 * huber (tail members at every iterate) make the
           estimator take steps of its own; the lattice is then on one side at every iterate it classifies, the mean is a
           contraction of the lattice's place (1 / 8 per pass), and all 240 cells settle.
  classes  a wall at 30 / 30 / 20 / 12 m with +-0.35 m of noise per pixel: the pixel normals are noise, the first plane is far
           off, and residuals of the Gauss-Newton steps fall in all three Huber classes (FF.cpp:134-170) and change class.
  view     depth = 1 + slope * (x - cell centre), slopes 0.02..0.1 per pixel over the cells: view_cos on both sides of
           MAX_ANGLE_COS (FF.cpp:329).
  wall01   five consecutive floats round 0.1: pixels in (0.05, 0.1] are plane members that the mean-depth list (FF.cpp:508)
           and the pixel normals leave out.
  wall001  five consecutive floats round 0.01 (seed initialisation, FF.cpp:600-613, and the pick's inverse depth): every seed
           ends with mean depth 0 -- the pick without its depth term, no plane, no surfel.
  lengths  m inliers per cell on a slightly tilted 4 m wall, the rest 0, m on both sides of every multiple of 8 (LIST_LENGTHS)
           and 0, dealt out so that four consecutive seeds hold long, short and empty lists; on a ragged camera the border
           cells own up to 144 pixels and take the longer lists of RAGGED_LENGTHS.
  tiny     seven rows or columns per cell on a 4 m wall with +-0.01 m of noise, one pixel placed where its centred coordinate
           is the smallest non-zero float: the exactness test of k_seed_fit's free-order Jacobian sums (dsm_math.h,
           gn_sum_is_exact) fails and the ordered sums run.
  edge     a flat wall whose first plane is exactly z = list mean, and eight pixels per cell whose first Gauss-Newton residual
           is the float below HUBER_RANGE or one of its neighbours (see _edge): the class test of FF.cpp:134 on the one
           float where `<` against the double differs from `<` against the float below it.

census(...) counts, in the oracle's own state, how many seeds or pixels sit on each side of the margin a family is for; the
labels and the seed table are read after the sweeps (mean_depth there is the value the fit tests against; FF.cpp:910 overwrites
it) and again after calculate_norms.  check_census() holds the conditions the tests assert before they compare anything.

Measured with PortOracle and tests/hostemu.cpp at 160x96 (S = 240), per variant 0..3 (MEASURED holds the least):
  valid    cells with n = 14 / 15 / 16 / 17 / 18: 48 each; fitted 0 / 0 / 48 / 48 / 48 (the same at 166x103)
  ratio    24 cells per pair; fitted 24 of 24 where m / n >= 0.8f (16/20, 32/40, 48/60 among them), 0 of 24 else
  huber    cells with lattice pixels within 1e-6 of the range on both sides: 240 of 240 at 0.4, 0.05 and 0.5
  classes  seeds with a non-core residual at step 1: 171 / 172 / 166 / 140 of 240; every one of them changes class later
  view     fitted seeds with view_cos < 0.1: 68 / 49 / 65 / 49, >= 0.1: 150 / 150 / 152 / 150 (22 / 41 / 23 / 41 fit NaN planes);
           new surfels 172 / 191 / 175 / 191 of 240 fitted
  wall01   240 cells whose plane-member and mean-depth-list counts differ, 240 new surfels
  wall001  240 seeds with mean depth 0, no plane, no surfel
  lengths  208 fitted seeds; the longest inlier list is 64 (at 166x103: 144 / 121 / 120 / 143, the corner cell's)
  edge     seeds with a first residual ON the float below the range: 0 / 240 / 0 / 240 at 0.4 (on the next float up: 240 / 0 /
           240 / 0), 240 / 0 / 240 / 0 at 0.05, 240 in every variant at 0.5 (which is that float)
  steps 2..5 that keep a non-empty class mask (the cached inverse stands after the mask comparison), huber family at 0.05:
           824 / 463 / 182 / 774; on the valid family 576 (its planes are NaN: depths under 0.1 have no pixel normal)
  steps 2..5 that fail the exactness test and take the ordered sums, tiny family: 82 / 69 / 86 / 78 (0 to 3 elsewhere)
"""
import numpy as np

from eigen33_cases import tilt
from fit_mask_cases import has_plane

F32 = np.float32
CELL = 8
GREYS = (10, 95, 180, 250)
VARIANTS = 4
HUBERS = (0.4, 0.05, 0.5)  # test_cpu_fit_masks.HUBERS: the reference's range, its commented-out alternative, one that IS a float
HUBER_PASSES = 12
LATTICE = 8
FAR_PIXELS = 4
ANGLE_COS = 0.1
RATIO_PAIRS = ((64, 51), (64, 52), (20, 15), (20, 16), (40, 31), (40, 32), (16, 12), (16, 13), (60, 47), (60, 48))
LIST_LENGTHS = (13, 16, 17, 23, 24, 25, 31, 32, 33, 47, 48, 49, 63, 64)
RAGGED_LENGTHS = (65, 71, 72, 73, 95, 96, 97, 119, 120, 121, 143, 144)  # for cells that own more than 64 pixels
CORNER_LENGTHS = (144, 121, 120, 143)
CLASS_WALLS = (30.0, 30.0, 20.0, 12.0)
FAMILIES = ("valid", "ratio", "huber", "classes", "view", "wall01", "wall001", "lengths", "tiny", "edge")
HUBER_FAMILIES = ("huber", "edge")  # the families whose frames depend on the Huber range


def batch_families(second=False):
    """one family per handle of a batch of eight; the second set has `edge` and `tiny` in place of the two walls"""
    return tuple({"wall01": "edge", "wall001": "tiny"}.get(f, f) if second else f for f in FAMILIES[:8])


POSE = tilt(np.eye(4))

# what the recipes gave when they were written: the least over the variants (view's `new`: the most)
MEASURED = {
    "huber_lattice_cells": {0.4: 240, 0.05: 240, 0.5: 240},
    "first_noncore": 140, "seeds_mask_changed": 140,   # classes family, per frame
    "reuse_nonempty": 182,                              # huber family at 0.05, per frame
    "ordered_after_test": 69,                           # tiny family, per frame
    "view": {"below": 49, "above": 150, "new": 191, "fitted": 240},
    "longest_list": {(160, 96): 64, (166, 103): 144},
    "edge_on_float_below": {0.4: 480, 0.05: 480, 0.5: 960},  # seeds, over the four variants
}


def constants_of(huber):
    """the stereo set (fusion_functions.h:13-16) with another HUBER_RANGE; None for the set the camera selects by itself"""
    return None if huber == 0.4 else (huber, 0.5, 4.0, 0.1)


def flt_below(c):
    f = F32(c)
    return f if float(f) <= c else np.nextafter(f, F32(-np.inf))


def flt_above(c):
    f = F32(c)
    return f if float(f) >= c else np.nextafter(f, F32(np.inf))


def steps(x, k):
    """the floats k steps above x > 0 (k an integer array, may be negative)"""
    return (np.asarray(x, F32).view(np.int32) + np.asarray(k, np.int32)).view(F32)


def grid(cam):
    return cam.width // CELL, cam.height // CELL


def expected_labels(cam):
    """the cell grid, extended to the border pixels that have a candidate cell (dsm_math.h has_candidate_cell), -1 beyond"""
    gw, gh = grid(cam)
    y, x = np.mgrid[0:cam.height, 0:cam.width]
    lab = np.minimum(y // CELL, gh - 1) * gw + np.minimum(x // CELL, gw - 1)
    return np.where((x < gw * CELL + CELL // 2) & (y < gh * CELL + CELL // 2), lab, -1).astype(np.int32)


def image(cam, v=0):
    gw, gh = grid(cam)
    y, x = np.mgrid[0:cam.height, 0:cam.width]
    gx, gy = np.minimum(x // CELL, gw - 1), np.minimum(y // CELL, gh - 1)
    return np.asarray(np.roll(GREYS, v), np.uint8)[(gy % 2) * 2 + gx % 2]


def _orders(cam, v):
    """per cell the flat indices of its pixels: row-major, reversed, column-major, or shuffled (by variant)"""
    lab = expected_labels(cam).ravel()
    S = grid(cam)[0] * grid(cam)[1]
    rng = np.random.default_rng(1000 + v)
    out = []
    for s in range(S):
        idx = np.flatnonzero(lab == s)
        if v % 4 == 1:
            idx = idx[::-1]
        elif v % 4 == 2:
            idx = idx[np.lexsort((idx // cam.width, idx % cam.width))]
        elif v % 4 == 3:
            idx = rng.permutation(idx)
        out.append(idx)
    return out


def _cells(cam):
    gw, gh = grid(cam)
    y, x = np.mgrid[0:cam.height, 0:cam.width]
    return x, y, np.minimum(x // CELL, gw - 1), np.minimum(y // CELL, gh - 1)


def _valid(cam, v):
    dep = np.full(cam.width * cam.height, flt_below(0.05), F32)
    for s, idx in enumerate(_orders(cam, v)):
        k = 14 + (s + v) % 5
        dep[idx[:k]] = steps(flt_above(0.05), (np.arange(k) + v) % 3)
    return dep


def _ratio(cam, v):
    dep = np.zeros(cam.width * cam.height, F32)
    for s, idx in enumerate(_orders(cam, v)):
        n, m = RATIO_PAIRS[(s + v) % len(RATIO_PAIRS)]
        dep[idx[:m]] = 4.0
        dep[idx[m:n]] = 5.5
    return dep


def _classes(cam, v):
    rng = np.random.default_rng(2000 + v)
    return (CLASS_WALLS[v % 4] + rng.uniform(-0.35, 0.35, cam.width * cam.height)).astype(F32)


def _tiny(cam, v):
    """seven rows (even variants) or columns (odd) of every cell on a 4 m wall with +-0.01 m of noise, the rest 0; one pixel of
    the middle row (column) moved to the depth where its centred y (x) coordinate -- FF.cpp:94-96 and 121-126 in float32,
    restated here sum by sum -- is the smallest non-zero float it can be: a Jacobian term ~2^-27 of its neighbours'"""
    rng = np.random.default_rng(4000 + v)
    gw, gh = grid(cam)
    w = cam.width
    wall = (4.0 + rng.uniform(-0.01, 0.01, w * cam.height)).astype(F32)
    dep = np.zeros(w * cam.height, F32)
    first = (v // 2) % 2
    c0, f = (F32(cam.cx), F32(cam.fx)) if v % 2 else (F32(cam.cy), F32(cam.fy))
    for s in range(gw * gh):
        x0, y0 = (s % gw) * CELL, (s // gw) * CELL
        yy, xx = np.mgrid[y0:y0 + CELL, x0:x0 + CELL]
        along, across = (yy - y0, xx - x0) if v % 2 else (xx - x0, yy - y0)
        keep = (across >= first) & (across < first + 7)
        idx = (yy * w + xx)[keep]                                  # row-major: the order the reference sums in
        dep[idx] = wall[idx]
        i0 = int(np.flatnonzero((across[keep] == first + 3) & (along[keep] == s % CELL))[0])
        ray = ((xx if v % 2 else yy)[keep].astype(F32) - c0) / f
        if ray[i0] == 0:
            continue
        best = None
        guess = F32(np.mean((ray * dep[idx]).astype(np.float64)) / np.float64(ray[i0]))
        for d in steps(guess, np.arange(-48, 49)):
            dd = dep[idx].copy()
            dd[i0] = d
            coord = ray * dd
            p = coord[i0] - np.cumsum(coord, dtype=F32)[-1] / F32(len(idx))
            if p != 0 and (best is None or abs(p) < best[0]):
                best = (abs(p), d)
        if best is not None and abs(float(best[1]) - 4.0) < 0.05:
            dep[idx[i0]] = best[1]
    return dep


EDGE_WALL = {0.4: (0.40, 0.09), 0.05: (0.11, 0.07), 0.5: (0.45, 0.09)}  # (wall, low pixels) per Huber range


def edge_mean(dep, idx):
    """the mean depth of a fitted list as FF.cpp:121-126 takes it: a float sum in window order, divided by the count"""
    idx = np.sort(idx)
    return np.cumsum(dep[idx], dtype=F32)[-1] / F32(len(idx))


def _edge(cam, v, huber):
    """The Huber class test of the fit's FIRST step on the float below the range.  One flat wall for the whole frame: every
    pixel normal it leaves is (0, 0, 1) exactly, so the first plane is z = list mean and a point's first residual is its
    depth minus that mean, an exact float difference.  Per cell the last column and row lie in (0.05, 0.1] -- members of the
    list that the mean-depth estimator leaves out (in every cell alike, the border cells with their clipped windows
    included), so the list's mean sits below the seed's mean depth and every pixel stays a depth inlier -- and eight pixels
    lie on consecutive floats about list mean + huber.  The depths are small enough for the float below the range to be a
    reachable difference; at such depths the pick's inverse-depth term outweighs the intensities, and the labels stay on
    the grid only because every seed has the same mean depth (the same layout in every cell)."""
    wall, low = EDGE_WALL[huber]
    wall = F32(wall * (1.0 + 0.002 * v))
    w = cam.width
    dep = np.full(w * cam.height, wall, F32)
    lab = expected_labels(cam).ravel()
    x, y, gx, gy = _cells(cam)
    dep[((x % CELL == CELL - 1) | (y % CELL == CELL - 1)).ravel()] = F32(low)
    gw, gh = grid(cam)
    for s in range(gw * gh):
        x0, y0 = (s % gw) * CELL, (s // gw) * CELL
        # (no lattice pixel has a lattice pixel to its right AND below: its normal would be a slightly tilted one)
        lat = np.array([(y0 + v) * w + x0 + c for c in range(6)] + [(y0 + v + 2) * w + x0, (y0 + v + 2) * w + x0 + 2])
        idx = np.flatnonzero(lab == s)
        dep[lat] = F32(wall + huber)
        for _ in range(64):  # (the list mean follows the lattice by an eighth: until it stands)
            was = dep[lat].copy()
            dep[lat] = steps(F32(edge_mean(dep, idx) + flt_below(huber)), np.arange(LATTICE) - LATTICE // 2)
            if np.array_equal(was, dep[lat]):
                break
    return dep


def _view(cam, v):
    gw, gh = grid(cam)
    S = gw * gh
    x, y, gx, gy = _cells(cam)
    s = gy * gw + gx
    slope = 0.02 + 0.08 * ((s * 37 + v * 11) % S) / (S - 1)
    dep = 1.0 + (-1.0 if v % 2 else 1.0) * slope * (x - (gx * CELL + 3.5))
    return np.where(expected_labels(cam) >= 0, dep, 0.0).astype(F32).ravel()


def _wall(cam, v, c):
    y, x = np.mgrid[0:cam.height, 0:cam.width]
    return steps(F32(c), (x * 3 + y * 5 + v) % 5 - 2).ravel()


def list_lengths(cam, v):
    """per cell the number of inliers the `lengths` family gives it"""
    values = (0,) + LIST_LENGTHS
    out = []
    for s, idx in enumerate(_orders(cam, 0)):
        m = values[(s * 7 + v) % len(values)]
        if len(idx) > 64:
            m = RAGGED_LENGTHS[(s + v) % len(RAGGED_LENGTHS)]
        if len(idx) > 120:  # the corner cell of a ragged camera: on both sides of kFitSmallCap (csrc/dsm_device.h) = 120
            m = CORNER_LENGTHS[v % 4]
        out.append(min(m, len(idx)))
    return out


def _lengths(cam, v):
    rng = np.random.default_rng(3000 + v)
    x, y, gx, gy = _cells(cam)
    wall = 4.0 + 0.004 * (x - (gx * CELL + 3.5)) + 0.002 * (y - (gy * CELL + 3.5)) + rng.uniform(-0.001, 0.001, x.shape)
    wall = wall.astype(F32).ravel()
    dep = np.zeros(cam.width * cam.height, F32)
    for idx, m in zip(_orders(cam, v), list_lengths(cam, v)):
        dep[idx[:m]] = wall[idx[:m]]
    return dep


def prefit_state(ob, cam, img, dep, huber=0.4):
    """(labels, seed table after the sweeps, seed table after calculate_norms) of one frame, stage by stage (FF.cpp:960-975)"""
    orc = ob.PortOracle(cam, constants=constants_of(huber))
    try:
        orc.set_frame(img, dep)
        orc.stage("initialize_seeds")
        for _ in range(3):
            orc.stage("update_pixels")
            orc.stage("update_seeds")
        lab, pre = orc.labels().copy(), orc.seeds().copy()
        orc.stage("calculate_norms")
        return lab, pre, orc.seeds().copy(), orc.norm_map().copy()
    finally:
        orc.close()


def _huber(ob, cam, v, huber):
    gw, gh = grid(cam)
    S = gw * gh
    orders = _orders(cam, v)
    img = image(cam, v)
    x, y, gx, gy = _cells(cam)
    s = gy * gw + gx
    dep = (4.0 + 0.06 * ((s * 7 + v * 3) % 16) / 15.0).astype(F32).ravel()
    for c in range(S):  # the far pixels: tail members of the robust mean at every iterate, so that it takes steps of its own
        dep[orders[c][LATTICE:LATTICE + FAR_PIXELS]] += F32(5 * huber)
    md = np.array([dep[orders[c][-1]] for c in range(S)], F32)
    for _ in range(HUBER_PASSES):
        for c in range(S):
            centre = F32(md[c] + F32(huber if c % 2 == 0 else -huber))
            dep[orders[c][:LATTICE]] = steps(centre, np.arange(LATTICE) - LATTICE // 2)
        md = prefit_state(ob, cam, img, np.ascontiguousarray(dep.reshape(cam.height, cam.width)), huber)[1]["mean_depth"]
    return dep


_CACHE = {}


def frames(ob, cam, family, huber=0.4):
    """[(image, depth)] * VARIANTS of a family; only `huber` depends on the Huber range (and asks the oracle)"""
    key = (cam, family, huber if family in HUBER_FAMILIES else None)
    if key not in _CACHE:
        out = []
        for v in range(VARIANTS):
            dep = {"valid": _valid, "ratio": _ratio, "classes": _classes, "view": _view, "lengths": _lengths, "tiny": _tiny,
                   "wall01": lambda c, w: _wall(c, w, 0.1), "wall001": lambda c, w: _wall(c, w, 0.01),
                   "huber": lambda c, w: _huber(ob, c, w, huber), "edge": lambda c, w: _edge(c, w, huber)}[family](cam, v)
            dep = np.ascontiguousarray(dep.reshape(cam.height, cam.width), F32)
            assert np.isfinite(dep).all() and dep.min() >= 0 and dep.max() < 1e5  # on the sensor side of the 1e6 sentinel
            out.append((image(cam, v), dep))
        _CACHE[key] = out
    return _CACHE[key]


# ----------------------------------------------------------------------------------------------------------------------
# the census: FF.cpp's statements in numpy over the oracle's labels and seed tables

def counts(cam, lab, dep, pre, huber):
    """per seed: plane members (label), members with depth > 0.05 (n), inliers of the pre-fit mean depth among them (m), the
    mean-depth list of the last update_seeds (depth > 0.1 inside the window clipped to w - 1, h - 1: FF.cpp:476-513)"""
    S = len(pre)
    lab1, d = lab.astype(np.int64).ravel(), dep.astype(F32).ravel()
    member = lab1 >= 0
    md = pre["mean_depth"].astype(F32)[np.where(member, lab1, 0)]
    has_depth = member & (d.astype(np.float64) > 0.05)
    r = (md - d).astype(F32).astype(np.float64)
    inlier = has_depth & (r < huber) & (r > -huber)
    y, x = np.mgrid[0:cam.height, 0:cam.width]
    in_mean = member & (d.astype(np.float64) > 0.1) & (x.ravel() < cam.width - 1) & (y.ravel() < cam.height - 1)
    cnt = lambda mask: np.bincount(lab1[mask], minlength=S)
    return cnt(member), cnt(has_depth), cnt(inlier), cnt(in_mean), r.astype(np.float64), inlier


def census(ob, cam, family, v, huber=0.4):
    """dict of the counts the family is for (see check_census), from PortOracle's state alone"""
    img, dep = frames(ob, cam, family, huber)[v]
    lab, pre, post, nmap = prefit_state(ob, cam, img, dep, huber)
    members, n, m, n_mean, r, inlier = counts(cam, lab, dep, pre, huber)
    fitted = has_plane(post)
    with np.errstate(invalid="ignore", divide="ignore"):
        quotient = (m.astype(F32) / n.astype(F32)).astype(np.float64)
    out = {"labels_on_grid": bool(np.array_equal(lab, expected_labels(cam))),
           "labels_below_zero": int(((lab < 0) & (expected_labels(cam) >= 0)).sum()),
           "n": n, "m": m, "fitted": fitted, "predicted": (n >= 16) & ~(quotient < 0.8),
           "longest_list": int(np.where(fitted, m, 0).max()), "pre": pre, "post": post}
    if family == "huber":
        orders = _orders(cam, v)
        both = 0
        for c in range(len(pre)):
            rl, il = np.abs(r[orders[c][:LATTICE]]), inlier[orders[c][:LATTICE]]
            near = np.abs(rl - huber) <= 1e-6
            both += bool((near & il).any() and (near & ~il).any())
        out["lattice_cells"] = both
    if family == "edge":
        # seeds whose first plane is exactly z = list mean (every pixel normal of the list (0, 0, 1) or none) and whose list holds
        # a first residual ON the float below the range (core; with flt_below in the class test it would not be) / on the next
        # float up (the first outside the core)
        d1, nm = dep.ravel(), nmap.reshape(-1, 3)
        on_below = on_above = 0
        for c in range(len(pre)):
            idx = np.flatnonzero((lab.ravel() == c) & inlier)
            if not fitted[c] or not len(idx) or (nm[idx, :2] != 0).any() or not np.isin(nm[idx, 2], (0.0, 1.0)).all() or not nm[idx, 2].any():
                continue
            res = np.abs((d1[idx] - edge_mean(d1, idx)).astype(F32))
            on_below += bool((res == flt_below(huber)).any())
            on_above += bool((res == np.nextafter(flt_below(huber), F32(1))).any())
        out["on_float_below"], out["on_next_float"] = on_below, on_above
    if family == "view":
        vc = post["view_cos"]
        out["below"] = int((fitted & (vc < F32(ANGLE_COS))).sum())
        out["above"] = int((fitted & (vc >= F32(ANGLE_COS))).sum())
    if family in ("wall01", "wall001"):
        out["member_vs_mean_list"] = int((members != n_mean).sum())
        out["mean_depth_zero"] = int((pre["mean_depth"] == 0).sum())
    if family in ("view", "wall01", "wall001"):
        orc = ob.PortOracle(cam, constants=constants_of(huber))
        out["new"] = orc.fuse_map(0, img, dep, POSE, np.zeros(0, ob.SURFEL_DTYPE))[1]
        orc.close()
    return out


def check_census(ob, cam, family, huber=0.4):
    """the conditions of a family on every variant; returns the censuses.  (The fit-class conditions need tests/hostemu.cpp's
    counters: tests/test_cpu_crafted_frames.py.)"""
    gw, gh = grid(cam)
    S = gw * gh
    out = []
    for v in range(VARIANTS):
        c = census(ob, cam, family, v, huber)
        tag = (family, v, huber)
        assert c["labels_on_grid"] and c["labels_below_zero"] == 0, tag
        assert np.array_equal(c["fitted"], c["predicted"]), (tag, "the float quotient does not predict the fitted seeds")
        if family == "valid":
            for k in (15, 16, 17):
                assert (c["n"] == k).sum() >= 24, (tag, k)
            assert not c["fitted"][c["n"] < 16].any() and c["fitted"][c["n"] >= 16].all(), tag
        if family == "ratio":
            for n, m in RATIO_PAIRS:
                cells = (c["n"] == n) & (c["m"] == m)
                assert cells.sum() >= 12, (tag, n, m, int(cells.sum()))
                want = not float(F32(m) / F32(n)) < 0.8
                assert (c["fitted"][cells] == want).all(), (tag, n, m)
        if family == "huber":
            assert c["lattice_cells"] >= 64, (tag, c["lattice_cells"])
        if family == "view":
            assert c["below"] >= 24 and c["above"] >= 24, (tag, c["below"], c["above"])
            assert c["new"] < c["fitted"].sum(), (tag, c["new"])
        if family == "wall01":
            assert c["member_vs_mean_list"] >= 24, (tag, c["member_vs_mean_list"])
        if family == "wall001":
            assert c["mean_depth_zero"] == S and c["new"] == 0 and not c["fitted"].any(), tag
        if family == "lengths":
            want = np.asarray(list_lengths(cam, v))
            assert np.array_equal(c["m"], want), tag
            assert c["fitted"][want >= 16].all() and not c["fitted"][want < 16].any(), tag
        out.append(c)
    if family == "edge":  # (every cell of a frame has the same layout: a variant puts all its seeds on the float or none)
        assert sum(c["on_float_below"] for c in out) >= S, (family, huber, [c["on_float_below"] for c in out])
        if huber == 0.4:  # (at 0.05 the residuals move four floats at a time: a frame on the float below never has the next one)
            assert sum(c["on_next_float"] for c in out) >= S, (family, huber, [c["on_next_float"] for c in out])
    return out


# ----------------------------------------------------------------------------------------------------------------------
# replays

def twice(fr):
    """every variant fed twice: reference index 0, then 1 -> [(image, depth, pose, ref)]"""
    return [(img, dep, POSE, ref) for img, dep in fr for ref in (0, 1)]


def lockstep(fr):
    """the variants as four frames of one handle -> [(image, depth, pose, ref)]"""
    return [(img, dep, POSE, t) for t, (img, dep) in enumerate(fr)]


def replay(ob, cam, frames_, huber=0.4, eigen33=False, reference=False):
    """one oracle (PortOracle, or the reference translation unit) through the frames from an empty map: per frame
    (new count, label image, seed table, map), copies"""
    oracle = ob.RefOracle(cam) if reference else ob.PortOracle(cam, constants=constants_of(huber), eigen33=eigen33)
    lo = np.zeros(0, ob.SURFEL_DTYPE)
    recs = []
    for img, dep, pose, ref in frames_:
        lo, k = oracle.fuse_map(ref, img, dep, pose, lo)
        recs.append((k, oracle.labels().copy(), oracle.seeds().copy(), lo.copy()))
    oracle.close()
    return recs
