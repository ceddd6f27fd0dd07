"""Painted frames for the superpixel sweeps: grey images whose LABEL IMAGE is chosen pixel by pixel, and depth images that put
k_init_seeds(_lanes), k_assign, k_update_seeds, k_update_seeds_rest and k_update_seeds_wave on the margins that exist only in
them -- built from numpy and the ORACLE alone (oracle/bindings.py, PortOracle), never from the product.

The device.  A pixel's candidates are the cells whose centre is less than 8 away in both axes: at most 2x2 cells.  The cells
carry four grey bands in a 2x2 tiling, at least 75 apart, so the candidates of every pixel have four different greys, and a
pixel painted with the grey of one candidate costs that candidate (FF.cpp:364-387) at least 75^2 / 100 = 56 less in intensity
than any other, against at most (14^2 + 14^2) / 16 = 24.5 of distance and 1.6 of depth (25 beside a seed whose mean depth is
+inf).  A seed whose members all carry its grey keeps that grey exactly (its intensity sum is n * g in fp32).  The label image
is therefore ours to choose among each pixel's candidates: paint(cam, owner, greys).  crafted_frames.py freezes the label image
on the cell grid (64 pixels a superpixel); here a superpixel has 1 to 225 pixels, its centroid is anywhere in its reach and its
depth list has any length up to 225.

A seed's centre pixel has that seed as its ONLY candidate (the neighbouring centres are exactly 8 away) and lies inside the
statistics window, so a seed always owns a pixel: the "first empty seed abandons its worker chunk" rule (FF.cpp:516-517) cannot
be reached from frames, only from injected labels (test_state_level_early_return does that).  40 random few-grey / hole /
near-depth frames and the eleven edge cases were searched with the oracle; none emptied an unstable seed.  Nobody need look
again.

Designs.  `big` seeds (one parity class of cells, chosen by the variant's phase: their reaches of 15x15 pixels do not overlap)
take a chosen subset of their reach; what they leave of their own cell goes to the four neighbours (shrink); every other pixel
stays with its own cell.  The grey tiling is rolled so that the big seeds sit on the band the family wants.

Families (frames(cam, family) -> VARIANTS x (image, depth, owner)):

  sizes      big seeds of 1 (centre only), 2, 63, 64, 65, 123, 124, 125, 224 and 225 pixels: the full 15x15 block, blocks pushed
             into each far corner of the reach (largest column and row sums), a single far row, a single far column; the border
             seeds keep the whole reach the image leaves them.  The big seeds' band is grey 255: a 225-pixel seed has the largest
             intensity sum there is (57 375, in the low half of k_update_seeds' packed count << 16 | sum).  Depth uniform in
             3.5 .. 4.5 m.
  lists      every big seed owns its whole reach; m of its members lie on a wall, the others on the float below 0.1 (variant 0),
             on 0 or on NaN: the member count and the depth list are independent (in variant 0 one entry of every long list is the
             float ABOVE 0.1, the least depth FF.cpp:508 takes).  m = LIST_M.  Placements, by seed: the FIRST m
             members in window order (the list passes 124 early and is followed by members without depth), the LAST m (it
             reaches its final length in the last quad of the window it touches), m at random (members with and without depth
             follow).  A few small seeds hold one pixel at +inf (`settled` in k_update_seeds) and a few are shrunk to their
             centre pixel, so that one wave of 64 consecutive seeds meets an `over` seed, a `settled` one, a one-pixel one and
             an empty list together.  Variant 0 keeps its wall within 4 +- 0.01 m: a pixel on 0.1 has an inverse-depth term of
             38 000 against every candidate, and the term's DIFFERENCE between two candidates must stay below the intensity gap.
  lists_inf  the same with one +inf among the m list entries of every big seed (the seed is `settled`: finished in the lane
             kernel whatever its length), m = INF_M.
  lists_long the same with m = LONG_M, for a camera of 320x192: more seeds of one frame are queued for a wave of their own
             than k_update_seeds_rest has workgroups for them (kRestOverBlocks = 128), which then stride the queue.  Not one
             of FAMILIES: only the test that needs it builds it.
  passes     lists below 124 whose robust mean needs 1 .. 5 Huber-Newton passes: L members with a depth, f of them on a far
             group (PASS_RECIPE), the rest on a 4 m wall; the others 0.  L = PASS_L sits on both sides of every block boundary of
             huber_pass_lanes / _regs (8) and of the register loads of k_update_seeds_rest (16, and the wave's longest list).
             Queued and unqueued seeds alternate along the seed index, so queue order differs from seed order.
  stable     the `moved < 0.2` margin (FF.cpp:522, a float against a double).  By intensity: n / 5 of a big seed's n members
             are one grey above the seed's grey g = 0 .. 20 -- the centroid stays, the mean becomes the float nearest g + 0.2:
             at or above 0.2 for g = 0 (ON float(0.2)), 1, 2, 3, 16, below for 4 .. 15.  By the centroid: 200 of the 225 pixels,
             the 25 left out chosen so that the offset sum / n is (0.2, 0), (0, 0.2) or (0.1, 0.1); the sum x / n lands on either
             side of 0.2 by the seed's image coordinates.  On the float BELOW float(0.2): no grey quotient gets there, a split
             between greys and offsets does (mix_below).  A stable flag shows in a frame's result only through what the next
             sweep skips: see _stable for the probe pixels that make it show.
  drift      pixels on greys between two bands that change owner in sweep 1 (next to seeds that sweep 0 left unstable, and
             next to seeds it froze and an earlier pixel of the scan wakes) and in sweep 2: see _drift.
  scan       seed initialisation (FF.cpp:596-613): windows whose first depth in scan order decides where a tell-tale pixel
             ends up after the three sweeps -- first hits in rows 1 .. 8 and column 15, two depths in the two rows of one row
             pair of the lane form, a window whose only depth lies in row 15, clipped windows, a depth in the last image column
             and row that the scan must not see, windows without any depth: see _scan_build.  (Every other depth of these frames is 0, so nothing is fused.)

census(ob, cam, img, dep, owner) runs PortOracle stage by stage (initialize_seeds, then update_pixels / update_seeds three
times), checks the labels after every sweep against the design, restates update_seeds in numpy (restate: integer sums, the
fp32 depth sum in window row-major order, the Huber-Newton passes chain by chain, double comparisons) and checks x, y, mean
intensity, mean depth and the stable flag bit for bit against the oracle's seed table -- that comparison is what makes the
restatement's counts trustworthy.  Per sweep it returns member count, list length and sum, moved, the stable flags, the pass
count and the two figures the device must reproduce exactly (dsm_debug_tier_counts):

  n_over  unstable seeds with a list of >= 124 depths whose sum is not +inf  (kQueueWave: k_update_seeds clamps the list's end
          to row 124 at the start of every quad, so its register length is >= 124 exactly when the true length is)
  n_rest  unstable seeds with a list of 1 .. 123 depths, sum not +inf, whose first pass steps by 0.01 or more  (kQueueRest)

Measured with PortOracle (and tests/hostemu.cpp for the pick) at 160x96 / 166x103, S = 240, per variant 0..3; MEASURED at the
end of the module holds every figure, test_cpu_painted_frames.py prints and asserts them.  At 160x96:
  sizes      13 .. 16 seeds of 225 pixels on grey 255; every size of SIZES in 2 .. 20 seeds; n_over 35 .. 40 in sweep 0
  lists      4 big seeds at each m of LIST_M; n_over 32 in sweep 0, 4 .. 8 in sweep 1; 2 .. 4 waves hold an over, a settled, a
             one-pixel and an empty-list seed together; quads that start at 121 + 3, 4, at 122 + 2, 3, 4, at 123 + 1, 2, 3, 4
  lists_inf  10 .. 21 big seeds at each m of INF_M, all settled, none of them queued for a wave: n_over 0 at 160x96; at 166x103,
             variant 0, n_over is 1 in sweeps 0 and 1 -- a small seed of the last cell column, which owns the border pixels
             beyond the grid there, holds 124 depths or more
  passes     seeds by pass count 1 / 2 / 3 / 4 / 5: 104 / 16 / 40 / 42 / 38 (variant 0); n_rest 133 .. 136; 2 .. 4 waves with a
             queued list of 123 among three or more queued lists of at most 8
  stable     moved within 1e-5 of 0.2: 17 .. 21 seeds at or above, 24 .. 28 below; 1 .. 3 ON float(0.2), 4 .. 6 on the float below;
             19 .. 20 by the centroid alone; 8 .. 9 probes leave in sweep 1 (1 .. 2 of them from a seed ON float(0.2)), 5 .. 6
             stay; 229 .. 231 of 240 seeds stable after sweep 1
  drift      190 .. 270 pixels change owner in sweep 1, 42 .. 60 in sweep 2, 11 .. 15 of them out of a seed that was stable when
             the sweep began; n_over 32 .. 45 and n_rest 21 .. 26 in sweep 2
  scan       58 crafted seeds, 56 of them end differently with the scan order reversed (all but the two row-15 windows, which hold
             one depth: both end differently when the scan stops a row early); 8 .. 9 pairs in the variants whose big seeds sit in the first
             cell row, all of them end differently with the rows of a pair swapped; 6 mirrored seeds in the variants whose big
             seeds sit in the last cell column; first hits in every window row 1 .. 8, 5 .. 6 in column 15, 6 .. 8 in the tell-tale's
             row; 2 empty windows
  lists_long (320x192, S = 960) n_over 210 .. 211 in sweep 0, past kRestOverBlocks = 128
  pick_seed_fast left no painted pixel open (a painted pixel's candidates differ by 20 in cost at the least).
"""
import numpy as np

from crafted_frames import CELL, F32, POSE, expected_labels, flt_above, flt_below, grid  # noqa: F401

VARIANTS = 4
FAMILIES = ("sizes", "lists", "lists_inf", "passes", "stable", "drift", "scan")
CAP = 124  # k_update_seeds: kLaneCap - 3, the list length from which a seed is queued for a wave of its own
SIZES = (1, 2, 63, 64, 65, 123, 124, 125, 224, 225)
LIST_M = (0, 1, 119, 120, 121, 122, 123, 124, 125, 126, 127, 128, 129, 224, 225)
INF_M = (10, 123, 124, 200)
LONG_M = (124, 125, 127, 123, 126, 129, 144, 128)  # lists_long: seven of eight big seeds are queued for a wave of their own
PASS_L = (1, 7, 8, 9, 15, 16, 17, 111, 112, 113, 122, 123)
# list length -> passes wanted -> (members of the far group, its depth): found by running FF.cpp:530-556 over a 4 m wall with the
# group spread evenly through the list, keeping the recipes whose FINAL mean stays within 3.5 .. 4.6 m (a group that sends
# the wall's residuals into the tail moves the mean by 0.04 per element and pass -- 4.4 m for a list of 123 -- and the
# inverse-depth term of such a mean breaks the paint).  The census counts the passes a frame really takes.
PASS_RECIPE = {
    1: {1: (0, 0.0)},
    7: {1: (0, 0.0), 3: (1, 4.6), 4: (1, 4.9), 5: (1, 5.6)},
    8: {1: (0, 0.0), 3: (1, 4.6), 4: (1, 5.3), 5: (1, 6.5)},
    9: {1: (0, 0.0), 2: (1, 4.6), 3: (1, 4.75), 4: (1, 5.3), 5: (1, 8.0)},
    15: {1: (0, 0.0), 2: (1, 4.45), 3: (1, 5.3), 4: (1, 8.0), 5: (1, 30.0)},
    16: {1: (0, 0.0), 2: (1, 4.45), 3: (1, 5.3), 4: (1, 8.0), 5: (1, 30.0)},
    17: {1: (0, 0.0), 2: (1, 4.45), 3: (1, 5.3), 4: (1, 12.0), 5: (1, 30.0)},
    111: {1: (0, 0.0), 2: (1, 5.6), 3: (4, 12.0), 4: (13, 30.0), 5: (9, 30.0)},
    112: {1: (0, 0.0), 2: (1, 5.6), 3: (4, 12.0), 4: (27, 12.0), 5: (9, 30.0)},
    113: {1: (0, 0.0), 2: (1, 5.6), 3: (4, 12.0), 4: (23, 30.0), 5: (9, 30.0)},
    122: {1: (0, 0.0), 2: (1, 5.6), 3: (5, 12.0), 4: (18, 30.0), 5: (10, 30.0)},
    123: {1: (0, 0.0), 2: (1, 5.6), 3: (5, 12.0), 4: (16, 30.0), 5: (10, 30.0)},
}
BANDS = (10, 95, 180, 255)       # the tiling; the big seeds sit on the LAST band
STABLE_BANDS = (255, 175, 95, 0)  # stable family: the big seeds' band is g = 0 .. 20 (last), the others >= 75 above it
PHASES = ((0, 0), (1, 1), (1, 0), (0, 1))  # (x, y) parity of the big seeds' cells, per variant


# ----------------------------------------------------------------------------------------------------------------------
# geometry

def seed_cells(cam):
    gw, gh = grid(cam)
    s = np.arange(gw * gh)
    return s % gw, s // gw


def centres(cam):
    gx, gy = seed_cells(cam)
    return gx * CELL + CELL // 2, gy * CELL + CELL // 2


def reach(cam, s):
    """(x0, x1, y0, y1), inclusive: the pixels that have seed s among their candidates"""
    cx, cy = centres(cam)
    return (max(cx[s] - 7, 0), min(cx[s] + 7, cam.width - 1), max(cy[s] - 7, 0), min(cy[s] + 7, cam.height - 1))


def is_interior(cam, s):
    gw, gh = grid(cam)
    gx, gy = s % gw, s // gw
    return 0 < gx < gw - 1 and 0 < gy < gh - 1


def big_seeds(cam, v):
    px, py = PHASES[v % 4]
    gx, gy = seed_cells(cam)
    return np.flatnonzero((gx % 2 == px) & (gy % 2 == py))


def seed_greys(cam, v, bands=BANDS):
    """per seed the grey of its cell: the 2x2 tiling of `bands`, rolled so that the big seeds of variant v sit on bands[-1]"""
    px, py = PHASES[v % 4]
    gx, gy = seed_cells(cam)
    return np.asarray(bands, np.uint8)[3 - (((gy + py) % 2) * 2 + (gx + px) % 2)]


def paint(cam, owner, greys):
    """the grey image of an owner image (per pixel one of its candidate cells, -1 where has_candidate_cell is false) and the
    seeds' greys"""
    owner = np.asarray(owner)
    assert owner.shape == (cam.height, cam.width) and np.array_equal(owner < 0, expected_labels(cam) < 0)
    y, x = np.mgrid[0:cam.height, 0:cam.width]
    cx, cy = centres(cam)
    o = np.where(owner < 0, 0, owner)
    assert ((np.abs(cx[o] - x) < CELL) & (np.abs(cy[o] - y) < CELL))[owner >= 0].all(), "an owner that is no candidate"
    assert np.array_equal(owner[cy, cx], np.arange(len(cx))), "a centre pixel has its own seed as its only candidate"
    return np.where(owner < 0, 0, np.asarray(greys, np.uint8)[o]).astype(np.uint8)


def shrink(cam, owner, s, keep=()):
    """what seed s still owns of its own cell goes to the four neighbours, but its centre and the pixels `keep` [(y, x)]"""
    gw, gh = grid(cam)
    assert is_interior(cam, s)
    cx, cy = centres(cam)
    ys, xs = np.nonzero(owner == s)
    for y, x in zip(ys, xs):
        if (y, x) == (cy[s], cx[s]) or (y, x) in keep:
            continue
        owner[y, x] = s + np.sign(x - cx[s]) if x != cx[s] else s + gw * np.sign(y - cy[s])


def claim(cam, owner, s, mask):
    """big seed s takes the pixels of its 15x15 reach where mask[dy + 7, dx + 7]; for an interior seed the rest of its own cell
    goes to the neighbours (its size is then exactly mask.sum()); a border seed takes its whole reach"""
    cx, cy = centres(cam)
    x0, x1, y0, y1 = reach(cam, s)
    if not is_interior(cam, s):
        owner[y0:y1 + 1, x0:x1 + 1] = s
        return
    assert mask[7, 7] and (x0, x1, y0, y1) == (cx[s] - 7, cx[s] + 7, cy[s] - 7, cy[s] + 7)
    box = owner[y0:y1 + 1, x0:x1 + 1]
    box[mask] = s
    shrink(cam, owner, s, keep={(y0 + dy, x0 + dx) for dy, dx in zip(*np.nonzero(mask))})


def corner_block(n, sx, sy, by_rows=True):
    """n pixels of the 15x15 reach pushed into the corner (sx, sy = +-1): whole far rows (columns), then part of the next one;
    the centre is always one of them"""
    m = np.zeros((15, 15), bool)
    m[7, 7] = True
    k = 0
    while m.sum() < n:
        a, b = divmod(k, 15)
        dy, dx = (7 - a) * sy, (7 - b) * sx
        if not by_rows:
            dy, dx = (7 - b) * sy, (7 - a) * sx
        m[dy + 7, dx + 7] = True
        k += 1
    return m


def window_order(cam):
    """per seed its 16x16 statistics window in row-major order (FF.cpp:482-513): pixel index (clipped into the image) and
    whether the window, clipped to [0, w - 1) x [0, h - 1), holds it -- the last column and row never count"""
    gx, gy = seed_cells(cam)
    j = np.arange(2 * CELL)
    X = (gx * CELL - CELL // 2)[:, None, None] + j[None, None, :]
    Y = (gy * CELL - CELL // 2)[:, None, None] + j[None, :, None]
    valid = (X >= 0) & (X < cam.width - 1) & (Y >= 0) & (Y < cam.height - 1)
    flat = np.clip(Y, 0, cam.height - 1) * cam.width + np.clip(X, 0, cam.width - 1)
    S = len(gx)
    X, Y = np.broadcast_to(X, flat.shape), np.broadcast_to(Y, flat.shape)
    return flat.reshape(S, -1), valid.reshape(S, -1), X.reshape(S, -1), Y.reshape(S, -1)


def members_in_order(cam, owner):
    """per seed the flat pixel indices of its members inside the statistics window, in the order update_seeds meets them"""
    flat, valid, _, _ = window_order(cam)
    lab = owner.ravel()[flat]
    return [flat[s][valid[s] & (lab[s] == s)] for s in range(len(flat))]


# ----------------------------------------------------------------------------------------------------------------------
# the families

def _base(cam):
    return expected_labels(cam).copy()


def _sizes(cam, v):
    rng = np.random.default_rng(100 + v)
    owner = _base(cam)
    shapes = []
    for i, n in enumerate((225, 224, 1, 225, 2, 63, 64, 225, 65, 123, 124, 225, 125, 16, 16, 225)):
        shapes.append((n, i))
    for k, s in enumerate(big_seeds(cam, v)):
        n, i = shapes[(k + 5 * v) % len(shapes)]
        sx, sy = (1, -1)[(k + v) % 2], (1, -1)[((k + v) // 2) % 2]
        if n == 16:  # a single far row (i even) or column: its 15 pixels and the centre
            mask = np.zeros((15, 15), bool)
            mask[7, 7] = True
            if i % 2 == 0:
                mask[7 + 7 * sy, :] = True
            else:
                mask[:, 7 + 7 * sx] = True
        else:
            mask = corner_block(n, sx, sy, by_rows=(k // 4) % 2 == 0)
        claim(cam, owner, s, mask)
    dep = rng.uniform(3.5, 4.5, owner.shape).astype(F32)
    return paint(cam, owner, seed_greys(cam, v)), dep, owner


def _full_big(cam, v):
    owner = _base(cam)
    for s in big_seeds(cam, v):
        claim(cam, owner, s, np.ones((15, 15), bool))
    return owner


def _small_interior(cam, v):
    """the small seeds left and right of (above and below) two big ones, interior: candidates for one-pixel and settled seeds"""
    px, py = PHASES[v % 4]
    gx, gy = seed_cells(cam)
    gw, gh = grid(cam)
    sel = (gx % 2 != px) & (gy % 2 == py) & (gx > 0) & (gx < gw - 1) & (gy > 0) & (gy < gh - 1)
    return np.flatnonzero(sel)


def _lists_build(cam, v, inf, long=False):
    """-> image, depth, owner, {big seed: (m, placement)}; placement 0: the FIRST m members in window order, 1: the LAST m, 2: m at random"""
    rng = np.random.default_rng(200 + v + 10 * inf)
    owner = _full_big(cam, v)
    small = _small_interior(cam, v)
    one_pixel, settled_small = small[v % 5::5], small[(v + 2) % 5::5]
    for s in one_pixel:
        shrink(cam, owner, s)
    narrow = v % 4 == 0 and not inf
    wall = (4.0 + rng.uniform(-0.01, 0.01, owner.shape) if narrow else rng.uniform(3.5, 4.5, owner.shape)).astype(F32)
    dep = wall.copy().ravel()
    cx, cy = centres(cam)
    order = members_in_order(cam, owner)
    bigs = big_seeds(cam, v)
    full = [s for s in bigs if len(order[s]) == 225]
    if inf:
        plan = [(s, [m for m in np.roll(INF_M, k + v) if m <= len(order[s])][0]) for k, s in enumerate(bigs)]
    else:
        top = full[v::5][:8]  # eight whole seeds take 224 and 225
        assert len(top) == 8
        values = LONG_M if long else LIST_M[:13]
        pool = [int(m) for m in np.roll(np.tile(values, -(-len(bigs) // len(values))), 3 * v)]
        rest = sorted((s for s in bigs if s not in top), key=lambda s: (len(order[s]) > 129, s))  # (clipped seeds choose first)
        plan = [(s, (224, 225)[k % 2]) for k, s in enumerate(top)]
        for s in rest:
            fits = [m for m in pool if m <= len(order[s])]
            m = fits[0] if fits else len(order[s])
            if fits:
                pool.remove(m)
            plan.append((s, m))
        plan.sort(key=lambda sm: sm[0])
    fillers = (flt_below(0.1), F32(0), F32(np.nan))
    seen_m, places = {}, {}
    for k, (s, m) in enumerate(plan):
        idx = order[s]
        n = len(idx)
        assert m <= n
        fill = fillers[0] if narrow else fillers[1 + (k + v) % 2]
        place = (seen_m.get(m, 0) + m + v) % 3  # (the seeds of one m take the three placements in turn)
        seen_m[m] = seen_m.get(m, 0) + 1
        places[int(s)] = (int(m), place)
        chosen = {0: np.arange(m), 1: np.arange(n - m, n), 2: np.sort(rng.permutation(n)[:m])}[place]
        centre = int(np.flatnonzero(idx == cy[s] * cam.width + cx[s])[0])
        if narrow and m and centre not in chosen:  # (a centre on 0.1 would be the seed's first mean depth: FF.cpp:598)
            chosen = np.sort(np.append(chosen[:-1] if place == 0 else chosen[1:], centre))
        own = np.flatnonzero(owner.ravel() == s)  # (the last column and row of the image included)
        dep[own] = fill
        dep[idx[chosen]] = wall.ravel()[idx[chosen]]
        if narrow and m >= 119:  # one list entry ON the float above 0.1, beside the fillers on the float below it
            dep[[i for i in idx[chosen] if i != cy[s] * cam.width + cx[s]][(k * 5) % (m - 1)]] = flt_above(0.1)
        if inf:
            dep[idx[chosen[(k * 7) % m]]] = np.inf
    if not inf:
        for s in settled_small:
            dep[order[s][len(order[s]) // 2]] = np.inf
    return paint(cam, owner, seed_greys(cam, v)), dep.reshape(owner.shape), owner, places


def _lists(cam, v, inf, long=False):
    return _lists_build(cam, v, inf, long)[:3]


def _passes(cam, v):
    rng = np.random.default_rng(300 + v)
    owner = _full_big(cam, v)
    order = members_in_order(cam, owner)
    wall = (4.0 + rng.uniform(-0.002, 0.002, owner.shape)).astype(F32).ravel()
    dep = np.zeros(owner.size, F32)
    k_big = k_small = 0
    bigs = set(big_seeds(cam, v).tolist())
    for s, idx in enumerate(order):
        n = len(idx)
        if s in bigs:
            L, want = PASS_L[(k_big + v) % len(PASS_L)], 1 + (k_big // len(PASS_L) + k_big + v) % 5
            k_big += 1
        else:
            L, want = PASS_L[(k_small + v) % 5], 1 + (k_small // 5 + k_small + 2 * v) % 5
            k_small += 1
        L = max(length for length in PASS_L if length <= min(L, n))
        f, far = PASS_RECIPE[L].get(want, PASS_RECIPE[L][1])
        chosen = {0: idx[:L], 1: idx[n - L:], 2: np.sort(rng.permutation(idx)[:L]), 3: idx[:L]}[(s + v) % 4]
        dep[chosen] = wall[chosen]
        if f:
            dep[chosen[np.linspace(0, L - 1, f + 2).astype(int)[1:-1]]] = F32(far)
    return paint(cam, owner, seed_greys(cam, v)), dep.reshape(owner.shape), owner


def _offset_set(rng, rx, ry, q=25):
    """q pixels of the 15x15 reach outside the seed's own cell whose offsets sum to (-rx, -ry): without them the block's offset sum
    is (rx, ry)"""
    dy, dx = np.mgrid[-7:8, -7:8]
    ring = np.flatnonzero(~((dx >= -4) & (dx <= 3) & (dy >= -4) & (dy <= 3)).ravel())
    dxr, dyr = dx.ravel(), dy.ravel()
    for _ in range(200000):
        pick = rng.choice(ring, q, replace=False)
        ex, ey = dxr[pick].sum() + rx, dyr[pick].sum() + ry
        for _ in range(40):  # walk the misfit down: move one pixel of the set
            if ex == 0 and ey == 0:
                m = np.ones(225, bool)
                m[pick] = False
                return m.reshape(15, 15)
            i = rng.integers(q)
            cand = rng.choice(ring)
            if cand in pick:
                continue
            nx, ny = ex - dxr[pick[i]] + dxr[cand], ey - dyr[pick[i]] + dyr[cand]
            if abs(nx) + abs(ny) <= abs(ex) + abs(ey):
                pick[i], ex, ey = cand, nx, ny
    raise AssertionError("no offset set")


def mix_below(cx, cy):
    """(n, k, rx, ry): a seed centred on (cx, cy) with n members of grey 0 whose offsets sum to (rx, ry), k of them on grey 1,
    has moved = k / n + |rx| / n + |ry| / n on the float BELOW float(0.2) -- (k + |rx| + |ry|) / n is 0.2, and the roundings of
    the two coordinate quotients carry the sum down; None where no split does.  Intensity alone cannot get there: no quotient
    of integers up to 225 lies within 2e-8 of 0.2 but 0.2 itself."""
    below = np.nextafter(F32(0.2), F32(0))
    cx, cy = F32(cx), F32(cy)
    for n in range(150, 225, 5):
        fn, T = F32(n), n // 5
        for k in range(T + 1):
            ax = np.arange(T + 1 - k)
            ay = T - k - ax
            for sx in (1, -1):
                for sy in (1, -1):
                    dx = np.abs(cx - (fn * cx + (sx * ax).astype(F32)) / fn)
                    dy = np.abs(cy - (fn * cy + (sy * ay).astype(F32)) / fn)
                    hit = np.flatnonzero((F32(k) / fn + dx) + dy == below)
                    if len(hit):
                        return n, k, int(sx * ax[hit[0]]), int(sy * ay[hit[0]])
    return None


PROBE = 35  # stable family: what a probe pixel is above its seed's grey


def _stable(cam, v):
    """-> image, depth, [the label image after sweep 0, 1, 2].  A seed's stable flag after sweep 0 shows in the frame's result
    only through what sweep 1 then does, so big seeds of the `grey` kind carry a PROBE pixel, four columns
    right of the centre and PROBE greys above the seed (it counts as PROBE of the greys one up).  The small seed B to the right
    has its centre on 95 and its other members on 50: its mean is 95 in sweep 0 and 55.6 afterwards.  The probe is A's in
    sweep 0 (12.25 against 16 at the least); in sweep 1 it would be B's (12.1 against 4.2 at the most) -- if sweep 1 looks at
    it, that is, if A was NOT stable.  The design says which, from `moved` in numpy."""
    rng = np.random.default_rng(400 + v)
    gw, gh = grid(cam)
    owner = _base(cam)
    greys = seed_greys(cam, v, STABLE_BANDS).copy()
    bigs = big_seeds(cam, v)
    cx, cy = centres(cam)
    kinds, ups = {}, {}
    for k, s in enumerate(bigs):
        kind = ("grey", "grey", "mix", "x", "y", "xy", "grey")[(k + v) % 7] if is_interior(cam, s) else "grey"
        mix = mix_below(cx[s], cy[s]) if kind == "mix" else None
        if kind == "mix" and mix is None:
            kind = "grey"
        kinds[s] = kind
        sign = (1, -1)[(k // 6) % 2]
        ups[s] = mix[1] if mix else None
        mask = {"grey": lambda: np.ones((15, 15), bool), "x": lambda: _offset_set(rng, 40 * sign, 0),
                "y": lambda: _offset_set(rng, 0, 40 * sign), "xy": lambda: _offset_set(rng, 20 * sign, -20 * sign),
                "mix": lambda: _offset_set(rng, mix[2], mix[3], 225 - mix[0])}[kind]()
        claim(cam, owner, s, mask)
        greys[s] = 0 if kind == "mix" else (k * 5 + v) % 21
    # (both big neighbours of B whole, so that B is exactly its column of eight)
    probed = [s for s in bigs if kinds[s] == "grey" and is_interior(cam, s) and is_interior(cam, s + 1) and kinds.get(s + 2) == "grey"]
    for j, s in enumerate(probed):  # moved is at or above 0.2 for g = 0 (ON float(0.2)), 1, 2, 3, 16 and below it for 4 .. 15
        greys[s] = (0, 1, 4, 2, 9, 3, 16, 12)[(j + v) % 8]
    img = paint(cam, owner, greys).ravel()
    order = members_in_order(cam, owner)
    designs = [owner.copy(), owner.copy(), owner.copy()]
    for s in bigs:
        n = len(order[s])
        if kinds[s] not in ("grey", "mix") or n % 5:
            continue
        k_up = n // 5 if ups[s] is None else ups[s]
        centre = cy[s] * cam.width + cx[s]
        probe = None
        if s in probed and k_up >= PROBE:
            spots = [i for i in order[s] if i % cam.width == cx[s] + 4 and abs(i // cam.width - cy[s]) <= 6]
            if spots:
                probe = spots[rng.integers(len(spots))]
                img[probe] += PROBE
                k_up -= PROBE
                ys, xs = np.nonzero(owner == s + 1)  # B: the column of eight right of s
                img[(ys * cam.width + xs)[ys != cy[s + 1]]] = 50
                g, fn = F32(greys[s]), F32(n)
                total = F32(n * int(greys[s]) + (n // 5 if ups[s] is None else ups[s]))
                offs = order[s] - centre  # the centroid, as update_seeds takes it
                mx = F32((order[s] % cam.width).sum()) / fn
                my = F32((order[s] // cam.width).sum()) / fn
                moved = np.abs(g - total / fn) + np.abs(F32(cx[s]) - mx) + np.abs(F32(cy[s]) - my)
                if not float(moved) < 0.2:  # A is unstable after sweep 0: sweep 1 looks at the probe
                    designs[1].ravel()[probe] = designs[2].ravel()[probe] = s + 1
        up = rng.permutation(order[s][(order[s] != centre) & (order[s] != probe)])[:k_up]
        img[up] += 1
    dep = rng.uniform(3.5, 4.5, owner.shape).astype(F32)
    return img.reshape(owner.shape), dep, designs


DRIFT_BANDS = (255, 180, 95, 10)  # drift family: the big seeds on 10, their left / right neighbours on 95, those above / below on 180
DRIFT_JUMP = 30                   # what the members of a small seed differ from its centre by: its mean jumps after sweep 0


def _drift(cam, v):
    """-> image, depth, [the label image after sweep 0, 1, 2].  Every big seed A owns its whole reach and is grey 10; the small
    seed B to its right (a column of eight pixels) has its centre on 95 and its other members on 65, so its mean is 95 in
    sweep 0 and 68.75 from sweep 1 on; the small seed C above A (a row of eight) has its centre on 180, the others on 210.
      kind a  eight pixels of A, 4 .. 6 columns right of its centre, are painted 50: A's in sweep 0 (16 against 20.25 in
              intensity), B's from sweep 1 on (15 against 3.5); A's mean moves by 1.8 and A stays unstable.  Two more, 1 or 2
              columns right of the centre, are painted 40: A's in sweeps 0 and 1 (8 against 8.3 and at least 2 of distance),
              B's in sweep 2, once B's mean has come down to 59.4 with the eight pixels it took (8.8 against 3.8).
      kind b  one pixel of A right of its centre column is painted 45: A's mean moves by 0.156 and A is STABLE after sweep 0.
              The pixel above A's centre is painted 100 and is C's in sweep 0 (67 against 81); C's mean jumps to 194 and the
              pixel comes to A in sweep 1 (81 against 92), which wakes A: the 45-pixel, later in the scan, is looked at after
              all and goes to B.  Its old seed was stable when the sweep began.
    Depths within 3.9 .. 4.1 m, the depth term stays below 0.1; 8 % of the pixels that keep their owner lie at 5 m."""
    rng = np.random.default_rng(500 + v)
    px, py = PHASES[v % 4]
    gw, gh = grid(cam)
    owner = _full_big(cam, v)
    greys = seed_greys(cam, v, DRIFT_BANDS)
    img = paint(cam, owner, greys)
    cx, cy = centres(cam)
    gx, gy = seed_cells(cam)
    small_h = ((gx + px) % 2 == 1) & ((gy + py) % 2 == 0)
    small_v = ((gx + px) % 2 == 0) & ((gy + py) % 2 == 1)
    for s in np.flatnonzero(small_h | small_v):
        ys, xs = np.nonzero(owner == s)
        keep = (ys != cy[s]) | (xs != cx[s])
        img[ys[keep], xs[keep]] += np.uint8(DRIFT_JUMP) if small_v[s] else np.uint8(256 - DRIFT_JUMP)
    designs = [owner.copy(), owner.copy(), owner.copy()]
    inner = [b for b in big_seeds(cam, v) if is_interior(cam, b) and is_interior(cam, b + 1) and is_interior(cam, b - gw)]
    for k, s in enumerate(inner):  # (B and C are interior too: a column and a row of exactly eight pixels)
        right, above = s + 1, s - gw
        if (k + v) % 3:  # kind a
            spots = [(dx, dy) for dx in range(4, 7) for dy in range(-6, 7)]
            for i in rng.permutation(len(spots))[:8]:
                dx, dy = spots[i]
                img[cy[s] + dy, cx[s] + dx] = 50
                designs[1][cy[s] + dy, cx[s] + dx] = designs[2][cy[s] + dy, cx[s] + dx] = right
            spots = [(dx, dy) for dx in (1, 2) for dy in range(-5, 6)]
            for i in rng.permutation(len(spots))[:2]:
                dx, dy = spots[i]
                img[cy[s] + dy, cx[s] + dx] = 40
                designs[2][cy[s] + dy, cx[s] + dx] = right
        else:  # kind b
            img[cy[s] - 1, cx[s]] = 100
            designs[0][cy[s] - 1, cx[s]] = above
            dx, dy = int(rng.integers(1, 8)), int(rng.integers(0, 7))
            img[cy[s] + dy, cx[s] + dx] = 45
            designs[1][cy[s] + dy, cx[s] + dx] = designs[2][cy[s] + dy, cx[s] + dx] = right
    dep = rng.uniform(3.9, 4.1, owner.shape).astype(F32)
    far = (rng.random(owner.shape) < 0.08) & (designs[0] == designs[2])  # (not on a pixel that changes hands, nor on a centre:
    far[cy, cx] = False                                                  # a seed's first mean depth, FF.cpp:598)
    dep[far] = 5.0  # tail members of the robust mean: lists of more than one pass in every sweep
    return img, dep, designs


SCAN_D1, SCAN_D2 = F32(0.2), F32(0.25)  # 400 * (5 - 4)^2 = 400 where a seed's first mean depth and a pixel's depth differ
SCAN_GREY = 54  # on a big seed of grey 10: 44 / 225 = 0.1956 of `moved`, still stable
SCAN_PLACES = ((1, 9), (4, 15), (6, 2), (7, 1), (8, 5), (2, 14), (3, 14), (5, 3))  # (window row, column) of the first hit


def scan_md(cam, dep, mode="first"):
    """seed initialisation's mean depth (FF.cpp:596-613) in numpy: the centre's depth, or where that is below 0.01 the first
    depth above 0.01 of the window clipped to [0, w - 1) x [0, h - 1) in row-major order.  The other modes are the mistakes the
    family is built against: "reverse" takes the LAST hit, "pair_swap" takes the rows of every pair (2j, 2j + 1) of the unclipped
    window in the other order, "stop_early" never looks at window row 15."""
    flat, valid, _, _ = window_order(cam)
    cx, cy = centres(cam)
    d = dep.ravel()
    md = d[cy * cam.width + cx].astype(F32).copy()
    order = np.arange(256)
    if mode == "pair_swap":
        order = (order.reshape(8, 2, 16)[:, ::-1]).ravel()
    if mode == "stop_early":
        order = order[:240]
    with np.errstate(invalid="ignore"):
        for s in np.flatnonzero(md.astype(np.float64) < 0.01):
            idx = flat[s][order]
            hits = np.flatnonzero(valid[s][order] & (d[idx].astype(np.float64) > 0.01))
            if len(hits):
                md[s] = d[idx[hits[-1 if mode == "reverse" else 0]]]
    return md


SCAN_BANDS = (255, 95, 95, 10)  # scan family: the small seeds beside AND above / below a big one on 95 (no pixel has both as candidates
                                # against anything but the big seed, whose 10 wins by paint)
SCAN_KINDS = ("first", "pair", "row15", "mirrored", "empty")


def _scan_build(cam, v):
    """-> image, depth, design, plan {big seed: (kind, (window row, column) of its depths before the tell-tale)}.
    Every big seed A owns its reach, is grey 10 and has NO depth at its centre; the small seeds left and right of the big
    ones (B, columns of eight) have SCAN_D1 at their centre; all other depths are 0 but a few per big seed.  The TELL-TALE is a
    pixel of SCAN_D2 painted SCAN_GREY whose only candidates are A and one small seed: the paint gives it to the small seed
    (16.8 against 19.4 of intensity, and nearer by 3), unless A's first mean depth is SCAN_D2 and the small seed's is
    SCAN_D1 -- then the small seed pays 400 for the depth and A nothing, A takes the tell-tale, is stable with it (moved =
    44 / 225 = 0.1956) and keeps it through sweeps 1 and 2, which skip the pixels of stable seeds.  Where the tell-tale ends
    therefore says which depth the scan took.  Kinds of big seed:
      first     SCAN_D1 at one of SCAN_PLACES (rows 1 .. 8; column 15; the tell-tale's own row), earlier in the scan than the
                tell-tale 7 columns right of the centre in the centre's row (window row 8, column 15), which is the LAST hit:
                it ends with B.  Windows clipped at the top and left borders are of this kind.
      pair      the big seeds of the first cell row (variants whose big seeds sit there): SCAN_D1 in window row 6, column 10, and
                SCAN_D2 in row 7, column 8 -- the two rows of ONE row pair of k_init_seeds_lanes, the earlier row with the later
                column.  The second is straight above the centre, where at the image's top A is the pixel's only candidate, so
                its depth cannot move it.  A starts on SCAN_D1 and the tell-tale (row 8, column 15) ends with B; a scan that
                takes the pair's rows in the other order, or columns before rows, starts on SCAN_D2 and A takes it.
      row15     the window's ONLY depth is its tell-tale, in row 15 below the centre, between A and the small seed under A
                (which has SCAN_D1 at its centre, one row below the window): seen, it ends with A; a scan that stops a row early
                leaves A on 0, the depth term does not apply and the paint gives it away.
      mirrored  the big seeds of the last cell column: the tell-tale 7 columns LEFT of the centre (row 8, column 1) beside the B
                there, the first hit in row 2, column 3 -- an earlier row with a later column -- and a SCAN_D2 in the image's last
                column, in window row 0: the scan must not see it (FF.cpp:604, the window is clipped to w - 1).  Likewise
                a SCAN_D2 in the last image row under every big seed of the last cell row.
      empty     no depth at all in the window (nor at the centre of the B left of it): the mean depth stays 0.
    scan_census counts the seeds of every kind and placement and proves each kind against the mistake it is for."""
    gw, gh = grid(cam)
    owner = _full_big(cam, v)
    greys = seed_greys(cam, v, SCAN_BANDS)
    cx, cy = centres(cam)
    gx, gy = seed_cells(cam)
    px, py = PHASES[v % 4]
    design = owner.copy()
    dep = np.zeros(owner.shape, F32)
    small_h = np.flatnonzero(((gx + px) % 2 == 1) & ((gy + py) % 2 == 0))
    dep[cy[small_h], cx[small_h]] = SCAN_D1
    img = paint(cam, owner, greys)
    plan = {}

    def tell_tale(y, x, to):
        dep[y, x], img[y, x], design[y, x] = SCAN_D2, SCAN_GREY, to

    for k, s in enumerate(big_seeds(cam, v)):
        s = int(s)
        in_first_column = (gy[s] - py) // 2 % 3 if gx[s] == px else 2  # down the first big column: empty, row15, first, ...
        if in_first_column < 2:  # nothing in rows 0 .. 14: not the centre of the B left of it either
            if px:
                dep[cy[s - 1], cx[s - 1]] = 0
            if in_first_column == 1 and cy[s] + 8 < cam.height - 1:
                tell_tale(cy[s] + 7, cx[s], s)
                dep[cy[s] + 8, cx[s]] = SCAN_D1  # the centre of the small seed under A
                plan[s] = ("row15", ((15, 8),))
            else:
                plan[s] = ("empty", ())
            continue
        side = 1 if gx[s] + 1 < gw else -1
        ty, tx = cy[s], cx[s] + 7 * side
        y0, x0 = cy[s] - 8, cx[s] - 8
        if side > 0 and gy[s] == 0:  # (window rows 4 .. 15 are inside the image)
            tell_tale(ty, tx, s + side)
            assert owner[y0 + 6, x0 + 10] == s and owner[y0 + 7, x0 + 8] == s
            dep[y0 + 6, x0 + 10], dep[y0 + 7, x0 + 8] = SCAN_D1, SCAN_D2
            plan[s] = ("pair", ((6, 10), (7, 8)))
            continue
        tell_tale(ty, tx, s + side)
        r, c = SCAN_PLACES[(k + v) % len(SCAN_PLACES)]
        if side < 0:
            r, c = 2, 3
        y, x = y0 + r, x0 + c
        if y < 0 or x < 0:  # (a window clipped at the top or the left border)
            y, x = max(y, 1 + k % 3), max(x, 2 + k % 2)
        assert owner[y, x] == s and (y, x) < (ty, tx)
        dep[y, x] = SCAN_D1
        plan[s] = ("mirrored" if side < 0 else "first", ((y - y0, x - x0),))
        if cx[s] + 8 > cam.width - 1 >= cx[s] - 8:
            dep[max(y0, 0), cam.width - 1] = SCAN_D2  # window row 0, the last image column: not seen
    for s in big_seeds(cam, v):
        if cy[s] + 8 > cam.height - 1 and dep[cam.height - 1, cx[s]] == 0:
            dep[cam.height - 1, cx[s]] = SCAN_D2      # the last image row (A its only candidate): not seen
    return img, dep, design, plan


def _scan(cam, v):
    return _scan_build(cam, v)[:3]


def scan_census(ob, cam, v):
    """the scan family's own proof: scan_md equals the oracle's initialisation bit for bit, and with the scan order REVERSED
    (fed through set_seeds) the oracle's final label image or seed table changes at the crafted seeds; -> the share that do,
    and how many seeds there are of every kind and placement"""
    img, dep, design, plan = _scan_build(cam, v)
    crafted = np.array([s for s, (kind, _) in plan.items() if kind != "empty"])
    finals = {}
    for mode in ("first", "reverse", "pair_swap", "stop_early"):
        orc = ob.PortOracle(cam)
        orc.set_frame(img, dep)
        orc.stage("initialize_seeds")
        seeds = orc.seeds().copy()
        assert np.array_equal(seeds["mean_depth"].view(np.int32), scan_md(cam, dep).view(np.int32)), "scan_md is not the oracle's scan"
        if mode != "first":
            seeds["mean_depth"] = scan_md(cam, dep, mode)
            orc.set_seeds(seeds)
        for _ in range(3):
            orc.stage("update_pixels")
            orc.stage("update_seeds")
        finals[mode] = (orc.labels().copy(), orc.seeds().copy())
        orc.close()
    lab0, sd0 = finals["first"]
    assert np.array_equal(lab0, design)

    def differs(s, mode):  # the final labels of the seed's reach, or its row of the seed table
        x0, x1, y0, y1 = reach(cam, s)
        lab1, sd1 = finals[mode]
        same = all(a == b or (a != a and b != b) for a, b in zip(sd0[s].tolist(), sd1[s].tolist()))  # field by field, NaN == NaN
        return bool((lab0[y0:y1 + 1, x0:x1 + 1] != lab1[y0:y1 + 1, x0:x1 + 1]).any() or not same)

    changed = sum(differs(s, "reverse") for s in crafted)
    md = scan_md(cam, dep)
    kinds = {kind: [s for s, (k_, _) in plan.items() if k_ == kind] for kind in SCAN_KINDS}
    first = [plan[s][1][0] for s in kinds["first"]]
    cx, cy = centres(cam)
    out = {"crafted": len(crafted), "changed_by_reversal": changed, "share": changed / len(crafted),
           "no_depth_at_all": int((md == 0).sum()),
           "pairs_changed_by_swap": sum(differs(s, "pair_swap") for s in kinds["pair"]),
           "row15_changed_by_stopping_early": sum(differs(s, "stop_early") for s in kinds["row15"]),
           "kinds": {kind: len(seeds_) for kind, seeds_ in kinds.items()},
           "first_in_tell_tale_row": int(sum(r == 8 for r, c in first)), "first_in_column_15": int(sum(c == 15 for r, c in first)),
           "first_rows": sorted({int(r) for r, c in first}),
           "clipped_left_or_top": int(sum(bool(cx[s] < 8 or cy[s] < 8) for s in crafted)),
           # two different depths, the earlier row holding the later column: the pairs and the mirrored seeds
           "earlier_row_later_column": len(kinds["pair"]) + len(kinds["mirrored"]),
           "last_column_unseen": int((dep[:, cam.width - 1] > 0).sum()), "last_row_unseen": int((dep[cam.height - 1] > 0).sum())}
    # what each kind's scan must find: SCAN_D2 in row 15 (the tell-tale ends with A), SCAN_D1 elsewhere, 0 in the empty windows
    for kind, want in (("first", SCAN_D1), ("mirrored", SCAN_D1), ("pair", SCAN_D1), ("row15", SCAN_D2), ("empty", F32(0))):
        assert (md[kinds[kind]] == want).all(), (kind, md[kinds[kind]])
    return out


def wide_camera(synth):
    """320x192, intrinsics scaled from TINY: 960 seeds, 240 of them big"""
    T = synth.TINY
    return synth.Camera(2 * T.width, 2 * T.height, 2 * T.fx, 2 * T.fy, 2 * T.cx + 0.5, 2 * T.cy + 0.5)


_CACHE = {}


def frames(cam, family):
    """[(image, depth, owner)] * VARIANTS of a family"""
    key = (cam, family)
    if key not in _CACHE:
        make = {"sizes": _sizes, "lists": lambda c, v: _lists(c, v, False), "lists_long": lambda c, v: _lists(c, v, False, True),
                "lists_inf": lambda c, v: _lists(c, v, True),
                "passes": _passes, "stable": _stable, "drift": _drift, "scan": _scan}[family]
        out = []
        for v in range(VARIANTS):
            img, dep, owner = make(cam, v)
            owner = [o.astype(np.int32) for o in owner] if isinstance(owner, list) else owner.astype(np.int32)
            out.append((np.ascontiguousarray(img, np.uint8), np.ascontiguousarray(dep, F32), owner))
        _CACHE[key] = out
    return _CACHE[key]


# ----------------------------------------------------------------------------------------------------------------------
# the census: update_seeds (FF.cpp:468-562) in numpy over the oracle's labels and seed tables

def restate(cam, lab, img, dep, before, huber=0.4):
    """one update_seeds over label image `lab`, from the seed table `before` it: dict of per-seed arrays (see census)"""
    flat, valid, X, Y = window_order(cam)
    S = len(flat)
    with np.errstate(all="ignore"):
        mem = valid & (lab.ravel()[flat] == np.arange(S)[:, None])
        d = dep.ravel()[flat].astype(F32)
        g = img.ravel()[flat].astype(np.int64)
        cnt = mem.sum(1)
        assert (cnt > 0).all()  # (the centre pixel)
        fn = cnt.astype(F32)
        # sums of integers below 2^24: exact in fp32 whatever the order
        x = (X * mem).sum(1).astype(F32) / fn
        y = (Y * mem).sum(1).astype(F32) / fn
        mi = (g * mem).sum(1).astype(F32) / fn
        moved = np.abs(before["mean_intensity"] - mi) + np.abs(before["x"] - x) + np.abs(before["y"] - y)
        assert moved.dtype == F32
        dv = mem & (d.astype(np.float64) > 0.1)
        nd = dv.sum(1)
        cols = np.flatnonzero(dv.any(0))
        total = np.zeros(S, F32)
        for k in cols:
            total = np.where(dv[:, k], total + d[:, k], total)
        md = np.where(nd > 0, total / np.maximum(nd, 1).astype(F32), F32(0)).astype(F32)
        active = nd > 0
        passes = np.zeros(S, np.int32)
        for _ in range(5):
            a, bb = np.zeros(S, F32), np.zeros(S, F32)
            for k in cols:
                r = md - d[:, k]
                rd = r.astype(np.float64)
                core = (rd < huber) & (rd > -huber)
                tail = (a.astype(np.float64) + np.where(r > 0, huber, -1 * huber)).astype(F32)
                a = np.where(dv[:, k], np.where(core, a + F32(2) * r, tail), a)
                bb = np.where(dv[:, k] & core, bb + F32(2), bb)
            delta = ((-a).astype(np.float64) / (bb.astype(np.float64) + 10.0)).astype(F32)
            md = np.where(active, md + delta, md)
            passes += active
            dd = delta.astype(np.float64)
            active = active & ~((dd < 0.01) & (dd > -0.01))
        # the list's length at the start of every quad of the window, and what the quad adds (k_update_seeds clamps there)
        run = np.cumsum(dv, 1)
        start = np.concatenate([np.zeros((S, 1), np.int64), run[:, 3:-1:4]], 1)
        add = run[:, 3::4] - start
    un = before["stable"] == 0
    return {"cnt": cnt, "nd": nd, "sum": total, "moved": moved, "unstable": un, "x": x, "y": y, "mean_intensity": mi,
            "mean_depth": md, "stable": np.where(un, moved.astype(np.float64) < 0.2, True), "passes": passes,
            "quad_start": start, "quad_add": add}


def census(ob, cam, img, dep, owner, huber=None):
    """PortOracle stage by stage; owner: the design, or one per sweep.  Asserts that the labels after every update_pixels equal
    the design and that restate() equals the oracle's seed table bit for bit; -> per sweep the dict of restate() with
    n_over, n_rest (what dsm_debug_tier_counts must say) added"""
    designs = owner if isinstance(owner, (list, tuple)) else [owner] * 3
    if huber is None:
        huber = 0.05 if cam.rgbd else 0.4  # fusion_functions.h:13-21: the constant set the camera selects
    orc = ob.PortOracle(cam)
    out = []
    try:
        orc.set_frame(img, dep)
        orc.stage("initialize_seeds")
        for sweep in range(3):
            orc.stage("update_pixels")
            lab, before = orc.labels().copy(), orc.seeds().copy()
            bad = int((lab != designs[sweep]).sum())
            assert bad == 0, f"sweep {sweep}: {bad} labels off the design, first at {np.argwhere(lab != designs[sweep])[:3].tolist()}"
            orc.stage("update_seeds")
            after = orc.seeds().copy()
            r = restate(cam, lab, img, dep, before, huber)
            un = r["unstable"]
            for f in ("x", "y", "mean_intensity", "mean_depth"):
                want = np.where(un, r[f], before[f]).astype(F32)
                assert np.array_equal(want.view(np.int32), after[f].view(np.int32)), \
                    f"sweep {sweep}: the restatement's {f} differs at seeds {np.flatnonzero(want.view(np.int32) != after[f].view(np.int32))[:5]}"
            assert np.array_equal(r["stable"], after["stable"] != 0), f"sweep {sweep}: stable flags"
            finite = r["sum"] != np.inf
            r["over"] = un & (r["nd"] >= CAP) & finite
            r["rest"] = un & (r["nd"] > 0) & (r["nd"] < CAP) & finite & (r["passes"] > 1)
            r["settled"] = un & ~finite
            r["n_over"], r["n_rest"] = int(r["over"].sum()), int(r["rest"].sum())
            out.append(r)
    finally:
        orc.close()
    return out


def _waves(S):
    return [slice(b, min(b + 64, S)) for b in range(0, S, 64)]


def check_family(ob, cam, family):
    """the censuses [variant][sweep] of a family, with the family's own conditions asserted; and a dict of what was counted"""
    out, seen = [], []
    for v, (img, dep, owner) in enumerate(frames(cam, family)):
        c = census(ob, cam, img, dep, owner)
        tag = (family, v, cam.width, cam.height)
        c0 = c[0]
        S = len(c0["cnt"])
        info = {"n_over": [r["n_over"] for r in c], "n_rest": [r["n_rest"] for r in c],
                "stable_after": [int(r["stable"].sum()) for r in c]}
        if family == "sizes":
            greys = seed_greys(cam, v)
            info["n225_at_255"] = int(((c0["cnt"] == 225) & (greys == 255)).sum())
            info["sizes"] = {n: int((c0["cnt"] == n).sum()) for n in SIZES}
            info["largest_sum"] = int((c0["cnt"] * greys.astype(np.int64)).max())
            assert info["n225_at_255"] >= 8 and info["largest_sum"] == 57375, (tag, info)
            assert min(info["sizes"].values()) >= 1, (tag, info["sizes"])
        if family == "lists":
            bigs = big_seeds(cam, v)
            info["per_m"] = {m: int((c0["nd"][bigs] == m).sum()) for m in LIST_M}
            assert min(info["per_m"].values()) >= 4, (tag, info["per_m"])
            assert (c0["cnt"][bigs] >= 100).all(), tag  # (225; 100 in the corner the image clips most)
            info["waves_with_all_four"] = sum(bool(c0["over"][w].any() and c0["settled"][w].any() and (c0["cnt"][w] == 1).any()
                                                   and (c0["nd"][w] == 0).any()) for w in _waves(S))
            assert info["waves_with_all_four"] >= 1, tag
            q = {(int(s), int(a)) for s, a in zip(c0["quad_start"].ravel(), c0["quad_add"].ravel()) if 121 <= s <= 123 and s + a >= CAP}
            info["quads_over_the_cap"] = sorted(q)
            assert {s for s, _ in q} == {121, 122, 123}, (tag, q)
            # m = 121 .. 127: the list that reaches its final length in the LAST quad it touches (placement 1) and the one that is
            # complete early and followed by members without depth (0) or with and without (2), each m in both ways
            places = _lists_build(cam, v, False)[3]
            info["placements"] = {m: sorted({pl for mm, pl in places.values() if mm == m}) for m in range(121, 128)}
            assert all(1 in pl and (0 in pl or 2 in pl) for pl in info["placements"].values()), (tag, info["placements"])
            assert info["n_over"][0] >= 20, (tag, info)
        if family == "lists_long":
            assert info["n_over"][0] >= 200, (tag, info)
        if family == "lists_inf":
            bigs = big_seeds(cam, v)
            info["per_m"] = {m: int((c0["nd"][bigs] == m).sum()) for m in INF_M}
            assert min(info["per_m"].values()) >= 4 and c0["settled"][bigs].all() and not c0["over"][bigs].any(), (tag, info)
        if family == "passes":
            info["per_pass_count"] = {p: int(((c0["passes"] == p) & (c0["nd"] < CAP)).sum()) for p in range(1, 6)}
            assert min(info["per_pass_count"][p] for p in range(2, 6)) >= 10 and info["per_pass_count"][1] >= 10, (tag, info)
            info["lengths"] = {n: int((c0["nd"] == n).sum()) for n in PASS_L}
            info["queued_lengths"] = {n: int(((c0["nd"] == n) & c0["rest"]).sum()) for n in PASS_L}
            assert min(info["lengths"].values()) >= 1 and info["n_over"] == [0, 0, 0], (tag, info)
            assert info["n_rest"][0] == sum(info["per_pass_count"][p] for p in range(2, 6)), (tag, info)
            mixed = 0
            for w in _waves(S):
                rest, nd = c0["rest"][w], c0["nd"][w]
                q = np.flatnonzero(rest)
                interleaved = len(q) and (~rest[:q[-1]]).any()  # an unqueued seed before a queued one: queue order != seed order
                mixed += bool(interleaved and (nd[q] == 123).sum() >= 1 and (nd[q] <= 8).sum() >= 3)
            info["waves_123_among_short"] = mixed
            assert mixed >= 1, (tag, info)
        if family == "stable":
            info["probes_left"] = int((owner[1] != owner[0]).sum())
            left = owner[0][owner[1] != owner[0]]  # the seeds whose probe left in sweep 1
            info["probes_left_on_float_0.2"] = int((c0["moved"][left] == F32(0.2)).sum())
            info["probes_kept"] = int(sum(owner[1][cy_ + dy, cx_ + 4] == s_ and img[cy_ + dy, cx_ + 4] == img[cy_, cx_] + PROBE
                                          for s_, (cx_, cy_) in enumerate(zip(*centres(cam))) if c0["cnt"][s_] == 225 for dy in range(-6, 7)))
            assert info["probes_left"] >= 2 and info["probes_kept"] >= 2 and 0 < info["stable_after"][1] < S, (tag, info)
            m = c0["moved"].astype(np.float64)
            near = np.abs(m - 0.2) <= 1e-5
            info["at_or_above"], info["below"] = int((near & (m >= 0.2)).sum()), int((near & (m < 0.2)).sum())
            info["on_float_0.2"] = int((c0["moved"] == F32(0.2)).sum())
            info["on_float_below"] = int((c0["moved"] == np.nextafter(F32(0.2), F32(0))).sum())
            info["by_centroid"] = int((near & (c0["mean_intensity"] == np.round(c0["mean_intensity"]))).sum())
            assert info["at_or_above"] >= 10 and info["below"] >= 10, (tag, info)
            assert 0 < info["stable_after"][0] < S, (tag, info)
        if family == "scan":
            info.update(scan_census(ob, cam, v))
            px_, py_ = PHASES[v]
            kinds = info["kinds"]
            assert info["share"] >= 0.8 and info["no_depth_at_all"] >= 1, (tag, info)
            assert kinds["first"] >= 30 and kinds["row15"] >= 2 and kinds["empty"] >= 1, (tag, info)
            assert info["row15_changed_by_stopping_early"] == kinds["row15"], (tag, info)
            assert kinds["pair"] >= (8 if py_ == 0 else 0) and info["pairs_changed_by_swap"] == kinds["pair"], (tag, info)
            assert kinds["mirrored"] >= (4 if px_ == 1 else 0), (tag, info)
            assert info["first_in_tell_tale_row"] >= 2 and info["first_in_column_15"] >= 2 and info["first_rows"] == list(range(1, 9)), (tag, info)
            assert info["clipped_left_or_top"] >= (4 if px_ == 0 or py_ == 0 else 0), (tag, info)
            # (two different depths, the earlier row holding the later column: in the three variants that have pairs or mirrored seeds)
            assert info["earlier_row_later_column"] >= (4 if py_ == 0 or px_ == 1 else 0), (tag, info)
            if cam.width % 8 == 0 and px_ == 1:
                assert info["last_column_unseen"] >= 4, (tag, info)
            if cam.height % 8 == 0 and py_ == 1:
                assert info["last_row_unseen"] >= 8, (tag, info)
        if family == "drift":
            info["changed"] = [int((owner[t] != owner[t - 1]).sum()) for t in (1, 2)]
            info["old_seed_stable"] = [int((c[t - 1]["stable"][owner[t - 1]] & (owner[t] != owner[t - 1]) & (owner[t - 1] >= 0)).sum()) for t in (1, 2)]
            assert info["changed"][0] >= 50 and info["changed"][1] >= 10 and sum(info["old_seed_stable"]) >= 10, (tag, info)
            for t in (0, 1):  # sweeps 1 and 2 skip some seeds and recompute others
                assert 0 < info["stable_after"][t] < S, (tag, info)
        out.append(c)
        seen.append(info)
    if family == "scan":  # over the variants every kind occurs
        for kind in SCAN_KINDS:
            assert sum(i["kinds"][kind] for i in seen) >= 4, (kind, [i["kinds"] for i in seen])
    if family == "stable":
        assert sum(i["on_float_0.2"] for i in seen) >= 1 and sum(i["on_float_below"] for i in seen) >= 1, seen
        assert sum(i["by_centroid"] for i in seen) >= 10, seen
        assert sum(i["probes_left_on_float_0.2"] for i in seen) >= 1, seen  # (`<=` at the comparison would keep that probe)
    return out, seen


# ----------------------------------------------------------------------------------------------------------------------
# replays

def twice(fr, pose=None):
    """every variant fed twice: reference index 0, then 1 -> [(image, depth, pose, ref)]"""
    pose = POSE if pose is None else pose
    return [(img, dep, pose, ref) for img, dep, _ in fr for ref in (0, 1)]


def lockstep(fr, shift=0, pose=None):
    """the variants (rotated by shift) as frames of one handle -> [(image, depth, pose, ref)]"""
    pose = POSE if pose is None else pose
    fr = fr[shift:] + fr[:shift]
    return [(img, dep, pose, t) for t, (img, dep, _) in enumerate(fr)]


# what the recipes gave when they were written, per variant 0..3 (n_over, n_rest: per variant, by sweep); pick_left_open: pixels
# the fp32 filter of pick_seed_fast left undecided over the family fed twice (tests/hostemu.cpp)
MEASURED = {'drift': {(160, 96): {'changed': [[236, 52], [216, 48], [270, 60], [190, 42]],
                       'n_over': [[60, 55, 40], [59, 50, 36], [59, 59, 45], [59, 46, 32]],
                       'n_rest': [[105, 105, 25], [119, 119, 26], [101, 101, 24], [117, 117, 21]],
                       'old_seed_stable': [[14, 0], [12, 0], [15, 0], [11, 0]],
                       'pick_left_open': 0},
           (166, 103): {'changed': [[236, 52], [216, 48], [270, 60], [190, 42]],
                        'n_over': [[61, 56, 40], [60, 36, 36], [60, 55, 45], [60, 38, 32]],
                        'n_rest': [[102, 102, 23], [103, 104, 17], [108, 108, 25], [112, 112, 19]],
                        'old_seed_stable': [[14, 0], [12, 0], [15, 0], [11, 0]],
                        'pick_left_open': 0}},
 'lists': {(160, 96): {'n_over': [[32, 5, 0], [32, 4, 0], [32, 8, 0], [32, 8, 0]],
                       'n_rest': [[20, 7, 0], [116, 110, 0], [114, 110, 0], [112, 105, 0]],
                       'pick_left_open': 0,
                       'placements': [{121: [0, 1, 2],
                                       122: [0, 1, 2],
                                       123: [0, 1, 2],
                                       124: [0, 1, 2],
                                       125: [0, 1, 2],
                                       126: [0, 1, 2],
                                       127: [0, 1, 2]},
                                      {121: [0, 1, 2],
                                       122: [0, 1, 2],
                                       123: [0, 1, 2],
                                       124: [0, 1, 2],
                                       125: [0, 1, 2],
                                       126: [0, 1, 2],
                                       127: [0, 1, 2]},
                                      {121: [0, 1, 2],
                                       122: [0, 1, 2],
                                       123: [0, 1, 2],
                                       124: [0, 1, 2],
                                       125: [0, 1, 2],
                                       126: [0, 1, 2],
                                       127: [0, 1, 2]},
                                      {121: [0, 1, 2],
                                       122: [0, 1, 2],
                                       123: [0, 1, 2],
                                       124: [0, 1, 2],
                                       125: [0, 1, 2],
                                       126: [0, 1, 2],
                                       127: [0, 1, 2]}],
                       'quads_over_the_cap': [(121, 3), (121, 4), (122, 2), (122, 3), (122, 4), (123, 1), (123, 2), (123, 3),
                                              (123, 4)]},
           (166, 103): {'n_over': [[33, 6, 0], [32, 0, 0], [32, 6, 0], [32, 4, 0]],
                        'n_rest': [[20, 7, 0], [117, 106, 0], [112, 102, 0], [119, 110, 0]],
                        'pick_left_open': 0,
                        'placements': [{121: [0, 1, 2],
                                        122: [0, 1, 2],
                                        123: [0, 1, 2],
                                        124: [0, 1, 2],
                                        125: [0, 1, 2],
                                        126: [0, 1, 2],
                                        127: [0, 1, 2]},
                                       {121: [0, 1, 2],
                                        122: [0, 1, 2],
                                        123: [0, 1, 2],
                                        124: [0, 1, 2],
                                        125: [0, 1, 2],
                                        126: [0, 1, 2],
                                        127: [0, 1, 2]},
                                       {121: [0, 1, 2],
                                        122: [0, 1, 2],
                                        123: [0, 1, 2],
                                        124: [0, 1, 2],
                                        125: [0, 1, 2],
                                        126: [0, 1, 2],
                                        127: [0, 1, 2]},
                                       {121: [0, 1, 2],
                                        122: [0, 1, 2],
                                        123: [0, 1, 2],
                                        124: [0, 1, 2],
                                        125: [0, 1, 2],
                                        126: [0, 1, 2],
                                        127: [0, 1, 2]}],
                        'quads_over_the_cap': [(121, 3), (121, 4), (122, 2), (122, 3), (122, 4), (123, 1), (123, 2),
                                               (123, 3), (123, 4)]}},
 'lists_inf': {(160, 96): {'n_over': [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
                           'n_rest': [[105, 105, 0], [106, 106, 0], [103, 103, 0], [124, 124, 0]],
                           'pick_left_open': 0},
               (166, 103): {'n_over': [[1, 1, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
                            'n_rest': [[112, 112, 0], [114, 114, 0], [107, 107, 0], [109, 109, 0]],
                            'pick_left_open': 0}},
 'lists_long': {'n_over': [[211, 28, 0], [210, 27, 0], [210, 27, 0], [210, 23, 0]]},
 'passes': {(160, 96): {'n_over': [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
                        'n_rest': [[136, 105, 0], [135, 104, 0], [133, 102, 0], [133, 101, 0]],
                        'per_pass_count': [{1: 104, 2: 16, 3: 40, 4: 42, 5: 38}, {1: 105, 2: 15, 3: 40, 4: 45, 5: 35},
                                           {1: 107, 2: 14, 3: 39, 4: 43, 5: 37}, {1: 107, 2: 14, 3: 40, 4: 42, 5: 37}],
                        'pick_left_open': 0},
            (166, 103): {'n_over': [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
                         'n_rest': [[136, 105, 0], [135, 93, 0], [133, 99, 0], [135, 98, 0]],
                         'per_pass_count': [{1: 104, 2: 16, 3: 40, 4: 45, 5: 35}, {1: 105, 2: 15, 3: 40, 4: 41, 5: 39},
                                            {1: 107, 2: 14, 3: 39, 4: 41, 5: 39}, {1: 105, 2: 16, 3: 40, 4: 43, 5: 36}],
                         'pick_left_open': 0}},
 'scan': {(160, 96): {'changed_by_reversal': [56, 56, 56, 56],
                      'clipped_left_or_top': [13, 0, 9, 4],
                      'crafted': [58, 58, 58, 58],
                      'earlier_row_later_column': [9, 6, 14, 0],
                      'first_in_column_15': [6, 6, 5, 6],
                      'first_in_tell_tale_row': [6, 6, 6, 8],
                      'kinds': [{'empty': 2, 'first': 47, 'mirrored': 0, 'pair': 9, 'row15': 2},
                                {'empty': 2, 'first': 50, 'mirrored': 6, 'pair': 0, 'row15': 2},
                                {'empty': 2, 'first': 42, 'mirrored': 6, 'pair': 8, 'row15': 2},
                                {'empty': 2, 'first': 56, 'mirrored': 0, 'pair': 0, 'row15': 2}],
                      'last_column_unseen': [0, 6, 6, 0],
                      'last_row_unseen': [0, 10, 0, 10],
                      'n_over': [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
                      'n_rest': [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
                      'no_depth_at_all': [4, 17, 12, 12],
                      'pairs_changed_by_swap': [9, 0, 8, 0],
                      'pick_left_open': 0,
                      'row15_changed_by_stopping_early': [2, 2, 2, 2]},
          (166, 103): {'changed_by_reversal': [56, 56, 56, 56],
                       'clipped_left_or_top': [13, 0, 9, 4],
                       'crafted': [58, 58, 58, 58],
                       'earlier_row_later_column': [9, 6, 14, 0],
                       'first_in_column_15': [6, 6, 5, 6],
                       'first_in_tell_tale_row': [6, 6, 6, 8],
                       'kinds': [{'empty': 2, 'first': 47, 'mirrored': 0, 'pair': 9, 'row15': 2},
                                 {'empty': 2, 'first': 50, 'mirrored': 6, 'pair': 0, 'row15': 2},
                                 {'empty': 2, 'first': 42, 'mirrored': 6, 'pair': 8, 'row15': 2},
                                 {'empty': 2, 'first': 56, 'mirrored': 0, 'pair': 0, 'row15': 2}],
                       'last_column_unseen': [0, 0, 0, 0],
                       'last_row_unseen': [0, 0, 0, 0],
                       'n_over': [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
                       'n_rest': [[0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]],
                       'no_depth_at_all': [4, 17, 12, 12],
                       'pairs_changed_by_swap': [9, 0, 8, 0],
                       'pick_left_open': 0,
                       'row15_changed_by_stopping_early': [2, 2, 2, 2]}},
 'sizes': {(160, 96): {'n_over': [[40, 21, 0], [37, 19, 0], [35, 20, 0], [37, 20, 0]],
                       'n_rest': [[121, 121, 0], [126, 125, 0], [130, 129, 0], [122, 122, 0]],
                       'pick_left_open': 0,
                       'sizes': [{1: 2, 2: 2, 63: 7, 64: 13, 65: 2, 123: 3, 124: 3, 125: 3, 224: 3, 225: 16},
                                 {1: 2, 2: 3, 63: 8, 64: 18, 65: 2, 123: 3, 124: 3, 125: 2, 224: 3, 225: 15},
                                 {1: 3, 2: 4, 63: 6, 64: 20, 65: 3, 123: 3, 124: 3, 125: 3, 224: 2, 225: 13},
                                 {1: 3, 2: 3, 63: 9, 64: 19, 65: 5, 123: 2, 124: 3, 125: 3, 224: 3, 225: 14}]},
           (166, 103): {'n_over': [[41, 22, 0], [38, 5, 0], [36, 16, 0], [38, 12, 0]],
                        'n_rest': [[114, 114, 0], [110, 108, 0], [114, 114, 0], [118, 118, 0]],
                        'pick_left_open': 0,
                        'sizes': [{1: 2, 2: 2, 63: 7, 64: 23, 65: 2, 123: 3, 124: 3, 125: 3, 224: 3, 225: 16},
                                  {1: 2, 2: 3, 63: 8, 64: 18, 65: 2, 123: 3, 124: 3, 125: 2, 224: 3, 225: 30},
                                  {1: 3, 2: 4, 63: 6, 64: 25, 65: 3, 123: 3, 124: 3, 125: 3, 224: 2, 225: 18},
                                  {1: 3, 2: 3, 63: 9, 64: 21, 65: 5, 123: 2, 124: 3, 125: 3, 224: 3, 225: 23}]}},
 'stable': {(160, 96): {'at_or_above': [19, 21, 18, 17],
                        'below': [26, 24, 27, 28],
                        'by_centroid': [20, 19, 20, 20],
                        'n_over': [[60, 34, 2], [59, 35, 0], [59, 32, 2], [59, 31, 1]],
                        'n_rest': [[123, 121, 4], [112, 113, 8], [127, 122, 5], [132, 129, 6]],
                        'on_float_0.2': [2, 1, 1, 3],
                        'on_float_below': [4, 6, 5, 5],
                        'pick_left_open': 0,
                        'probes_kept': [5, 5, 6, 5],
                        'probes_left': [9, 9, 8, 8],
                        'probes_left_on_float_0.2': [2, 1, 1, 1]},
            (166, 103): {'at_or_above': [19, 27, 21, 20],
                         'below': [26, 33, 29, 34],
                         'by_centroid': [20, 19, 20, 20],
                         'n_over': [[61, 35, 2], [60, 27, 0], [60, 31, 0], [60, 26, 1]],
                         'n_rest': [[123, 121, 7], [120, 118, 7], [136, 132, 7], [120, 120, 7]],
                         'on_float_0.2': [2, 1, 2, 4],
                         'on_float_below': [4, 6, 5, 5],
                         'pick_left_open': 0,
                         'probes_kept': [5, 5, 6, 5],
                         'probes_left': [9, 9, 8, 8],
                         'probes_left_on_float_0.2': [2, 1, 1, 1]}}}
