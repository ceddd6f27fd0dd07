"""Shared by tests/test_cpu_render_align_scale.py and tests/test_gpu_render_align_scale.py: inputs that take the renderer
(csrc/dsm_k_render.h) and the alignment (csrc/dsm_k_align.h) past the caps of their grids, so that every grid-stride loop makes a
second trip, and the geometries one handle is walked through so that its scratch is regrown and reused.  Every builder is
deterministic (a seeded numpy generator); the conditions that make a case worth running -- how many survivors, winners on both
sides of every trip boundary -- are counted on the host checkers alone by `*_conditions`, which both test files assert."""
import functools

import numpy as np

import align_cases as ac
import render_cases as rc

f32 = np.float32
# what one trip of a capped grid covers (the launch code of csrc/dsm_k_render.h, csrc/dsm_k_align.h, csrc/dsm_k_cloud.h)
PX_TRIP = 8192 * 256      # pixels: k_render_clear, k_render_resolve
RUN_TRIP = 4096 * 256     # records of the store's runs: k_render_setup_run
SCAN_TRIP = 1024 * 1024   # map records behind the 1024 tiles (of kCloudTile = 1024 records) k_cloud_scan takes at a time
SMALL_TRIP = 16384 * 16   # small-tier splats: k_render_splat
BIG_TRIP = 2048           # big-tier splats: k_render_splat_big
ALIGN_TRIP = 1024 * 256   # sampled pixels: k_align (kAlignMaxBlocks workgroups of 256)
SMALL_W, SMALL_AREA = 16, 256  # kRenderSmallW, kRenderSmallArea of csrc/dsm_device.h


def scaled_camera(cam, width, height, far=None):
    """`cam` with its focal lengths and centre scaled by width / cam.width"""
    s = width / cam.width
    return rc.Camera(width, height, cam.fx * s, cam.fy * s, cam.cx * s, cam.cy * s, cam.near_dist, cam.far_dist if far is None else far)


def discs(dtype, cam, u, v, z, rho, tilt, color, update_times):
    """discs whose centres lie at depth z on the ray of (fractional) pixel (u, v) of `cam` at the identity pose, rho pixels in
    radius there, with the normal (tilt_x, tilt_y, -1) normalised"""
    n = len(u)
    a = np.zeros(n, dtype)
    z = np.asarray(z, np.float64)
    a["px"], a["py"], a["pz"] = (u - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z, z
    nn = np.stack([tilt[:, 0], tilt[:, 1], -np.ones(n)], 1)
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    a["nx"], a["ny"], a["nz"] = nn.T
    a["size"] = rho * z / cam.fx
    a["color"] = color
    a["weight"] = 1.0
    a["update_times"] = update_times
    return a


def tiers(box, keep):
    """(small, big): the list render_emit puts every survivor on"""
    bw, bh = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    small = keep & (bw <= SMALL_W) & (bw * bh <= SMALL_AREA)
    return small, keep & ~small


# ------------------------------------------------------------------ 1. the pixel loops
# 2048 x 1100 = 2 252 800 pixels: rows 1024 .. 1099 (155 648 pixels) are the second trip of k_render_clear and k_render_resolve.
# The far plane is at 29 m and not CAM_96's 30: the crafted set holds discs at 29.5 .. 29.9 m that would otherwise put a hit in
# every pixel, and the case wants pixels WITHOUT one behind the trip boundary as well.  Those discs still pass render_setup
# with a box of the whole image, so the big tier walks all 2 252 800 pixels for each of them.
CAM_2048 = scaled_camera(rc.CAM_96, 2048, 1100, far=29.0)


@functools.lru_cache(maxsize=None)
def pixel_loop_records(dtype):
    """about 300 records: the crafted set for CAM_2048, two discs of 450 and 500 pixels radius, and 256 random discs of 1.5 to 60 pixels
    radius, three in four of them centred in the last 90 rows"""
    cam = CAM_2048
    rng = np.random.default_rng(31)
    crafted, _ = rc.crafted_records(dtype, cam)
    n = 256
    u = rng.uniform(0, cam.width, n)
    v = np.where(np.arange(n) % 4 != 0, rng.uniform(cam.height - 90, cam.height, n), rng.uniform(0, cam.height, n))
    rho = np.where(np.arange(n) % 3 == 0, rng.uniform(1.5, 6.0, n), rng.uniform(8.0, 60.0, n))
    rand = discs(dtype, cam, u, v, rng.uniform(0.8, 8.0, n), rho, rng.uniform(-0.8, 0.8, (n, 2)), rng.uniform(0, 255, n),
                 rng.choice(np.array([0, 2, 7], np.int32), n))
    wide = discs(dtype, cam, np.array([600.0, 1500.0]), np.array([900.0, 300.0]), np.array([5.0, 7.0]), np.array([450.0, 500.0]),
                 np.array([[0.3, 0.2], [-0.2, 0.4]]), np.array([33.0, 66.0]), np.array([7, 3], np.int32))
    out = np.concatenate([crafted, wide, rand])
    out.setflags(write=False)
    return out


def pixel_loop_conditions(planes):
    """on the checker's planes: at least 1000 pixels of the second trip hold a hit and at least 1000 do not"""
    idx = planes["index"].ravel()
    tail = idx[PX_TRIP:]
    hit, miss = int((tail >= 0).sum()), int((tail < 0).sum())
    assert idx.size > PX_TRIP + 100000 and hit >= 1000 and miss >= 1000, (idx.size, hit, miss)
    assert int((idx[:PX_TRIP] >= 0).sum()) >= 1000
    return hit, miss


# ------------------------------------------------------------------ 2. the sequence loops
N_STORE, N_MAP = 1_120_000, 1_130_000  # both above 1 048 576 + 1024
N_BIG_FAR, N_BIG_NEAR, N_DUP = 4700, 800, 300
SEQ_CAM = rc.CAM_96
# three runs that tile the store, out of store order
RUNS_3 = [(700_000, N_STORE - 700_000), (0, 300_000), (300_000, 400_000)]
RUNS_1 = [(0, N_STORE)]
UT_MIX = np.array([0, 1, 2, 3, 4, 5, 6, 9], np.int32)  # select 1 keeps 3 in 8, select 2 keeps 7 in 8


def _pick_boxes(dtype, cam, make, want, ok):
    """the first `want` records of make(n) whose render_setup box passes ok(width, height)"""
    s = make(3 * want)
    box, keep = rc.host_boxes(s, cam, rc.IDENTITY)
    good = np.flatnonzero(keep & ok(box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]))
    assert len(good) >= want, (len(good), want)
    return s[good[:want]]


@functools.lru_cache(maxsize=None)
def sequence_case(dtype):
    """The sequence case: "upload", the map to upload (N_STORE records of last_update 1 and N_MAP of last_update 0, interleaved at
    random); "store" and "live", what store_deactivate(1) makes of it (the store's records in order; the map with their slots
    dead); "map part", the records of last_update 0 in order, and "map_pos", where each sits in the map; and where the duplicate
    pairs sit.

    Small tier: discs of 0.35 to 0.9 pixels radius between 0.6 and 6 m, all over the image.  render_setup's box reaches one pixel
    beyond the disc on every side and one more for the exclusive end, so inside the image a disc of whatever size has a box of three
    pixels a side at least: these have three to six (fewer where the image's border clips them).
    Big tier (box width 17 to 24): 4700 discs behind the small ones (6.5 to 7.5 m: survivors that rarely show) and 800 in front of
    them (0.42 to 0.46 m) over the columns left of 62, tilted, so that they cut through each other and some two hundred of them show.
    Duplicates: 300 pairs between 0.5 and 0.55 m on the rays of distinct pixels right of column 63, in front of everything there.
    The first copy sits in the store below RUN_TRIP; the twin of an even pair in the store's tail above RUN_TRIP, of an odd pair in
    the live map."""
    cam = SEQ_CAM
    rng = np.random.default_rng(47)
    n = N_STORE + N_MAP

    def small(k):
        return discs(dtype, cam, rng.uniform(-0.5, cam.width - 0.5, k), rng.uniform(-0.5, cam.height - 0.5, k), rng.uniform(0.6, 6.0, k),
                     rng.uniform(0.35, 0.9, k), rng.uniform(-0.5, 0.5, (k, 2)), rng.uniform(0, 255, k), rng.choice(UT_MIX, k))

    def big_far(k):
        return discs(dtype, cam, rng.uniform(12, cam.width - 12, k), rng.uniform(12, cam.height - 12, k), rng.uniform(6.5, 7.5, k),
                     rng.uniform(6.3, 9.5, k), rng.uniform(-0.3, 0.3, (k, 2)), rng.uniform(0, 255, k), rng.choice(UT_MIX, k))

    def big_near(k):
        return discs(dtype, cam, rng.uniform(12, 50, k), rng.uniform(12, cam.height - 12, k), rng.uniform(0.42, 0.46, k),
                     rng.uniform(6.3, 9.5, k), rng.uniform(-0.6, 0.6, (k, 2)), rng.uniform(0, 255, k), rng.choice(UT_MIX[2:], k))

    everything = small(n)
    wide = lambda bw, bh: (bw >= 17) & (bw <= 24)
    bigs = np.concatenate([_pick_boxes(dtype, cam, big_far, N_BIG_FAR, wide), _pick_boxes(dtype, cam, big_near, N_BIG_NEAR, wide)])
    # positions: the big ones anywhere in store and map; the duplicates where the docstring says
    free = rng.permutation(n)
    at_big = free[:len(bigs)]
    taken = set(at_big.tolist())
    everything[at_big] = bigs[rng.permutation(len(bigs))]
    cells = [(x, y) for y in range(1, cam.height, 2) for x in range(64, cam.width, 2)]
    pick = rng.permutation(len(cells))[:N_DUP]
    du, dv = np.array([cells[i][0] for i in pick], np.float64), np.array([cells[i][1] for i in pick], np.float64)
    dup = discs(dtype, cam, du, dv, 0.5 + 0.05 * np.arange(N_DUP) / N_DUP, np.full(N_DUP, 0.6), np.zeros((N_DUP, 2)),
                rng.uniform(0, 255, N_DUP), np.full(N_DUP, 7, np.int32))

    def free_in(lo, hi, k):
        out = []
        for p in rng.permutation(np.arange(lo, hi)):
            if int(p) not in taken:
                out.append(int(p))
                taken.add(int(p))
                if len(out) == k:
                    return np.array(out)
        raise AssertionError("no room")

    first = free_in(0, RUN_TRIP, N_DUP)                      # in the store, below the trip boundary
    n_even = (N_DUP + 1) // 2
    twin = np.zeros(N_DUP, np.int64)
    twin[0::2] = free_in(RUN_TRIP, N_STORE, n_even)          # the store's tail
    twin[1::2] = free_in(N_STORE, n, N_DUP - n_even)         # the map part (position twin - N_STORE there)
    everything[first] = dup
    everything[twin] = dup
    store, part = everything[:N_STORE], everything[N_STORE:]
    store["last_update"], part["last_update"] = 1, 0
    # store_deactivate takes the LIVE records of its key (update_times > 0) and leaves their slots behind with update_times 0:
    # the store's records are all live, the zeros of the mix are the map part's, and the map keeps its length
    store["update_times"][store["update_times"] == 0] = 3
    in_store = np.zeros(n, bool)
    in_store[rng.permutation(n)[:N_STORE]] = True
    upload = np.zeros(n, dtype)
    upload[in_store], upload[~in_store] = store, part
    live = upload.copy()
    live["update_times"][in_store] = 0
    map_pos = np.flatnonzero(~in_store)
    for a in (store, part, upload, live, map_pos, first, twin):
        a.setflags(write=False)
    return {"store": store, "map part": part, "upload": upload, "live": live, "map_pos": map_pos, "dup_first": first, "dup_twin": twin}


def sequence_of(case, select, segs):
    """the runs first, then the map part"""
    runs = [case["store"][b:b + c] for b, c in segs]
    return np.concatenate(runs + [rc.keep_select(case["live"], select)])


@functools.lru_cache(maxsize=None)
def sequence_expected(dtype, which):
    """the boxed checker's planes of ("one run" | "three runs" | "map only"), computed once and left alone"""
    case = sequence_case(dtype)
    select, segs = {"one run": (2, RUNS_1), "three runs": (2, RUNS_3), "map only": (1, [])}[which]
    seq = sequence_of(case, select, segs)
    planes = rc.host_render(seq, SEQ_CAM, rc.IDENTITY, brute=False)
    for a in planes.values():
        a.setflags(write=False)
    return select, segs, len(seq), planes


def sequence_conditions(dtype):
    """Every count the case is built for, on host_boxes and the checker's index plane of the one-run render; returns them."""
    case = sequence_case(dtype)
    store, part, live = case["store"], case["map part"], case["live"]
    assert len(store) > RUN_TRIP + 1024 and len(live) > SCAN_TRIP + 1024 and (case["map_pos"] >= SCAN_TRIP + 1024).sum() > 100000
    assert rc.keep_select(live, 2).tobytes() == rc.keep_select(part, 2).tobytes()
    select, segs, n_seq, planes = sequence_expected(dtype, "one run")
    seq = sequence_of(case, select, segs)
    box, keep = rc.host_boxes(seq, SEQ_CAM, rc.IDENTITY)
    small, big = tiers(box, keep)
    bw, bh = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    assert small.sum() >= 2 * SMALL_TRIP and big.sum() >= 2 * BIG_TRIP, (small.sum(), big.sum())
    assert (np.maximum(bw, bh)[small] <= 6).all()                                   # the tiny discs
    assert ((bw[big] >= 17) & (bw[big] <= 24)).sum() >= 4500                        # the big tier as described
    big_at = np.flatnonzero(big)                                                    # ... spread through the whole sequence
    assert (big_at < RUN_TRIP).sum() > 1000 and ((big_at >= RUN_TRIP) & (big_at < N_STORE)).sum() > 50 and (big_at >= N_STORE + SCAN_TRIP // 2).sum() > 500
    winners = np.unique(planes["index"][planes["index"] >= 0])
    assert len(winners) >= 1000 and big[winners].sum() >= 100, (len(winners), big[winners].sum())
    run_w = winners[winners < N_STORE]
    map_pos = np.flatnonzero(live["update_times"] != 0)[winners[winners >= N_STORE] - N_STORE]  # positions in the map
    counts = {"small": int(small.sum()), "big": int(big.sum()), "winners": len(winners), "big winners": int(big[winners].sum()),
              "run winners below": int((run_w < RUN_TRIP).sum()), "run winners above": int((run_w >= RUN_TRIP).sum()),
              "map winners below": int((map_pos < SCAN_TRIP).sum()), "map winners above": int((map_pos >= SCAN_TRIP).sum())}
    for k in ("run winners below", "run winners above", "map winners below", "map winners above"):
        assert counts[k] >= 20, counts
    # the duplicates: both copies in the sequence, the same bytes but for last_update; the first wins, the twin never shows
    first, twin = case["dup_first"], case["dup_twin"]
    num_twin = np.where(twin < N_STORE, twin, N_STORE + np.cumsum(part["update_times"] != 0)[np.maximum(twin - N_STORE, 0)] - 1)
    assert (first < RUN_TRIP).all() and (num_twin >= RUN_TRIP).all() and len(first) >= 200
    for f in seq.dtype.names:
        if f != "last_update":
            assert seq[f][first].tobytes() == seq[f][num_twin].tobytes(), f
    won = np.isin(first, winners)
    counts["duplicate pairs that win"] = int(won.sum())
    counts["twins in the store's tail that win"] = int(won[0::2].sum())
    assert won.sum() >= 50 and won[0::2].sum() >= 25 and won[1::2].sum() >= 25 and not np.isin(num_twin, winners).any(), counts
    # selects 1 and 2 differ, the three runs change the numbering
    _, _, n3, planes3 = sequence_expected(dtype, "three runs")
    _, _, n1, planes1 = sequence_expected(dtype, "map only")
    assert n3 == n_seq and not np.array_equal(planes3["index"], planes["index"]) and np.array_equal(planes3["depth"], planes["depth"])
    assert n1 < n_seq - N_STORE and n1 > SCAN_TRIP // 4 and (planes1["index"] >= 0).mean() > 0.9
    return counts


# ------------------------------------------------------------------ 3. one handle, many geometries
CAM_1 = rc.Camera(1, 1, 40.0, 40.0, 0.0, 0.0, 0.3, 30.0)
CAM_17 = rc.Camera(17, 5, 14.5, 13.25, 8.3, 2.4, 0.3, 30.0)            # a width that is no multiple of 16
CAM_ROW = rc.Camera(8192, 1, 5800.0, 60.0, 4095.5, 0.2, 0.3, 30.0)     # kRenderMaxSide: the ray tables are largest relative to the keys
CAM_COLUMN = rc.Camera(1, 8192, 60.0, 8000.0, 0.3, 4095.5, 0.3, 30.0)
N_GROWN = 20000


@functools.lru_cache(maxsize=None)
def handle_maps(dtype):
    """"first": 100 records; "second": 5000 with last_update in {0, 1, 2} (two store runs); "grown": N_GROWN records whose last 2000
    lie in front of the others (the sequence scratch grows while the key scratch is kept: the tail of the sequence must show)"""
    rng = np.random.default_rng(59)
    first = rc.render_records(rng, 100, dtype, ut=7)
    second = rc.render_records(rng, 5000, dtype)
    second["last_update"] = np.arange(5000) % 3
    grown = rc.render_records(rng, N_GROWN, dtype)
    grown["last_update"] = 0
    tail = grown[-2000:]
    k = f32(0.5) / tail["pz"]  # along their rays to 0.5 m, the size with them; the others a metre back
    k = np.concatenate([(grown["pz"][:-2000] + f32(1.0)) / grown["pz"][:-2000], k]).astype(f32)
    for f in ("px", "py", "pz", "size"):
        grown[f] = grown[f] * k
    tail["update_times"] = 7
    out = {"first": first, "second": second, "grown": grown}
    for a in out.values():
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ 4. k_align
# 640 x 416 = 266 240 samples at stride 1: 1040 workgroups, capped to 1024.  FRAME_100's intrinsics scaled by 6.4 across and by 8
# down (its field of view, which CAM_96 covers): the samples behind the trip boundary are the rows from 409 on, and they have to
# land inside the model image to pass.
FRAME_640 = dict(width=640, height=416, fx=88.5 * 6.4, fy=91.25 * 8, cx=48.7 * 6.4, cy=26.4 * 8, near_dist=0.3, far_dist=30.0)
ALIGN_CAM = rc.CAM_96


@functools.lru_cache(maxsize=None)
def align_planes():
    depth, zm, nm = ac.random_planes(np.random.default_rng(67), FRAME_640, ALIGN_CAM)
    mm = np.clip(np.nan_to_num(depth, nan=0.0, posinf=0.0, neginf=0.0) * 1000.0, 0, 65535).astype(np.uint16)
    for a in (depth, zm, nm, mm):
        a.setflags(write=False)
    return depth, zm, nm, mm


def align_cases():
    """(T, stride, huber) of every evaluation"""
    return [(T, stride, huber) for T in (ac.IDENTITY, ac.OBLIQUE_T) for stride in (1, 2, 3) for huber in (0.01, 0.0)]


def align_conditions(fd, plane, cam, zm, nm, T, p):
    """at stride 1, on the checker's census: at least 300 passing pixels on either side of the trip boundary"""
    assert p.stride == 1 and ac.n_sampled(fd, 1) > ALIGN_TRIP + 1024
    sums, k, census, exits = ac.host_equations(fd, plane, cam, zm, nm, T, p, census=True)
    assert len(exits) == ac.n_sampled(fd, 1)  # (in sampled_index's order: row-major)
    below, above = int((exits[:ALIGN_TRIP] == ac.PASS).sum()), int((exits[ALIGN_TRIP:] == ac.PASS).sum())
    assert below >= 300 and above >= 300 and below + above == sums[28], (below, above, sums[28])
    return below, above


def own_camera(fr):
    return rc.Camera(fr["width"], fr["height"], fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["near_dist"], fr["far_dist"])
