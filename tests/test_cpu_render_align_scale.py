"""The inputs of tests/test_gpu_render_align_scale.py without a GPU: tests/render_scale_cases.py builds them, and every condition
that makes them worth running on the device -- hits and misses behind the pixel loops' first trip, twice a trip's worth of
survivors in either splat list, winners on both sides of every trip boundary, duplicate pairs that win across one, passing
pixels behind k_align's first trip, a room that converges at 640 x 416 -- is asserted here on the host checkers alone, so the
device tests cannot pass on nothing and a builder that drifts fails on a machine without a GPU.
  1. the pixel-loop case; boxed == brute on the same records seen by a camera an eighth the size
  2. the sequence case; boxed == brute on every 200th record
  3. the geometries one handle is walked through
  4. the alignment case: the census, the second scale, the restatement, the room"""
import numpy as np
import pytest

import align_cases as ac
import render_cases as rc
import render_scale_cases as sc

f32 = np.float32


@pytest.fixture(scope="module")
def dtype():
    from densesurfelmapping_amd import api
    return api.SURFEL_DTYPE


# ------------------------------------------------------------------ 1. the pixel loops
def test_pixel_loop_case(dtype):
    cam = sc.CAM_2048
    m = sc.pixel_loop_records(dtype)
    assert 280 <= len(m) <= 320 and cam.width * cam.height == 2252800
    assert abs(cam.fx / cam.width - rc.CAM_96.fx / rc.CAM_96.width) < 1e-6 and abs(cam.cy / cam.width - rc.CAM_96.cy / rc.CAM_96.width) < 1e-6
    seq = rc.keep_select(m, 2)
    assert len(seq) < len(m)
    planes = rc.host_render(seq, cam, rc.IDENTITY, brute=False)
    hit, miss = sc.pixel_loop_conditions(planes)
    print("pixel-loop case: %d records, behind the first trip %d pixels with a hit and %d without" % (len(seq), hit, miss))
    # both tiers take part, and boxes of the whole image are among the big ones
    box, keep = rc.host_boxes(seq, cam, rc.IDENTITY)
    small, big = sc.tiers(box, keep)
    whole = big & (box[:, 0] == 0) & (box[:, 1] == 0) & (box[:, 2] == cam.width) & (box[:, 3] == cam.height)
    assert small.sum() >= 50 and big.sum() >= 100 and whole.sum() >= 3, (small.sum(), big.sum(), whole.sum())
    # the boxes lose no hit: the same records through a camera an eighth the size (the same rays, every eighth of them)
    cam8 = sc.scaled_camera(cam, 256, 138)
    rc.same_planes(rc.host_render(seq, cam8, rc.IDENTITY, brute=False), rc.host_render(seq, cam8, rc.IDENTITY, brute=True), "an eighth")


# ------------------------------------------------------------------ 2. the sequence loops
def test_sequence_case(dtype):
    counts = sc.sequence_conditions(dtype)
    print("sequence case:", counts)
    case = sc.sequence_case(dtype)
    up = case["upload"]
    assert len(up) == sc.N_STORE + sc.N_MAP and set(np.unique(up["last_update"]).tolist()) == {0, 1}
    # what store_deactivate(1) does (k_mark_key, k_extract_marked): the live records of the key, in order; their slots dead
    moved = (up["last_update"] == 1) & (up["update_times"] > 0)
    assert moved.sum() == sc.N_STORE and up[moved].tobytes() == case["store"].tobytes()
    after = up.copy()
    after["update_times"][moved] = 0
    assert after.tobytes() == case["live"].tobytes() and up[case["map_pos"]].tobytes() == case["map part"].tobytes()
    ut = case["map part"]["update_times"]
    assert (ut == 0).mean() > 0.1 and ((ut > 0) & (ut < 5)).mean() > 0.3 and (ut >= 5).mean() > 0.3
    assert sum(c for _, c in sc.RUNS_3) == sc.N_STORE and sorted(sc.RUNS_3) != sc.RUNS_3


def test_sequence_case_boxed_equals_brute(dtype):
    case = sc.sequence_case(dtype)
    thin = sc.sequence_of(case, 2, sc.RUNS_1)[::200]
    assert len(thin) > 10000
    boxed, brute = (rc.host_render(thin, sc.SEQ_CAM, rc.IDENTITY, brute=b) for b in (False, True))
    rc.same_planes(boxed, brute, "every 200th record")
    assert (brute["index"] >= 0).mean() > 0.9


# ------------------------------------------------------------------ 3. one handle, many geometries
def test_handle_geometries(dtype):
    maps = sc.handle_maps(dtype)
    assert (len(maps["first"]), len(maps["second"]), len(maps["grown"])) == (100, 5000, sc.N_GROWN)
    assert (rc.host_render(maps["first"], rc.CAM_48, rc.IDENTITY)["index"] >= 0).sum() > 100
    live = maps["second"][maps["second"]["last_update"] == 0]
    seq = rc.keep_select(live, 2)
    for cam, least in ((sc.CAM_1, 1), (sc.CAM_17, 40), (sc.CAM_ROW, 4000), (sc.CAM_COLUMN, 4000)):
        boxed = rc.host_render(seq, cam, rc.IDENTITY, brute=False)
        rc.same_planes(boxed, rc.host_render(seq, cam, rc.IDENTITY, brute=True), (cam.width, cam.height))
        assert (boxed["index"] >= 0).sum() >= least, (cam.width, cam.height, (boxed["index"] >= 0).sum())
    assert sc.CAM_17.width % 16 and sc.CAM_ROW.width == 8192 == sc.CAM_COLUMN.height
    # the grown map: the scratch of the 5000-record render holds 5000 + 5000 / 4 + 64 records; winners lie behind that
    grown = rc.keep_select(maps["grown"], 2)
    idx = rc.host_render(grown, rc.CAM_48, rc.IDENTITY, brute=False)["index"]
    assert len(np.unique(idx[idx >= 5000 + 1250 + 64])) >= 100


# ------------------------------------------------------------------ 4. the alignment
def test_align_case_census_and_scale():
    depth, zm, nm, mm = sc.align_planes()
    fr, cam = sc.FRAME_640, sc.ALIGN_CAM
    fd = ac.frame_desc(fr)
    assert ac.n_sampled(fd, 1) == 266240 and (ac.n_sampled(fd, 1) + 255) // 256 == 1040
    for T in (ac.IDENTITY, ac.OBLIQUE_T):
        below, above = sc.align_conditions(fd, depth, cam, zm, nm, T, ac.params(stride=1, huber=0.01, dist_max=0.1))
        print("640 x 416 at stride 1: %d passing pixels below the trip boundary, %d at or above it" % (below, above))
    ks = {}
    for stride in (1, 2, 3):
        _, ks[stride] = ac.host_equations(fd, depth, cam, zm, nm, ac.IDENTITY, ac.params(stride=stride, dist_max=0.1))
        assert ks[stride] == ac.np_scale(cam, ac.n_sampled(fd, stride))
    small = ac.np_scale(cam, ac.n_sampled(ac.frame_desc(ac.FRAME_64), 1))
    assert ks[1] < small and ks[1] < ks[3]  # a second (and third) fixed-point scale
    # the uint16 frame is the same scene to a millimetre: it passes about as often
    from densesurfelmapping_amd import api
    d16 = api.depth_from_u16(mm, 0.001, "multiply")
    sc.align_conditions(fd, d16, cam, zm, nm, ac.OBLIQUE_T, ac.params(stride=1, huber=0.01, dist_max=0.1))


def test_align_case_equals_restatement():
    depth, zm, nm, _ = sc.align_planes()
    fd = ac.frame_desc(sc.FRAME_640)
    p = ac.params(stride=1, huber=0.01, dist_max=0.1)
    sums, k, census, exits = ac.host_equations(fd, depth, sc.ALIGN_CAM, zm, nm, ac.OBLIQUE_T, p, census=True)
    want, want_exits, _ = ac.np_equations(fd, depth, sc.ALIGN_CAM, zm, nm, ac.OBLIQUE_T, p)
    assert np.array_equal(exits, want_exits) and [int(v) for v in sums] == want and census[ac.PASS] == sums[28] > 1000


def test_align_case_room_converges(dtype):
    fr = sc.FRAME_640
    cam = sc.own_camera(fr)
    surfels = ac.room_surfels(dtype)
    guess = ac.ROOM_GUESS.astype(f32)
    model = rc.host_render(rc.keep_select(surfels, 1), cam, guess, brute=False)
    assert (model["depth"] > 0).mean() > 0.9
    r = ac.host_frame(ac.frame_desc(fr), ac.room_depth(fr, ac.ROOM_TRUTH), cam, model["depth"], model["normal"], guess, ac.params(**ac.ROOM_PARAMS))
    pose = np.array(r.pose16, f32).reshape(4, 4).T
    dt, dr = ac.pose_error(pose, ac.ROOM_TRUTH)
    print("room corner at 640 x 416: status %d after %d iterations, %d pixels, rms %.3g m; %.3g mm and %.3g degrees from the truth"
          % (r.status, r.iterations, r.n_pixels, r.rms, 1e3 * dt, dr))
    assert r.status == ac.CONVERGED and r.n_pixels > sc.ALIGN_TRIP // 2
    assert dt < 1e-3 and dr < 0.05
