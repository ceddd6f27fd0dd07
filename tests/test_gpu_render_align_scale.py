"""The renderer and the alignment on the GPU past the caps of their grids and across regrowth of a handle's scratch: bit for bit
against the host checkers (tests/render_host.cpp in its boxed mode, tests/align_host.cpp), as tests/test_gpu_render.py and
tests/test_gpu_align.py compare the small cases.  The inputs and the counts that make them worth running come from
tests/render_scale_cases.py; tests/test_cpu_render_align_scale.py asserts the same counts without a GPU.
  1. the pixel loops' second trip (k_render_clear, k_render_resolve): a 2048 x 1100 image
  2. the sequence loops' second trip (k_render_setup_run, k_cloud_scan with k_render_setup_map, k_render_splat,
     k_render_splat_big): 2.25 M records, store runs and map part both above 1 048 576
  3. one handle through many geometries: scratch_grow regrows and reuses the render and align scratch
  4. k_align's second trip: a 640 x 416 frame at stride 1, and dsm_align_frame on it"""
import time

import numpy as np
import pytest

import align_cases as ac
import render_cases as rc
import render_scale_cases as sc
from test_gpu_align import Model, _as_dict, _both, _params, _same_result
from test_gpu_render import _device_buffers, _read_device

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def api():
    import torch
    torch.cuda.init()  # (before the library's first HIP call, as in the other GPU suites)
    from densesurfelmapping_amd import api as api_mod
    return api_mod


def _engine(api, fr=ac.FRAME_64, cap=1 << 15):
    ff = api.FusionFunctions()
    ff.initialize(fr["width"], fr["height"], fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["far_dist"], fr["near_dist"], surfel_capacity=cap, frame_slots=2)
    return ff


def _render_is(api, ff, select, segs, cam, pose, exp, n_seq, what):
    """host destination and guarded device destination: both the checker's planes `exp`, n_surfels the sequence's length"""
    host = ff.render(select, segs, cam, pose)
    assert host["n_surfels"] == n_seq, (what, host["n_surfels"], n_seq)
    rc.same_planes(host, exp, (what, "host destination"))
    bufs = _device_buffers(api, cam)
    assert ff.render(select, segs, cam, pose, dst_ptrs={k: t.data_ptr() for k, t in bufs.items()}) == n_seq, what
    rc.same_planes(_read_device(api, cam, bufs, what), exp, (what, "device destination"))
    return host


def _check(api, ff, seq, select, segs, cam, pose, what):
    return _render_is(api, ff, select, segs, cam, pose, rc.host_render(seq, cam, pose, brute=False), len(seq), what)


# ------------------------------------------------------------------ 1. the pixel loops
def test_pixel_loops_second_trip(api):
    t0 = time.perf_counter()
    cam = sc.CAM_2048
    m = sc.pixel_loop_records(api.SURFEL_DTYPE)
    seq = rc.keep_select(m, 2)
    exp = rc.host_render(seq, cam, rc.IDENTITY, brute=False)
    hit, miss = sc.pixel_loop_conditions(exp)
    ff = _engine(api)
    ff.map_upload(m)
    got = _render_is(api, ff, 2, (), cam, rc.IDENTITY, exp, len(seq), "2048 x 1100")
    # (said once more on what the device wrote: the normal plane's 3 * i behind 2^21 pixels)
    tail = got["index"].ravel()[sc.PX_TRIP:] >= 0
    assert tail.sum() == hit and (got["normal"].reshape(-1, 3)[sc.PX_TRIP:][tail] != 0).any(axis=1).all()
    assert not got["normal"].reshape(-1, 3)[sc.PX_TRIP:][~tail].any() and not got["depth"].ravel()[sc.PX_TRIP:][~tail].any()
    ff.close()
    print("pixel loops: %d and %d pixels behind the first trip with and without a hit; %.2f s" % (hit, miss, time.perf_counter() - t0))


# ------------------------------------------------------------------ 2. the sequence loops
def test_sequence_loops_second_trip(api):
    t0 = time.perf_counter()
    dtype = api.SURFEL_DTYPE
    counts = sc.sequence_conditions(dtype)
    case = sc.sequence_case(dtype)
    t1 = time.perf_counter()
    ff = _engine(api, cap=len(case["upload"]))
    ff.map_upload(case["upload"])
    begin, n = ff.store_deactivate(1)
    assert (begin, n) == (0, sc.N_STORE) and ff.store_size() == sc.N_STORE and ff.map_size() == len(case["live"])
    # the store and the live map are what the builder says: the checker's sequences are the device's
    assert ff.store_download(0, sc.N_STORE)[0].tobytes() == case["store"].tobytes()
    assert ff.map_download().tobytes() == case["live"].tobytes()
    t2 = time.perf_counter()
    for which in ("one run", "three runs", "map only"):
        select, segs, n_seq, exp = sc.sequence_expected(dtype, which)
        _render_is(api, ff, select, segs, sc.SEQ_CAM, rc.IDENTITY, exp, n_seq, which)
    ff.close()
    t3 = time.perf_counter()
    print("sequence loops:", counts)
    print("sequence loops: %.2f s building the case and the checker's planes, %.2f s upload, deactivate and download, %.2f s for six renders"
          % (t1 - t0, t2 - t1, t3 - t2))


# ------------------------------------------------------------------ 3. one handle, many geometries
def _frame_parity(api, ff, fr, select, segs, model_cam, guess, p, what):
    """dsm_align_frame == the checker's loop fed the planes dsm_render_compose wrote for the same sequence"""
    cam = sc.own_camera(fr) if model_cam is None else model_cam
    planes = ff.render(select, segs, cam, guess, planes=("depth", "normal"))
    got = ff.align_frame(0, select, segs, guess, model_cam=model_cam, params=_params(api, p))
    plane = ff.frame_planes(0)[1]
    want = ac.host_frame(ac.frame_desc(fr, plane.shape[1]), plane, cam, planes["depth"], planes["normal"], guess, p)
    _same_result(got, _as_dict(api, want), what)
    return got, planes


def test_one_handle_many_geometries(api):
    t0 = time.perf_counter()
    dtype, fr = api.SURFEL_DTYPE, ac.FRAME_64
    maps = sc.handle_maps(dtype)
    room = ac.room_surfels(dtype).copy()
    room["last_update"] = np.where(np.arange(len(room)) % 3 == 1, 5, 0)
    ff = _engine(api, cap=max(sc.N_GROWN, len(room)) + 4096)
    # a small image and a short sequence first
    ff.map_upload(maps["first"])
    first = _check(api, ff, maps["first"], 2, (), rc.CAM_48, rc.IDENTITY, "first")
    assert (first["index"] >= 0).sum() > 100
    # a larger image, a longer sequence, two store runs: key scratch and sequence scratch both grow
    ff.map_upload(maps["second"])
    r1, r2 = ff.store_deactivate(1), ff.store_deactivate(2)
    store = ff.store_download(0, ff.store_size())[0]
    live = ff.map_download()
    assert r1[1] > 1000 and r2 == (r1[1], ff.store_size() - r1[1]) and r2[1] > 1000 and len(rc.keep_select(live, 2)) > 1000
    two_runs = [r2, r1]
    runs = np.concatenate([store[b:b + c] for b, c in two_runs])
    seq = np.concatenate([runs, rc.keep_select(live, 2)])
    got = _check(api, ff, seq, 2, two_runs, rc.CAM_96, rc.IDENTITY, "second")
    winners = np.unique(got["index"][got["index"] >= 0])
    assert (winners < len(runs)).sum() > 20 and (winners >= len(runs)).sum() > 20
    # one pixel; a width that is no multiple of 16; the longest row and the longest column (kRenderMaxSide)
    for cam in (sc.CAM_1, sc.CAM_17, sc.CAM_ROW, sc.CAM_COLUMN):
        got = _check(api, ff, seq, 2, two_runs, cam, rc.IDENTITY, ("second", cam.width, cam.height))
        assert (got["index"] >= 0).sum() >= min(cam.width * cam.height, 40)
    # a longer sequence behind a smaller image: the sequence scratch grows, the key scratch stays
    ff.map_upload(maps["grown"])
    seq = np.concatenate([runs, rc.keep_select(maps["grown"], 2)])
    got = _check(api, ff, seq, 2, two_runs, rc.CAM_48, rc.IDENTITY, "grown")
    assert len(np.unique(got["index"][got["index"] >= len(seq) - 2000])) >= 100  # (the discs in front are the sequence's tail)
    # the alignment: its own camera first (2048 model pixels), then a larger one (6144: the model planes' scratch grows while the
    # render inside the call finds its scratch as the renders above left it)
    ff.map_upload(room)
    rb, rn = ff.store_deactivate(5)
    assert rn > 1000 and ff.map_size() > 2000 and rb == r1[1] + r2[1]
    room_runs = [(rb + rn // 2, rn - rn // 2), (rb, rn // 2)]
    ff.frame_upload(0, np.zeros((fr["height"], fr["width"]), np.uint8), ac.room_depth(fr, ac.ROOM_TRUTH))
    before = (ff.store_download(0, ff.store_size())[0].tobytes(), ff.map_download().tobytes(), ff.frame_planes(0)[1].tobytes())
    guess, p = ac.ROOM_GUESS.astype(f32), ac.params(**ac.ROOM_PARAMS)
    for model_cam in (None, rc.CAM_96):
        got, planes = _frame_parity(api, ff, fr, 1, room_runs, model_cam, guess, p, ("room", model_cam is None))
        cam = sc.own_camera(fr) if model_cam is None else model_cam
        rc.same_planes(planes, rc.host_render(np.concatenate([room[room["last_update"] == 5][rn // 2:], room[room["last_update"] == 5][:rn // 2],
                                                               rc.keep_select(room[room["last_update"] == 0], 1)]), cam, guess, brute=False), "the room's model")
        dt, dr = ac.pose_error(got["pose"], ac.ROOM_TRUTH)
        assert got["status"] == api.ALIGN_CONVERGED and dt < 1e-3 and dr < 0.05, (got["status"], dt, dr)
    assert (ff.store_download(0, ff.store_size())[0].tobytes(), ff.map_download().tobytes(), ff.frame_planes(0)[1].tobytes()) == before
    # the first geometry again: the same bytes
    ff.map_upload(maps["first"])
    again = _check(api, ff, maps["first"], 2, (), rc.CAM_48, rc.IDENTITY, "first again")
    for k in api.RENDER_PLANES:
        assert again[k].tobytes() == first[k].tobytes(), k
    # dsm_align_equations on planes the caller holds, after all that
    rng = np.random.default_rng(71)
    depth, zm, nm = ac.random_planes(rng, fr, rc.CAM_70)
    model = Model(rc.CAM_70, zm, nm)
    ff.frame_upload(1, np.zeros(depth.shape, np.uint8), depth)
    for T in (ac.IDENTITY, ac.OBLIQUE_T):
        assert _both(api, ff, fr, 1, model, T, ac.params(stride=1, huber=0.01, dist_max=0.1), "equations afterwards")[28] > 300
    # nothing but scratch was written: the store and the other slot's frame as they were, the map as uploaded
    assert ff.store_download(0, ff.store_size())[0].tobytes() == before[0] and ff.frame_planes(0)[1].tobytes() == before[2]
    assert ff.map_download().tobytes() == maps["first"].tobytes()
    ff.close()
    print("one handle: %.2f s" % (time.perf_counter() - t0))


# ------------------------------------------------------------------ 4. k_align
def test_align_second_trip(api):
    t0 = time.perf_counter()
    fr, cam = sc.FRAME_640, sc.ALIGN_CAM
    depth, zm, nm, mm = sc.align_planes()
    room = ac.room_surfels(api.SURFEL_DTYPE)
    ff = _engine(api, fr, cap=len(room) + 4096)
    fd = ac.frame_desc(fr, ff.frame_pitch())
    model = Model(cam, zm.copy(), nm.copy())
    ff.frame_upload(0, np.zeros(depth.shape, np.uint8), depth)
    ff.frame_upload_u16(1, np.zeros(depth.shape, np.uint8), mm, 0.001, "multiply")
    assert np.array_equal(ff.frame(1)[1], api.depth_from_u16(mm, 0.001, "multiply"))
    small_k = ac.np_scale(cam, ac.n_sampled(ac.frame_desc(ac.FRAME_64), 1))
    for slot in (0, 1):
        plane = ff.frame_planes(slot)[1]
        for T, stride, huber in sc.align_cases():
            p = ac.params(stride=stride, huber=huber, dist_max=0.1)
            what = ("640 x 416", slot, stride, huber)
            if stride == 1 and huber > 0:
                sc.align_conditions(fd, plane, cam, zm, nm, T, p)  # passing pixels on both sides of the trip boundary
            sums, k = ff.align_equations(slot, cam, model.d_zm.data_ptr(), model.d_nm.data_ptr(), T, _params(api, p))
            want, want_k = ac.host_equations(fd, plane, cam, zm, nm, T, p)
            assert np.array_equal(sums, want), (what, sums.tolist(), want.tolist())
            assert sums[28] > 1000
            assert k == want_k == ac.np_scale(cam, ac.n_sampled(fd, stride)) and (stride > 1 or k < small_k), (what, k, want_k, small_k)
    t1 = time.perf_counter()
    # the loop on this frame: the room at 640 x 416, the model rendered by the handle's own camera (266 240 pixels as well)
    ff.map_upload(room)
    ff.frame_upload(0, np.zeros(depth.shape, np.uint8), ac.room_depth(fr, ac.ROOM_TRUTH))
    guess, p = ac.ROOM_GUESS.astype(f32), ac.params(**ac.ROOM_PARAMS)
    got, planes = _frame_parity(api, ff, fr, 1, [], None, guess, p, "room at 640 x 416")
    rc.same_planes(planes, rc.host_render(rc.keep_select(room, 1), sc.own_camera(fr), guess, brute=False), "the room's model")
    dt, dr = ac.pose_error(got["pose"], ac.ROOM_TRUTH)
    print("room corner at 640 x 416 on the GPU: status %d after %d iterations, %d pixels, rms %.3g m; %.3g mm and %.3g degrees from the truth"
          % (got["status"], got["iterations"], got["n_pixels"], got["rms"], 1e3 * dt, dr))
    assert got["status"] == api.ALIGN_CONVERGED and got["n_pixels"] > sc.ALIGN_TRIP // 2
    assert dt < 1e-3 and dr < 0.05
    ff.close()
    print("k_align: %.2f s for 24 evaluations and their checker, %.2f s for the loop" % (t1 - t0, time.perf_counter() - t1))
