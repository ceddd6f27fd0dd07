"""The frame-to-map alignment on the GPU (dsm_align_equations, dsm_align_frame, dsm_surfel_map_align_last): the 29 sums word for
word, and every field of the loop's result bit for bit, against the checker tests/align_host.cpp, which evaluates the same
csrc/dsm_align.h functions as the kernel and which tests/test_cpu_align.py pins to a numpy restatement of the definition."""
import ctypes as C

import numpy as np
import pytest

import align_cases as ac
import render_cases as rc

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


def _params(api, p):
    return api._AlignParams.from_buffer_copy(bytes(p))


def _own_camera(fr):
    return rc.Camera(fr["width"], fr["height"], fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["near_dist"], fr["far_dist"])


class Model:
    """model planes in device memory (torch), and on the host for the checker"""

    def __init__(self, cam, zm, nm):
        import torch
        self.cam, self.zm, self.nm = cam, np.ascontiguousarray(zm, f32), np.ascontiguousarray(nm, f32)
        self.d_zm, self.d_nm = torch.from_numpy(self.zm).cuda(), torch.from_numpy(self.nm).cuda()
        torch.cuda.synchronize()


def _upload(ff, slot, depth):
    ff.frame_upload(slot, np.zeros(depth.shape, np.uint8), np.ascontiguousarray(depth, f32))


def _both(api, ff, fr, slot, model, T, p, what):
    """dsm_align_equations == the checker over the slot's plane as it is (pad columns included); returns the sums"""
    sums, k = ff.align_equations(slot, model.cam, model.d_zm.data_ptr(), model.d_nm.data_ptr(), T, _params(api, p))
    plane = ff.frame_planes(slot)[1]
    want, want_k = ac.host_equations(ac.frame_desc(fr, plane.shape[1]), plane, model.cam, model.zm, model.nm, T, p)
    assert k == want_k, what
    assert np.array_equal(sums, want), (what, sums.tolist(), want.tolist())
    return sums


# ------------------------------------------------------------------ 1. equations parity: the crafted set
def test_equations_crafted(api):
    ff = _engine(api)
    depth, zm, nm, cases = ac.crafted_case()
    _upload(ff, 0, depth)
    assert ff.frame_pitch() >= 64
    model = Model(rc.CAM_70, zm, nm)
    passed = 0
    for T, _ in cases + [(ac.IDENTITY, {}), (ac.OBLIQUE_T, {})]:
        for stride in (1, 2, 3):
            for huber in (ac.CRAFTED_PARAMS["huber"], 0.0):
                p = ac.params(**dict(ac.CRAFTED_PARAMS, stride=stride, huber=huber))
                passed += _both(api, ff, ac.FRAME_64, 0, model, T, p, ("crafted", stride, huber))[28]
    assert passed > 100
    ff.close()


# ------------------------------------------------------------------ 2. equations parity: random planes, every upload path, pad columns
@pytest.mark.parametrize("fr,cam", [(ac.FRAME_64, rc.CAM_96), (ac.FRAME_100, rc.CAM_70), (ac.FRAME_100, rc.CAM_96)], ids=["64x32-96", "100x52-70", "100x52-96"])
def test_equations_random(api, fr, cam):
    rng = np.random.default_rng(21)
    ff = _engine(api, fr)
    pitch = ff.frame_pitch()
    if fr is ac.FRAME_100:
        assert pitch == 128  # 5200 pixels, no multiple of 64, 28 pad columns a row
    depth, zm, nm = ac.random_planes(rng, fr, cam)
    model = Model(cam, zm, nm)
    _upload(ff, 0, depth)
    # slot 1: the same scene from a uint16 frame (millimetres), so the slot plane is read whatever path wrote it
    mm = np.clip(np.nan_to_num(depth, nan=0.0, posinf=0.0, neginf=0.0) * 1000.0, 0, 65535).astype(np.uint16)
    ff.frame_upload_u16(1, np.zeros(depth.shape, np.uint8), mm, 0.001, "multiply")
    assert np.array_equal(ff.frame(1)[1], api.depth_from_u16(mm, 0.001, "multiply"))
    counts = []
    for slot in (0, 1):
        for T in (ac.IDENTITY, ac.OBLIQUE_T):
            for stride in (1, 2, 3):
                for huber in (0.01, 0.0):
                    p = ac.params(stride=stride, huber=huber, dist_max=0.1)
                    counts.append(_both(api, ff, fr, slot, model, T, p, ("random", slot, stride, huber))[28])
    assert min(counts) > 20 and max(counts) > 300  # (the comparison is not an empty one: the checker's own counts)
    # pad columns filled with depths that would pass: the sums do not change
    p = ac.params(stride=1, huber=0.01, dist_max=0.1)
    before = _both(api, ff, fr, 0, model, ac.OBLIQUE_T, p, "before the pad columns are filled")
    img, plane = ff.frame_planes(0)
    if pitch > fr["width"]:
        plane[:, fr["width"]:] = 2.0
        ff.frame_planes(0, depth=plane)
        assert (ff.frame_planes(0)[1][:, fr["width"]:] == 2.0).all()
        after = _both(api, ff, fr, 0, model, ac.OBLIQUE_T, p, "pad columns filled")
        assert np.array_equal(before, after)
    # a frame in which no pixel passes: 29 zeros
    _upload(ff, 1, np.zeros_like(depth))
    assert not _both(api, ff, fr, 1, model, ac.IDENTITY, p, "empty frame").any()
    empty = Model(cam, np.zeros_like(zm), nm)
    assert not _both(api, ff, fr, 0, empty, ac.IDENTITY, p, "empty model").any()
    ff.close()


# ------------------------------------------------------------------ 3. the 29 words are cleared before every evaluation
def test_sums_are_cleared_every_time(api):
    rng = np.random.default_rng(22)
    fr, cam = ac.FRAME_100, rc.CAM_96
    ff = _engine(api, fr)
    depth, zm, nm = ac.random_planes(rng, fr, cam)
    model = Model(cam, zm, nm)
    _upload(ff, 0, depth)
    p1, p2 = ac.params(stride=1, huber=0.01, dist_max=0.1), ac.params(stride=2, huber=0.0, dist_max=0.2)
    a = _both(api, ff, fr, 0, model, ac.OBLIQUE_T, p1, "first")
    b = _both(api, ff, fr, 0, model, ac.OBLIQUE_T, p1, "the same call again")
    c = _both(api, ff, fr, 0, model, ac.IDENTITY, p2, "another call")
    d = _both(api, ff, fr, 0, model, ac.OBLIQUE_T, p1, "the first call after another")
    assert a[28] > 1000 and np.array_equal(a, b) and np.array_equal(a, d) and not np.array_equal(a, c)
    ff.close()


# ------------------------------------------------------------------ 4. the loop
def _as_dict(api, r):
    return api.align_result(api._AlignResult.from_buffer_copy(bytes(r)))


def _same_result(got, want, what):
    for k in ("pose", "T", "sums"):
        assert got[k].tobytes() == want[k].tobytes(), (what, k, got[k], want[k])
    for k in ("status", "iterations", "n_pixels", "scale_log2"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.float64(got["rms"]).tobytes() == np.float64(want["rms"]).tobytes(), (what, got["rms"], want["rms"])


def _frame_parity(api, ff, fr, select, segs, model_cam, guess, p, what):
    """dsm_align_frame == the checker's loop fed the planes dsm_render_compose wrote for the same sequence"""
    cam = _own_camera(fr) if model_cam is None else model_cam
    planes = ff.render(select, segs, cam, guess, planes=("depth", "normal"))
    got = ff.align_frame(0, select, segs, guess, model_cam=model_cam, params=_params(api, p))
    plane = ff.frame_planes(0)[1]
    want = ac.host_frame(ac.frame_desc(fr, plane.shape[1]), plane, cam, planes["depth"], planes["normal"], guess, p)
    _same_result(got, _as_dict(api, want), what)
    return got


def _room_engine(api, planes=ac.ROOM_PLANES):
    """the room's surfels, a third of them in the store (two runs), the rest in the map"""
    ff = _engine(api)
    s = ac.room_surfels(api.SURFEL_DTYPE, planes)
    s["last_update"] = np.arange(len(s)) % 3
    ff.map_upload(s)
    ff.store_deactivate(1)
    n = ff.store_size()
    assert n > 1000 and ff.map_size() > 2000
    return ff, [(n // 2, n - n // 2), (0, n // 2)]


def test_frame_room_corner(api):
    fr = ac.FRAME_64
    ff, segs = _room_engine(api)
    _upload(ff, 0, ac.room_depth(fr, ac.ROOM_TRUTH))
    guess = ac.ROOM_GUESS.astype(f32)
    p = ac.params(**ac.ROOM_PARAMS)
    store_before, map_before, frame_before = ff.store_download(0, ff.store_size())[0].tobytes(), ff.map_download().tobytes(), ff.frame_planes(0)[1].tobytes()
    for model_cam in (None, rc.CAM_96):
        got = _frame_parity(api, ff, fr, 1, segs, model_cam, guess, p, ("room", model_cam is None))
        dt, dr = ac.pose_error(got["pose"], ac.ROOM_TRUTH)
        print("room corner on the GPU (%s): status %d after %d iterations, %d pixels, rms %.3g m; %.3g mm and %.3g degrees from the truth"
              % ("own camera" if model_cam is None else "CAM_96", got["status"], got["iterations"], got["n_pixels"], got["rms"], 1e3 * dt, dr))
        assert got["status"] == api.ALIGN_CONVERGED
        assert dt < 1e-3 and dr < 0.05
    # fewer iterations than it needs; the map part alone (a third of the surfels missing: it still converges to the same place)
    one = _frame_parity(api, ff, fr, 1, segs, None, guess, ac.same_params(p, max_iterations=1), "one iteration")
    assert one["status"] == api.ALIGN_MAX_ITERATIONS and one["iterations"] == 1
    part = _frame_parity(api, ff, fr, 1, [], None, guess, p, "map part only")
    assert part["status"] == api.ALIGN_CONVERGED
    # nothing but scratch was written
    assert ff.store_download(0, ff.store_size())[0].tobytes() == store_before and ff.map_download().tobytes() == map_before
    assert ff.frame_planes(0)[1].tobytes() == frame_before
    ff.close()


def test_frame_degenerate(api):
    fr = ac.FRAME_64
    p = ac.params(**ac.ROOM_PARAMS)
    wall = (((0.0, 0.0, 1.0), 2.0),)
    ff, segs = _room_engine(api, wall)
    _upload(ff, 0, ac.room_depth(fr, ac.rigid((0, 0, 0), (0, 0, 0.02)), wall))
    got = _frame_parity(api, ff, fr, 1, segs, None, ac.IDENTITY, p, "one plane")
    assert got["status"] == api.ALIGN_SINGULAR and got["iterations"] == 0 and got["n_pixels"] > 1500
    # no overlap: the guess looks away from the wall; and an empty sequence
    away = ac.rigid((0, np.pi, 0)).astype(f32)
    for what, select, sg, guess in (("looking away", 1, segs, away), ("no surfels", 0, [], ac.IDENTITY)):
        got = _frame_parity(api, ff, fr, select, sg, None, guess, p, what)
        assert got["status"] == api.ALIGN_TOO_FEW and got["n_pixels"] == 0 and got["rms"] == 0.0 and not got["sums"].any()
        assert got["T"].tobytes() == np.eye(4, dtype=f32).tobytes() and got["pose"].tobytes() == np.asarray(guess, f32).tobytes()
    ff.close()


# ------------------------------------------------------------------ 5. the node
def _pose_matrix(p7):
    """geometry_msgs/Pose (px py pz qx qy qz qw) -> 4x4 float32, as the node casts its double matrix"""
    x, y, z, w = (np.float64(v) for v in p7[3:])
    s = 2.0 / (x * x + y * y + z * z + w * w)
    m = np.eye(4)
    m[:3, :3] = [[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                 [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                 [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]]
    m[:3, 3] = p7[:3]
    return m.astype(f32)


def test_node_align_last(api):
    from densesurfelmapping_amd import surfel_map, synth
    cam, scene = synth.TINY, synth.Scene()
    node = surfel_map.SurfelMap(cam, drift_free_poses=2)
    # After eight frames the active set is a couple of mature surfels covering a few hundred pixels of the 160x96 frame (the
    # inactive runs cover several times that), so every pixel is sampled and the loop asks for 100: with the default stride and
    # min_pixels the active case would stop as TOO_FEW before its first step and compare nothing of the loop.
    p = ac.params(stride=1, min_pixels=100)
    for kind in ("active", "inactive", "all", "neighbor"):  # (neighbor: its runs start from the pose of the latest fuse)
        with pytest.raises(api.DsmError) as e:
            node.align_last(kind, params=_params(api, p))
        assert e.value.code == api.DSM_E_STATE, kind
    with pytest.raises(api.DsmError) as e:
        node.last_pose()
    assert e.value.code == api.DSM_E_STATE
    last = {}
    node.set_publish(("active",), lambda pub: last.update(pub))
    for ev in synth.node_messages(cam, scene, 8, lap=40, keyframe_every=2):
        node.feed(ev)
    node.set_publish((), None)
    assert node.frames_fused == 8
    with pytest.raises(api.DsmError) as e:
        node.align_last("raw", params=_params(api, p))
    assert e.value.code == api.DSM_E_INVALID
    poses = [node.pose(i) for i in range(node.pose_count)]
    runs = [(q["points_begin_index"], q["n_attached"]) for q in poses if not q["is_local"] and q["n_attached"] > 0]
    before = (node.local_surfels().tobytes(), node.inactive_cloud().tobytes(), [node.attached_surfels(i).tobytes() for i in range(node.pose_count)])
    # the engine of the node, borrowed: the same handle, the slot of the latest fuse, the node's camera
    eng = api.FusionFunctions()
    eng._h = C.c_void_p(node._lib.dsm_surfel_map_engine(node._h))
    try:
        slot = (node.frames_fused - 1) & 1
        # the guess the node takes by default: the float matrix of the latest fuse, which the publication reports as a quaternion
        # pose (the same to an ulp of float at 6 m)
        fuse_pose = node.last_pose()
        assert np.abs(fuse_pose - _pose_matrix(last["fuse_pose"])).max() <= 1e-6
        for kind, select, segs in (("active", 1, []), ("all", 1, runs)):
            got = node.align_last(kind, params=_params(api, p))
            assert got["status"] != api.ALIGN_TOO_FEW and got["n_pixels"] >= p.min_pixels, (kind, got["status"], got["n_pixels"])
            print("node, %s: status %d after %d iterations, %d pixels, rms %.3g m" % (kind, got["status"], got["iterations"], got["n_pixels"], got["rms"]))
            want = eng.align_frame(slot, select, segs, fuse_pose, model_cam=api.render_camera(cam), params=_params(api, p))
            _same_result(got, want, kind)
            again = node.align_last(kind, pose_guess=fuse_pose, params=_params(api, p))
            _same_result(again, got, (kind, "explicit guess"))
    finally:
        eng._h = None
    after = (node.local_surfels().tobytes(), node.inactive_cloud().tobytes(), [node.attached_surfels(i).tobytes() for i in range(node.pose_count)])
    assert before == after
    node.close()


# ------------------------------------------------------------------ 6. argument checks
def test_invalid_arguments_touch_nothing(api):
    rng = np.random.default_rng(23)
    fr, cam = ac.FRAME_64, rc.CAM_70
    ff, segs = _room_engine(api)
    store_n = ff.store_size()
    depth, zm, nm = ac.random_planes(rng, fr, cam)
    model = Model(cam, zm, nm)
    _upload(ff, 0, depth)
    lib, good = ff._lib, ac.params(stride=1, dist_max=0.1)
    qmax = float(ac.np_qmax(cam))
    nan_T, inf_T = ac.IDENTITY.copy(), ac.IDENTITY.copy()
    nan_T[1, 3], inf_T[0, 0] = np.nan, np.inf

    def cam_with(**kw):
        c = api._RenderCamera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, cam.near_dist, cam.far_dist)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    bad_params = [dict(stride=0), dict(stride=-2), dict(dist_max=0.0), dict(dist_max=-1.0), dict(dist_max=float(np.nextafter(f32(qmax), f32(np.inf)))),
                  dict(dist_max=float("nan")), dict(min_view_cos=-0.1), dict(min_view_cos=1.5), dict(huber=-1.0), dict(huber=float("inf")),
                  dict(huber=float("nan")), dict(max_iterations=0),
                  dict(struct_size=32), dict(struct_size=40)]
    bad_cams = [cam_with(width=0), cam_with(height=8193), cam_with(fx=0.0), cam_with(fy=float("nan")), cam_with(near_dist=0.0), cam_with(near_dist=31.0),
                cam_with(far_dist=1e9)]  # (the last one: a fixed-point scale below 2^10)
    cases = [dict(params=ac.same_params(good, **b)) for b in bad_params] + [dict(cam=c) for c in bad_cams]
    cases += [dict(T=nan_T), dict(T=inf_T), dict(slot=-1), dict(slot=2)]
    frame_only = [dict(segs=[(0, store_n + 1)]), dict(segs=[(-1, 2)]), dict(segs=[(store_n, 1)]), dict(segs=[(3, -1)]), dict(select=3)]
    sums = np.full(ac.N_SUMS, 77, np.int64)
    k = C.c_int32(-7)
    res = api._AlignResult()
    C.memset(C.byref(res), 0x4d, C.sizeof(res))
    untouched = bytes(res)
    for case in cases + frame_only:
        kw = dict(params=good, cam=cam_with(), T=ac.IDENTITY, slot=0, segs=segs, select=1)
        kw.update(case)
        prm, t = _params(api, kw["params"]), ac.colmajor(kw["T"])
        seg = np.asarray(kw["segs"], np.int32).reshape(-1, 2)
        b, c = np.ascontiguousarray(seg[:, 0]), np.ascontiguousarray(seg[:, 1])
        if case not in frame_only:
            rcode = lib.dsm_align_equations(ff._h, kw["slot"], C.byref(kw["cam"]), C.c_void_p(model.d_zm.data_ptr()), C.c_void_p(model.d_nm.data_ptr()),
                                            t.ctypes.data, C.byref(prm), sums.ctypes.data, C.addressof(k))
            assert rcode == api.DSM_E_INVALID, ("equations", case)
        rcode = lib.dsm_align_frame(ff._h, kw["slot"], kw["select"], len(seg), b.ctypes.data, c.ctypes.data, C.byref(kw["cam"]), t.ctypes.data, C.byref(prm),
                                    C.byref(res))
        assert rcode == api.DSM_E_INVALID, ("frame", case)
        assert (sums == 77).all() and k.value == -7 and bytes(res) == untouched, case
    # null arguments
    t, prm = ac.colmajor(ac.IDENTITY), _params(api, good)
    assert lib.dsm_align_equations(ff._h, 0, C.byref(cam_with()), None, C.c_void_p(model.d_nm.data_ptr()), t.ctypes.data, C.byref(prm), sums.ctypes.data,
                                   C.addressof(k)) == api.DSM_E_INVALID
    assert lib.dsm_align_frame(ff._h, 0, 1, 0, None, None, None, None, C.byref(prm), C.byref(res)) == api.DSM_E_INVALID
    assert (sums == 77).all() and bytes(res) == untouched
    # ... and the handle still aligns
    _both(api, ff, fr, 0, model, ac.OBLIQUE_T, good, "after the refusals")
    ff.close()
