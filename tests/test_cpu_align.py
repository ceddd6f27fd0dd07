"""The frame-to-map alignment's definition without a GPU: csrc/dsm_align.h through the checker tests/align_host.cpp (what
tests/test_gpu_align.py compares the kernel and dsm_align_frame with, word for word).
  1. the checker's 29 sums == an independent numpy restatement, exactly; a census of the per-pixel rule's exits
  2. the order of the pixels does not matter
  3. the bound behind the fixed-point scale: int64 == __int128 at the bound; a camera that leaves k < 10 is refused
  4. the loop: a room corner converges to the truth; degenerate inputs end TOO_FEW / SINGULAR / MAX_ITERATIONS
  5. align_host.cpp's own main under the sanitizers
  6. the declarations"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import align_cases as ac
import render_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
PITCH = 80  # pad columns of the CPU tests' frames, filled with a depth that would pass


@pytest.fixture(scope="module")
def dtype():
    from densesurfelmapping_amd import api
    return api.SURFEL_DTYPE


@pytest.fixture(scope="module")
def crafted():
    return ac.crafted_case()


def _same(fd, depth, cam, zm, nm, T, p, what):
    got = ac.host_equations(fd, depth, cam, zm, nm, T, p, census=True)
    assert got is not None, what
    sums, k, census, exits = got
    want, want_exits, weight = ac.np_equations(fd, depth, cam, zm, nm, T, p)
    assert k == ac.np_scale(rc.as_camera(cam), ac.n_sampled(fd, p.stride)), what
    assert np.array_equal(exits, want_exits), (what, np.flatnonzero(exits != want_exits)[:5])
    assert [int(v) for v in sums] == want, (what, [i for i in range(ac.N_SUMS) if int(sums[i]) != want[i]])
    assert census.sum() == ac.n_sampled(fd, p.stride) and census[ac.PASS] == sums[28]
    return sums, census, exits, weight


# ------------------------------------------------------------------ 1. the restatement, and the census
def test_crafted_equals_restatement_and_takes_every_exit(crafted):
    depth, zm, nm, cases = crafted
    fd = ac.frame_desc(ac.FRAME_64, PITCH)
    dp = ac.pitched(depth, PITCH, 1.5)
    taken = np.zeros(ac.N_EXITS, np.int64)
    for T, names in cases + [(ac.IDENTITY, {}), (ac.OBLIQUE_T, {})]:
        for stride in (1, 2, 3):
            for huber in (ac.CRAFTED_PARAMS["huber"], 0.0):
                p = ac.params(**dict(ac.CRAFTED_PARAMS, stride=stride, huber=huber))
                sums, census, exits, weight = _same(fd, dp, rc.CAM_70, zm, nm, T, p, ("crafted", stride, huber))
                for (u, v), (name, allowed) in names.items():  # every crafted pixel leaves where it was built to leave
                    assert exits[ac.sampled_index(fd, stride, u, v)] in allowed, (name, stride, exits[ac.sampled_index(fd, stride, u, v)])
                if stride == 1 and huber > 0:
                    taken += census
                    if T is ac.CRAFTED_T:
                        by_name = {name: weight[ac.sampled_index(fd, 1, u, v)] for (u, v), (name, _) in names.items()}
                        assert by_name["|r| just inside huber"] == 1.0 and 0.999 < by_name["|r| just outside huber"] < 1.0
                        assert census[ac.PASS] >= 10
    print("census over the three crafted transforms:", taken.tolist())
    assert (taken > 0).all(), taken.tolist()


@pytest.mark.parametrize("fr,cam", [(ac.FRAME_64, rc.CAM_70), (ac.FRAME_100, rc.CAM_96)], ids=["64x32", "100x52"])
def test_random_planes_equal_restatement(fr, cam):
    rng = np.random.default_rng(11)
    fd = ac.frame_desc(fr, 128)
    depth, zm, nm = ac.random_planes(rng, fr, cam)
    dp = ac.pitched(depth, 128, 2.0)
    for T in (ac.IDENTITY, ac.OBLIQUE_T):
        for stride in (1, 2, 3):
            for huber in (0.01, 0.0):
                p = ac.params(stride=stride, huber=huber, dist_max=0.1)
                sums, census, _, _ = _same(fd, dp, cam, zm, nm, T, p, ("random", stride, huber))
                assert census[ac.PASS] > 0.3 * census.sum() and (census[[ac.X_DEPTH, ac.X_MODEL_DEPTH, ac.X_NORMAL, ac.X_DISTANCE]] > 0).all()


def test_strides_up_to_int_max():
    """a stride beyond the image side samples one column, one row or the pixel (0, 0) alone: the size of the sampled grid is
    computed without overflow for every stride an int holds"""
    rng = np.random.default_rng(13)
    fr, cam = ac.FRAME_100, rc.CAM_96
    fd = ac.frame_desc(fr, 128)
    depth, zm, nm = ac.random_planes(rng, fr, cam, garbage=False)
    dp = ac.pitched(depth, 128, 2.0)
    for stride, n in ((51, 4), (52, 2), (99, 2), (100, 1), (2**31 - 1, 1)):
        assert ac.n_sampled(fd, stride) == n
        p = ac.params(stride=stride, huber=0.0, dist_max=0.1)
        _, census, _, _ = _same(fd, dp, cam, zm, nm, ac.IDENTITY, p, ("stride", stride))
        assert census.sum() == n


# ------------------------------------------------------------------ 2. the order of the pixels
def test_pixel_order_does_not_matter(crafted):
    rng = np.random.default_rng(12)
    fd = ac.frame_desc(ac.FRAME_100, 128)
    depth, zm, nm = ac.random_planes(rng, ac.FRAME_100, rc.CAM_96)
    dp = ac.pitched(depth, 128)
    for stride in (1, 3):
        p = ac.params(stride=stride, huber=0.01, dist_max=0.1)
        n = ac.n_sampled(fd, stride)
        row_major, _ = ac.host_equations(fd, dp, rc.CAM_96, zm, nm, ac.OBLIQUE_T, p)
        assert row_major[28] > 100
        for order in (np.arange(n), np.arange(n)[::-1], rng.permutation(n)):
            sums, _ = ac.host_equations(fd, dp, rc.CAM_96, zm, nm, ac.OBLIQUE_T, p, order=order)
            assert np.array_equal(sums, row_major)
        half, _ = ac.host_equations(fd, dp, rc.CAM_96, zm, nm, ac.OBLIQUE_T, p, order=np.arange(n // 2))
        assert not np.array_equal(half, row_major)  # (the order argument is used)


# ------------------------------------------------------------------ 3. the bound
def _extreme(far):
    """a camera near the refusal, and 16 frame pixels that all land on its far corner pixel at 0.99 far with normals of length^2
    1.99 perpendicular to the ray: the rotational terms are as large as the rule lets them be"""
    cam = rc.Camera(16, 16, 8.0, 8.0, 7.5, 7.5, 1.0, far)
    fr = dict(width=4, height=4, fx=1e4, fy=1e4, cx=1.5, cy=1.5, near_dist=0.3, far_dist=4.0 * far)
    a = (15 - 7.5) / 8.0
    c = np.array([a, a, 1.0])
    length = np.linalg.norm(c)
    axis = np.cross([0.0, 0.0, 1.0], c / length)
    axis *= np.arccos(1.0 / length) / np.linalg.norm(axis)
    T = ac.rigid(axis).astype(f32)
    depth = np.full((4, 4), 0.99 * far * length, f32)
    zm = np.ones((16, 16), f32)
    nm = np.tile((np.sqrt(1.99 / 2) * np.array([1.0, -1.0, 0.0])).astype(f32), (16, 16, 1))
    return fr, cam, T, depth, zm, nm


def test_bound_holds_at_the_bound():
    lib = ac.host_lib()
    fr, cam, T, depth, zm, nm = _extreme(6.5e6)
    fd = ac.frame_desc(fr)
    qmax = lib.align_host_qmax(C.byref(cam))
    assert qmax == ac.np_qmax(cam)
    p = ac.params(stride=1, dist_max=qmax, min_view_cos=0.0, huber=0.0)
    k = lib.align_host_scale(C.byref(cam), 16)
    assert 10 <= k <= 12 and k == ac.np_scale(cam, 16)
    sums = np.zeros(ac.N_SUMS, np.int64)
    fill = C.c_double(0)
    t = ac.colmajor(T)
    same = lib.align_host_equations_wide(C.byref(fd), depth.ctypes.data, C.byref(cam), zm.ctypes.data, nm.ctypes.data, t.ctypes.data, C.byref(p),
                                         sums.ctypes.data, C.addressof(fill))
    print("k = %d, 16 of 16 pixels, the largest sum fills %.3f of int64" % (k, fill.value))
    assert same == 1 and sums[28] == 16
    # M = 2 qmax^2 per term; this scene reaches 2 * 1.99 * a^2 (0.99 far)^2 in the (omega_z, omega_z) entry: at least a tenth of int64
    assert 0.1 < fill.value < 0.5
    want, _, _ = ac.np_equations(fd, depth, cam, zm, nm, T, p)
    assert [int(v) for v in sums] == want
    # ordinary cameras get the cap or close to it
    assert lib.align_host_scale(C.byref(rc.CAM_70), 2048) == ac.np_scale(rc.CAM_70, 2048) >= 39 and ac.np_scale(rc.CAM_70, 228) == 40
    assert lib.align_host_scale(C.byref(rc.CAM_96), 1226 * 370) == ac.np_scale(rc.CAM_96, 1226 * 370) >= 30


def test_camera_that_leaves_less_than_ten_bits_is_refused():
    fr, cam, T, depth, zm, nm = _extreme(6.5e6 * 64)
    fd = ac.frame_desc(fr)
    assert ac.np_scale(cam, 16) < 10
    p = ac.params(stride=1, dist_max=1.0, min_view_cos=0.0, huber=0.0)
    assert ac.host_equations(fd, depth, cam, zm, nm, T, p) is None
    assert ac.host_frame(fd, depth, cam, zm, nm, ac.IDENTITY, p) is None
    # ... and so is every bad parameter
    fr, cam, T, depth, zm, nm = _extreme(6.5e6)
    good = ac.params(stride=1, dist_max=1.0)
    assert ac.host_equations(ac.frame_desc(fr), depth, cam, zm, nm, T, good) is not None
    qmax = float(ac.np_qmax(cam))
    for bad in (dict(stride=0), dict(dist_max=0.0), dict(dist_max=-1.0), dict(dist_max=float(np.nextafter(f32(qmax), f32(np.inf)))), dict(dist_max=float("nan")),
                dict(min_view_cos=-0.1), dict(min_view_cos=1.5), dict(huber=-1.0), dict(huber=float("inf")), dict(max_iterations=0), dict(struct_size=32)):
        assert ac.host_equations(ac.frame_desc(fr), depth, cam, zm, nm, T, ac.same_params(good, **bad)) is None, bad


# ------------------------------------------------------------------ 4. the loop
@pytest.fixture(scope="module")
def room(dtype):
    """the room seen by FRAME_64's own camera at the guess pose (the model), and the analytic frame at the true pose"""
    fr = ac.FRAME_64
    cam = rc.Camera(fr["width"], fr["height"], fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["near_dist"], fr["far_dist"])
    model = rc.host_render(ac.room_surfels(dtype), cam, ac.ROOM_GUESS.astype(f32))
    return fr, cam, model, ac.room_depth(fr, ac.ROOM_TRUTH)


def test_room_corner_converges_to_the_truth(room):
    fr, cam, model, depth = room
    assert (model["depth"] > 0).mean() > 0.95
    fd = ac.frame_desc(fr, PITCH)
    start = ac.pose_error(ac.ROOM_GUESS, ac.ROOM_TRUTH)
    assert abs(start[0] - 0.03) < 1e-6 and abs(start[1] - 1.5) < 1e-4
    r = ac.host_frame(fd, ac.pitched(depth, PITCH, 1.0), cam, model["depth"], model["normal"], ac.ROOM_GUESS.astype(f32), ac.params(**ac.ROOM_PARAMS))
    pose = np.array(r.pose16, f32).reshape(4, 4).T
    dt, dr = ac.pose_error(pose, ac.ROOM_TRUTH)
    print("room corner: status %d after %d iterations, %d pixels, rms %.3g m; %.3g mm and %.3g degrees from the truth" %
          (r.status, r.iterations, r.n_pixels, r.rms, 1e3 * dt, dr))
    assert r.status == ac.CONVERGED and r.iterations < ac.ROOM_PARAMS["max_iterations"]
    assert dt < 1e-3 and dr < 0.05
    assert r.n_pixels > 1500 and r.scale_log2 == ac.np_scale(cam, 2048)
    # pose = guess . T
    T = np.array(r.T16, f32).reshape(4, 4).T
    assert np.abs(ac.ROOM_GUESS.astype(f32).astype(np.float64) @ T.astype(np.float64) - pose).max() < 1e-6
    # one iteration only: the same first step, reported as MAX_ITERATIONS
    one = ac.host_frame(fd, ac.pitched(depth, PITCH, 1.0), cam, model["depth"], model["normal"], ac.ROOM_GUESS.astype(f32),
                        ac.params(**dict(ac.ROOM_PARAMS, max_iterations=1)))
    assert one.status == ac.MAX_ITERATIONS and one.iterations == 1
    assert ac.pose_error(np.array(one.pose16, f32).reshape(4, 4).T, ac.ROOM_TRUTH)[0] < start[0]


def test_degenerate_inputs(room, dtype):
    fr, cam, model, depth = room
    fd = ac.frame_desc(fr)
    p = ac.params(**ac.ROOM_PARAMS)
    # one plane only: three of the six directions are free
    wall = (((0.0, 0.0, 1.0), 2.0),)
    one = rc.host_render(ac.room_surfels(dtype, wall), cam, ac.IDENTITY)
    assert (one["depth"] > 0).mean() > 0.95
    r = ac.host_frame(fd, ac.room_depth(fr, ac.rigid((0, 0, 0), (0, 0, 0.02)), wall), cam, one["depth"], one["normal"], ac.IDENTITY, p)
    assert r.status == ac.SINGULAR and r.iterations == 0 and r.n_pixels > 1500
    # no overlap: the model shows nothing
    r = ac.host_frame(fd, depth, cam, np.zeros_like(model["depth"]), np.zeros_like(model["normal"]), ac.ROOM_GUESS.astype(f32), p)
    assert r.status == ac.TOO_FEW and r.iterations == 0 and r.n_pixels == 0 and r.rms == 0.0 and not any(r.sums)
    assert bytes(r.T16) == ac.colmajor(ac.IDENTITY).tobytes() and bytes(r.pose16) == ac.colmajor(ac.ROOM_GUESS).tobytes()
    # ... or the frame sees nothing
    r = ac.host_frame(fd, np.zeros_like(depth), cam, model["depth"], model["normal"], ac.ROOM_GUESS.astype(f32), p)
    assert r.status == ac.TOO_FEW and r.n_pixels == 0


# ------------------------------------------------------------------ 5. the stand-alone program under the sanitizers
def test_align_host_main_under_sanitizers(crafted, tmp_path):
    exe = str(tmp_path / "align_host_main")
    r = ac.build_main(exe)
    assert r.returncode == 0, r.stderr
    depth, zm, nm, _ = crafted
    paths = [str(tmp_path / "crafted.bin"), str(tmp_path / "random.bin")]
    ac.write_case(paths[0], ac.frame_desc(ac.FRAME_64, PITCH), ac.pitched(depth, PITCH, 1.5), rc.CAM_70, zm, nm)
    rd, rz, rn = ac.random_planes(np.random.default_rng(13), ac.FRAME_100, rc.CAM_96)
    ac.write_case(paths[1], ac.frame_desc(ac.FRAME_100, 128), ac.pitched(rd, 128, 2.0), rc.CAM_96, rz, rn)
    r = subprocess.run([exe] + paths, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout, r.stderr[-3000:])
    assert "every order agrees" in r.stdout


# ------------------------------------------------------------------ 6. the declarations
def test_align_abi_declarations():
    from densesurfelmapping_amd import api, build, surfel_map
    build.build_library()
    lib = C.CDLL(api.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "dsm.h")).read()
    node_hdr = open(os.path.join(ROOT, "include", "dsm_surfel_map.h")).read()
    for name in ("dsm_align_params_init", "dsm_align_equations", "dsm_align_frame"):
        assert name in api.ABI_SYMBOLS and name + "(" in hdr and hasattr(lib, name), name
    for name in ("dsm_surfel_map_align_last", "dsm_surfel_map_last_pose16"):
        assert name in surfel_map.ABI_SYMBOLS and name + "(" in node_hdr and hasattr(lib, name), name
    assert re.search(r"#define DSM_ABI_VERSION 4\b", hdr)
    lib.dsm_abi_version.restype = C.c_int
    assert lib.dsm_abi_version() == 4
    assert re.search(r"#define DSM_ALIGN_SUMS 29\b", hdr) and api.ALIGN_SUMS == 29 == ac.N_SUMS
    for k, name in enumerate(("CONVERGED", "MAX_ITERATIONS", "TOO_FEW", "SINGULAR")):
        assert re.search(r"DSM_ALIGN_%s = %d\b" % (name, k), hdr) and getattr(api, "ALIGN_" + name) == k == getattr(ac, name)
    assert C.sizeof(api._AlignParams) == 36 == C.sizeof(ac.Params) and C.sizeof(api._AlignResult) == 384 == C.sizeof(ac.Result)
    assert [f[0] for f in api._AlignParams._fields_] == [f[0] for f in ac.Params._fields_]
    assert [f[0] for f in api._AlignResult._fields_] == [f[0] for f in ac.Result._fields_]
    # the defaults are the documented ones, and the checker's params() restates them
    p = api._AlignParams()
    lib.dsm_align_params_init.argtypes = [C.c_void_p]
    lib.dsm_align_params_init.restype = None
    lib.dsm_align_params_init(C.byref(p))
    assert bytes(p) == bytes(ac.params()) and p.struct_size == 36
    # without a handle every call is refused before anything else
    lib.dsm_align_equations.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 7
    assert lib.dsm_align_equations(None, 0, None, None, None, None, None, None, None) == api.DSM_E_INVALID
    lib.dsm_align_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int32] + [C.c_void_p] * 6
    assert lib.dsm_align_frame(None, 0, 1, 0, None, None, None, None, None, None) == api.DSM_E_INVALID
    lib.dsm_surfel_map_align_last.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 3
    assert lib.dsm_surfel_map_align_last(None, 0, None, None, None) == api.DSM_E_INVALID
    assert "dsm_align_frame(" in open(os.path.join(ROOT, "include", "dsm_fusion_functions.hpp")).read()
    lib.dsm_surfel_map_last_pose16.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.dsm_surfel_map_last_pose16(None, None) == api.DSM_E_INVALID
    node_hpp = open(os.path.join(ROOT, "include", "dsm_surfel_map.hpp")).read()
    assert "dsm_surfel_map_align_last(" in node_hpp and "dsm_surfel_map_last_pose16(" in node_hpp
    for cls, names in ((api.FusionFunctions, ("align_equations", "align_frame")), (surfel_map.SurfelMap, ("align_last", "last_pose"))):
        assert all(hasattr(cls, n) for n in names)
