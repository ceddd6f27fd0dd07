"""Viewpoint gain on the GPU (dsm_grid_view, dsm_surfel_map_view_gain*, msglog --save-view-gain): every score and every visible plane
equal, byte for byte, to the brute-force host checker of tests/view_host.cpp, which evaluates csrc/dsm_view.h over every pose, voxel
and interior point of its line by the closed form, and which tests/test_cpu_view.py pins to a numpy restatement.  Destinations are
poisoned device buffers with guard bytes behind them."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_cases as gc
import space_cases as sc
import view_cases as vc

ROOT = vc.ROOT
pytestmark = pytest.mark.gpu

GUARD = 0x4d   # the byte a poisoned destination holds
N_GUARD = 256  # guard bytes behind every device buffer


@pytest.fixture(scope="module")
def api():
    import torch
    torch.cuda.init()  # (before the library's first HIP call, as in the other GPU suites)
    from densesurfelmapping_amd import api as api_mod
    return api_mod


@pytest.fixture(scope="module")
def ff(api):
    """one engine for the calls that need nothing of it but its scratch and its stream"""
    cam = sc.CAM_64
    f = api.FusionFunctions()
    f.initialize(cam.w, cam.h, cam.fx, cam.fy, cam.cx, cam.cy, 30.0, 0.3, surfel_capacity=1 << 12, frame_slots=2)
    yield f
    f.close()


def _spec(api, s):
    return api.grid_spec(s.origin[:], s.voxel, (s.nx, s.ny, s.nz), 0)


def _words(n_words, init=None):
    """a device buffer of n_words words with guard bytes behind it: poisoned, or holding `init`"""
    import torch
    t = torch.full((n_words * 4 + N_GUARD,), GUARD, dtype=torch.uint8, device="cuda")
    if init is not None:
        t[:n_words * 4] = torch.from_numpy(np.array(init, np.uint32).view(np.uint8).ravel()).cuda()  # (a copy: the shared sets are read-only)
    return t


def _read(t, shape, dtype=np.uint32, what=""):
    a = t.cpu().numpy()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    assert (a[n:] == GUARD).all(), (what, "guard bytes written")
    return a[:n].view(dtype).reshape(shape).copy()


def _untouched(t, what=""):
    assert (t.cpu().numpy() == GUARD).all(), (what, "written")


def _row_major(inv16):
    return np.asarray(inv16, np.float32).reshape(4, 4).T


class _Sets:
    """the three sources of a call in guarded device buffers"""

    def __init__(self, occ, fre, tgt):
        self.host = (occ, fre, tgt)
        self.dev = [_words(b.size, b) for b in (occ, fre, tgt)]
        self.occ, self.fre, self.tgt = (t.data_ptr() for t in self.dev)

    def intact(self, what=""):
        for t, b in zip(self.dev, self.host):
            assert np.array_equal(_read(t, b.shape, what=what), b), (what, "a source was written")


def _view(api, ff, s, poses, sets, target=True, invs=None, scores="host", planes=True, what=""):
    """dsm_grid_view into poisoned, guarded destinations: (scores or None, visible planes or None)"""
    n, shape = len(poses), vc.words(s)
    vis = _words(n * int(np.prod(shape))) if planes else None
    dsc = _words(n * 8) if scores == "device" else None
    got = ff.grid_view(_spec(api, s), vc.cam_of(s), poses, sets.occ, sets.fre, sets.tgt if target else None, s.flags,
                       None if invs is None else [_row_major(i) for i in invs], vis.data_ptr() if planes else None, dsc.data_ptr() if dsc is not None else None,
                       scores=scores is not None)
    if scores == "device":
        assert got is None
        got = _read(dsc, (n * 8,), np.int32, what).view(vc.SCORE_DTYPE)
    elif scores is None:
        assert got is None
    sets.intact(what)
    return got, (_read(vis, (n,) + shape, what=what) if planes else None)


def _same(got, vis, exp, what):
    if got is not None:
        assert got.tobytes() == exp["scores"].tobytes(), (what, got, exp["scores"])
    if vis is not None:
        assert vis.tobytes() == exp["visible"].tobytes(), (what, int((vis != exp["visible"]).sum()))


# ------------------------------------------------------------------ 1. parity on the shared calls
SMALL = [name for name in vc.CALLS if not name.startswith(("33x5x3", "256x64x32"))]


@pytest.mark.parametrize("name", SMALL)
def test_view_parity(api, ff, name):
    """the wave unit of 64, the word seams, the partial word, a single voxel; 1, 3 and 65 poses; cameras inside, outside and at both
    ends of the reach; both flags, with and without a target; host and device scores; scores only and planes only"""
    s, poses, occ, fre, tgt = vc.call(name)
    sets = _Sets(occ, fre, tgt)
    for flags in (0, vc.UNKNOWN_BLOCKS):
        t = vc.with_flags(s, flags)
        for target in (True, False):
            exp = vc.expected(name, flags, target)
            _same(*_view(api, ff, t, poses, sets, target, what=(name, flags, target)), exp, (name, flags, target))
            assert target or not exp["scores"]["target"].any()
    exp = vc.expected(name)
    _same(*_view(api, ff, s, poses, sets, scores="device", what=(name, "device scores")), exp, (name, "device scores"))
    got, vis = _view(api, ff, s, poses, sets, scores="device", planes=False, what=(name, "scores only"))
    assert vis is None
    _same(got, None, exp, (name, "scores only"))
    got, vis = _view(api, ff, s, poses, sets, scores="host", planes=False, what=(name, "host scores only"))
    _same(got, None, exp, (name, "host scores only"))
    got, vis = _view(api, ff, s, poses, sets, scores=None, what=(name, "planes only"))
    assert got is None
    _same(None, vis, exp, (name, "planes only"))
    if name.endswith("/reach"):
        assert exp["scores"]["in_view"].sum() > 0
        for axis in range(3):  # one voxel past either end: refused, nothing written
            for side in ("low-1", "high+1"):
                dst = _words(8)
                with pytest.raises(api.DsmError) as e:
                    ff.grid_view(_spec(api, s), vc.cam_of(s), [vc.reach_pose(s, axis, side)], sets.occ, sets.fre, scores_ptr=dst.data_ptr())
                assert e.value.code == api.DSM_E_INVALID
                _untouched(dst, (name, axis, side))


def test_view_at_the_pose_limit(api, ff):
    """DSM_VIEW_MAX_POSES poses in one call: the pose dimension of the launch past its cap"""
    name = "33x5x3/4096"
    s, poses, occ, fre, tgt = vc.call(name)
    assert len(poses) == vc.MAX_POSES == api.VIEW_MAX_POSES
    sets = _Sets(occ, fre, tgt)
    exp = vc.expected(name)
    _same(*_view(api, ff, s, poses, sets, what=name), exp, name)
    assert (exp["scores"]["visible"] > 0).sum() > 1000
    dst = _words(8 * (vc.MAX_POSES + 1))
    with pytest.raises(api.DsmError) as e:
        ff.grid_view(_spec(api, s), vc.cam_of(s), poses + poses[:1], sets.occ, sets.fre, scores_ptr=dst.data_ptr())
    assert e.value.code == api.DSM_E_INVALID
    _untouched(dst)


def test_view_past_one_grid_stride_trip(api, ff):
    """256 x 64 x 32 voxels with 8 poses: more units than the launch has waves, so every wave makes several trips"""
    name = "256x64x32/8"
    s, poses, occ, fre, tgt = vc.call(name)
    assert (s.nx + 63) // 64 * s.ny * s.nz > 4 * 1024  # (kViewBlocksX workgroups of 4 waves)
    sets = _Sets(occ, fre, tgt)
    for flags in (0, vc.UNKNOWN_BLOCKS):
        _same(*_view(api, ff, vc.with_flags(s, flags), poses, sets, what=(name, flags)), vc.expected(name, flags), (name, flags))
    assert vc.expected(name)["scores"]["visible"].sum() > 1000


def test_census_calls_on_the_device(api, ff):
    """every exit and line shape of the census, and the caller's inverse taken bit for bit"""
    s, poses, occ, fre, tgt, _ = vc.census_call()
    sets = _Sets(occ, fre, tgt)
    for flags in (0, vc.UNKNOWN_BLOCKS):
        t = vc.with_flags(s, flags)
        _same(*_view(api, ff, t, poses, sets, what=("census", flags)), vc.host_view(t, poses, occ, fre, tgt), ("census", flags))
    s, pose, base, inv = vc.inverse_call()
    occ, fre, tgt = vc.sets_of(s, 81)
    sets = _Sets(occ, fre, tgt)
    closed, own = vc.host_view(s, [pose], occ, fre, tgt), vc.host_view(s, [pose], occ, fre, tgt, invs=[inv])
    assert closed["scores"]["in_view"][0] != own["scores"]["in_view"][0]
    _same(*_view(api, ff, s, [pose], sets, what="closed form"), closed, "closed form")
    _same(*_view(api, ff, s, [pose], sets, invs=[base], what="the closed form handed in"), closed, "the closed form handed in")
    _same(*_view(api, ff, s, [pose], sets, invs=[inv], what="own inverse"), own, "own inverse")


# ------------------------------------------------------------------ 2. refusals
def test_refusals_touch_nothing(api, ff):
    name = "130x3x2/3"
    s, poses, occ, fre, tgt = vc.call(name)
    sets = _Sets(occ, fre, tgt)
    lib, h = ff._lib, ff._h
    n, n_words = len(poses), int(np.prod(vc.words(s)))
    vis, dsc = _words(n * n_words), _words(n * 8)
    host_scores = np.full(n * 8, -7, np.int32)
    p16 = api.view_poses(poses)
    nan, inf = float("nan"), float("inf")

    def spec_with(**kw):
        sp = _spec(api, s)
        for k, v in kw.items():
            setattr(sp, k, v)
        return sp

    def cam_with(**kw):
        c = api.render_camera(vc.cam_of(s))
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    def bad_pose(k, v):
        p = p16.copy()
        p[1, k] = v
        return p

    origin_nan = _spec(api, s)
    origin_nan.origin[1] = nan
    far_away = p16.copy()
    far_away[2, 13] = s.origin[1] + (s.ny + vc.MAX_REACH + 0.5) * s.voxel
    ok = dict(spec=_spec(api, s), cam=cam_with(), flags=0, n=n, poses=p16, inv=None, occ=sets.occ, fre=sets.fre, tgt=sets.tgt, scores=dsc.data_ptr(), on_device=1,
              vis=vis.data_ptr())
    bad = [dict(spec=None), dict(cam=None), dict(poses=None), dict(occ=None), dict(fre=None), dict(scores=None, vis=None),
           dict(flags=2), dict(flags=0x80000000), dict(flags=3),
           dict(occ=sets.occ + 2), dict(fre=sets.fre + 1), dict(tgt=sets.tgt + 2), dict(vis=vis.data_ptr() + 2), dict(scores=dsc.data_ptr() + 1),
           dict(spec=spec_with(struct_size=32)), dict(spec=spec_with(voxel=0.0)), dict(spec=spec_with(voxel=nan)), dict(spec=spec_with(nx=0)), dict(spec=spec_with(nz=-1)),
           dict(spec=spec_with(nx=1 << 13, ny=1 << 13, nz=8)), dict(spec=spec_with(inflate=17)), dict(spec=spec_with(inflate=-1)), dict(spec=origin_nan),
           dict(cam=cam_with(width=0)), dict(cam=cam_with(height=8193)), dict(cam=cam_with(fx=0.0)), dict(cam=cam_with(fy=-1.0)), dict(cam=cam_with(fx=nan)),
           dict(cam=cam_with(cx=inf)), dict(cam=cam_with(cy=nan)), dict(cam=cam_with(near_dist=0.0)), dict(cam=cam_with(near_dist=nan)), dict(cam=cam_with(far_dist=inf)),
           dict(cam=cam_with(far_dist=0.1)), dict(cam=cam_with(near_dist=5.0)),
           dict(poses=bad_pose(3, nan)), dict(poses=bad_pose(12, inf)), dict(inv=bad_pose(5, nan)), dict(inv=bad_pose(14, -inf)), dict(poses=far_away),
           dict(n=0), dict(n=-1), dict(n=vc.MAX_POSES + 1),
           # an output overlapping a source, or the other output
           dict(vis=sets.occ), dict(vis=sets.fre + 4), dict(vis=sets.tgt - 4), dict(scores=sets.occ), dict(scores=sets.fre + n_words * 4 - 4),
           dict(scores=vis.data_ptr() + 8), dict(vis=dsc.data_ptr())]
    lib.dsm_grid_view.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_int32] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p]
    for case in bad:
        kw = dict(ok, **case)
        pp = kw["poses"]
        if kw["n"] > n and pp is not None:
            pp = np.ascontiguousarray(np.tile(p16[:1], (kw["n"], 1)))
        rc = lib.dsm_grid_view(h, None if kw["spec"] is None else C.byref(kw["spec"]), None if kw["cam"] is None else C.byref(kw["cam"]), kw["flags"], kw["n"],
                               None if pp is None else pp.ctypes.data, None if kw["inv"] is None else kw["inv"].ctypes.data, kw["occ"], kw["fre"], kw["tgt"],
                               kw["scores"], kw["on_device"], kw["vis"])
        assert rc == api.DSM_E_INVALID, (case, rc)
        _untouched(vis, case)
        _untouched(dsc, case)
        sets.intact(case)
    # host scores are not written either, and a host destination may lie anywhere
    rc = lib.dsm_grid_view(h, C.byref(ok["spec"]), C.byref(ok["cam"]), 2, n, p16.ctypes.data, None, sets.occ, sets.fre, sets.tgt, host_scores.ctypes.data, 0, None)
    assert rc == api.DSM_E_INVALID and (host_scores == -7).all()
    with pytest.raises(api.DsmError) as e:  # the Python wrapper raises the same
        ff.grid_view(_spec(api, s), vc.cam_of(s), poses, sets.occ, sets.fre, flags=4)
    assert e.value.code == api.DSM_E_INVALID
    # ... and the handle still works
    _same(*_view(api, ff, s, poses, sets, what="after the refusals"), vc.expected(name), "after the refusals")


# ------------------------------------------------------------------ 3. shared scratch
def test_interleaved_with_the_other_grid_calls(api, ff):
    """small, larger, small: dsm_grid_view between dsm_grid_classify, dsm_grid_components and dsm_grid_inflate on one handle, each of
    which regrows scratch the others use"""
    import torch
    for name in ("130x3x2/3", "70x33x19/65", "1x1x1/3", "256x64x32/8", "130x3x2/65"):
        s, poses, occ, fre, tgt = vc.call(name)
        sets = _Sets(occ, fre, tgt)
        g, shape = vc.dims(s), vc.words(s)
        n_words, n_vox = int(np.prod(shape)), s.nx * s.ny * s.nz
        exp = vc.expected(name)
        _same(*_view(api, ff, s, poses, sets, what=(name, "first")), exp, (name, "first"))
        want = sc.host_classify(occ, fre, s.nx)
        fr = _words(n_words)
        assert ff.grid_classify(g, sets.occ, sets.fre, {"frontier": fr.data_ptr()}) == want["n_frontier"]
        frontier = _read(fr, shape)
        assert np.array_equal(frontier, want["frontier"])
        _same(*_view(api, ff, s, poses, sets, what=(name, "after classify")), exp, (name, "after classify"))
        label = torch.empty((n_vox,), dtype=torch.int32, device="cuda")
        n_comp, n_all = ff.grid_components(g, fr.data_ptr(), 26, 1, label_ptr=label.data_ptr())
        assert n_comp == n_all and (n_comp > 0) == bool(want["n_frontier"])
        inflated = _words(n_words)
        ff.grid_inflate(g, 1, sets.occ, inflated.data_ptr())
        assert np.array_equal(_read(inflated, shape), gc.pack(gc.np_inflate(gc.unpack(occ, s.nx), 1)))
        # the frontier as the target, as the node passes it
        got, vis = _view(api, ff, s, poses, _Sets(occ, fre, frontier), what=(name, "frontier target"))
        _same(got, vis, vc.host_view(s, poses, occ, fre, frontier), (name, "frontier target"))


# ------------------------------------------------------------------ 4. the node and msglog
NODE_VOXEL, NODE_DIMS = 0.5, (32, 160, 16)  # around the origin, where the first camera sits; it drives along +y, z is up
NODE_CARVE = dict(near_dist=0.5, far_dist=25.0, margin=0.9)
NODE_VIEW_CAM = vc.Cam(48, 16, 23.0, 21.5, 23.6, 7.7, 0.5, 25.0)  # a coarse sensor model: not the node's own camera


def _node_poses(msglog, node):
    """candidates around the latest pose: turned about its y axis, and one moved 40 m away to where it sees nothing"""
    poses = list(msglog.yaw_poses(node.last_pose(), 5))
    away = poses[0].copy()
    away[:3, 3] += 60.0 * away[:3, 2]
    return poses + [away]


def _node_check(api, ff, vc_grid, node, msglog, what):
    """view_gain of the node, host and device destinations, against the checker and against dsm_grid_view driven by hand from the
    node's own planes"""
    spec = node._space_spec
    nx = spec.nx
    poses = _node_poses(msglog, node)
    occ = node.grid("all", spec=spec, planes=("occupied",))["occupied"]
    fre, _ = node.free_space()
    frontier = node.space("all")["frontier"]
    shape = occ.shape
    for flags in (0, vc.UNKNOWN_BLOCKS):
        for target in ("frontier", "none"):
            s = vc.with_flags(vc_grid, flags)
            exp = vc.host_view(s, poses, occ, fre, frontier if target == "frontier" else None)
            scores, vis = node.view_gain(poses, "all", camera=NODE_VIEW_CAM, target=target, flags=flags, visible=True)
            _same(scores, vis, exp, (what, flags, target, "host"))
            assert node.view_gain(poses, "all", camera=NODE_VIEW_CAM, target=target, flags=flags).tobytes() == exp["scores"].tobytes()
            dsc, dvis = _words(len(poses) * 8), _words(len(poses) * occ.size)
            assert node.view_gain(poses, "all", camera=NODE_VIEW_CAM, target=target, flags=flags, dst_ptrs={"scores": dsc.data_ptr(), "visible": dvis.data_ptr()}) is None
            _same(_read(dsc, (len(poses) * 8,), np.int32).view(vc.SCORE_DTYPE), _read(dvis, (len(poses),) + shape), exp, (what, flags, target, "device"))
            dsc = _words(len(poses) * 8)
            node.view_gain(poses, "all", camera=NODE_VIEW_CAM, target=target, flags=flags, dst_ptrs={"scores": dsc.data_ptr()})
            _same(_read(dsc, (len(poses) * 8,), np.int32).view(vc.SCORE_DTYPE), None, exp, (what, flags, target, "device scores only"))
            # by hand on another handle, from the node's planes
            by_hand = _view(api, ff, s, poses, _Sets(occ, fre, frontier), target == "frontier", what=(what, "by hand"))
            _same(*by_hand, exp, (what, flags, target, "by hand"))
    return vc.host_view(vc_grid, poses, occ, fre, frontier), occ, fre


def test_node_view_gain(api, ff, tmp_path):
    from densesurfelmapping_amd import msglog, surfel_map, synth
    import node_state
    case = node_state.SCENARIOS[0]  # one lap and ONE loop closure
    (cam, scene), dfp = node_state.camera_and_scene(case, synth), case["drift_free_poses"]
    events = list(synth.node_messages(cam, scene, case["frames"], **case["kw"]))
    log = str(tmp_path / "node.dsmlog")
    msglog.write_log(log, cam, dfp, iter(events))
    spec = api.grid_spec_around((0.0, 0.0, 0.0), NODE_VOXEL, NODE_DIMS)  # (what msglog --save-view-gain takes)
    vc_grid = vc.make(NODE_DIMS, NODE_VIEW_CAM, origin=spec.origin[:], voxel=NODE_VOXEL)
    node = surfel_map.SurfelMap(cam, drift_free_poses=dfp)
    one = [np.eye(4, dtype=np.float32)]
    with pytest.raises(api.DsmError) as e:  # DSM_E_STATE before set_free_space ...
        node.view_gain(one, camera=NODE_VIEW_CAM)
    assert e.value.code == api.DSM_E_STATE
    q = node.view_query()  # the node's own camera; the library's carve range while free space is off
    assert (q.camera.width, q.camera.height, q.camera.fx, q.camera.cy) == (cam.width, cam.height, np.float32(cam.fx), np.float32(cam.cy))
    assert q.camera.near_dist == np.float32(0.1) and q.camera.far_dist == 10.0 and q.target == api.VIEW_TARGET_FRONTIER and q.flags == 0
    node.set_free_space(spec, NODE_CARVE)
    q = node.view_query()
    assert q.camera.near_dist == 0.5 and q.camera.far_dist == 25.0  # the accumulator's carve range
    with pytest.raises(api.DsmError) as e:  # ... and before the first fuse
        node.view_gain(one, camera=NODE_VIEW_CAM)
    assert e.value.code == api.DSM_E_STATE
    checked_reset = False
    for ev in events:
        resets = node.free_space_resets
        node.feed(ev)
        if node.free_space_resets != resets and not checked_reset:  # right behind the loop-closure reset: nothing is known free
            checked_reset = True
            exp, occ, fre = _node_check(api, ff, vc_grid, node, msglog, "after the reset")
            if not fre.any():
                assert not exp["scores"]["free"].any() and (exp["scores"]["unknown"] + exp["scores"]["occupied"] == exp["scores"]["visible"]).all()
    assert checked_reset and node.free_space_resets == 1
    exp, occ, fre = _node_check(api, ff, vc_grid, node, msglog, "at the end")
    print("node view gain at the end:", exp["scores"])
    assert exp["scores"]["visible"].sum() > 0 and exp["scores"]["free"].sum() > 0
    # refusals of the node's own
    for kw in (dict(target=7), dict(flags=2), dict(kind="raw")):
        with pytest.raises(api.DsmError) as e:
            node.view_gain(one, camera=NODE_VIEW_CAM, **kw)
        assert e.value.code == api.DSM_E_INVALID, kw
    with pytest.raises(api.DsmError) as e:
        node.view_gain(one, camera=NODE_VIEW_CAM, dst_ptrs={})
    assert e.value.code == api.DSM_E_INVALID
    # the node's own camera by default: what msglog scores with
    own_cam = vc.Cam(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy, 0.5, 25.0)
    yaws = msglog.yaw_poses(node.last_pose(), 3)
    frontier = node.space("all")["frontier"]
    want = vc.host_view(vc.make(NODE_DIMS, own_cam, origin=spec.origin[:], voxel=NODE_VOXEL), list(yaws), occ, fre, frontier)
    assert node.view_gain(yaws).tobytes() == want["scores"].tobytes()
    frames_fused = node.frames_fused
    node.close()
    # msglog --save-view-gain writes the same (a process of its own: that is what the command is)
    out = str(tmp_path / "view.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "densesurfelmapping_amd.msglog", log, "--save-view-gain", out, "--view-yaws", "3", "--grid-voxel", str(NODE_VOXEL), "--grid-dims"]
                         + [str(d) for d in NODE_DIMS] + ["--carve-near", "0.5", "--carve-far", "25", "--carve-margin", "0.9"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    summary = json.loads(run.stdout.strip().splitlines()[-1])
    assert summary["frames_fused"] == frames_fused and summary["view_poses"] == 3 and summary["view_unknown_seen"] == want["scores"]["unknown"].tolist()
    saved = np.load(out)
    assert saved["origin"].tolist() == list(spec.origin) and saved["dims"].tolist() == list(NODE_DIMS) and saved["voxel"] == np.float32(NODE_VOXEL)
    assert np.array_equal(saved["poses"], yaws) and saved["scores"].tobytes() == want["scores"].tobytes()
    assert saved["camera"].tolist() == [cam.width, cam.height, np.float32(cam.fx), np.float32(cam.fy), np.float32(cam.cx), np.float32(cam.cy), 0.5, 25.0]
