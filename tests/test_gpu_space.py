"""Free space and the three-state map on the GPU (dsm_grid_carve, dsm_grid_classify, dsm_surfel_map_set_free_space / _free_space* /
_space* / _carve_last, msglog --save-space): every bit equal to the brute-force host checker of tests/space_host.cpp, which
evaluates csrc/dsm_carve.h's carve_voxel over every voxel and frame and classifies neighbour by neighbour, and which
tests/test_cpu_space.py pins to a numpy restatement."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_cases as gc
import space_cases as sc

ROOT = sc.ROOT
pytestmark = pytest.mark.gpu

GUARD = 0x4d   # the byte a poisoned destination holds
N_GUARD = 256  # guard bytes behind every device buffer


@pytest.fixture(scope="module")
def api():
    import torch
    torch.cuda.init()  # (before the library's first HIP call, as in the other GPU suites)
    from densesurfelmapping_amd import api as api_mod
    return api_mod


def _engine(api, cam, slots=4):
    ff = api.FusionFunctions()
    ff.initialize(cam.w, cam.h, cam.fx, cam.fy, cam.cx, cam.cy, 30.0, 0.3, surfel_capacity=1 << 15, frame_slots=slots)
    assert ff.frame_pitch() == cam.pitch
    return ff


def _spec(api, s):
    return api.grid_spec(s.origin[:], s.voxel, (s.nx, s.ny, s.nz), 0)


def _params(api, s):
    return api.carve_params(near_dist=s.near_d, far_dist=s.far_d, margin=s.margin)


def _load(ff, slot, plane):
    """the whole pitched plane of a slot, pad columns included, through the debug tap; read back to be sure"""
    ff.frame_planes(slot, depth=plane)
    back = ff.frame_planes(slot)[1]
    assert back.tobytes() == np.ascontiguousarray(plane, np.float32).tobytes()
    if plane.shape[1] > ff.width:
        assert (back[:, ff.width:] == sc.PAD_DEPTH).all()  # a kernel that reads a pad column frees voxels the checker does not


def _words(n_words, init=None):
    """a device buffer of n_words words with guard bytes behind it: poisoned, or holding `init`"""
    import torch
    t = torch.full((n_words * 4 + N_GUARD,), GUARD, dtype=torch.uint8, device="cuda")
    if init is not None:
        t[:n_words * 4] = torch.from_numpy(np.ascontiguousarray(init, np.uint32).view(np.uint8).ravel()).cuda()
    return t


def _bytes(n, init=None):
    import torch
    t = torch.full((n + N_GUARD,), GUARD, dtype=torch.uint8, device="cuda")
    if init is not None:
        t[:n] = torch.from_numpy(np.ascontiguousarray(init).view(np.uint8).ravel()).cuda()
    return t


def _read(t, shape, dtype=np.uint32, what=""):
    a = t.cpu().numpy()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    assert (a[n:] == GUARD).all(), (what, "guard bytes written")
    return a[:n].view(dtype).reshape(shape).copy()


def _untouched(t, what=""):
    assert (t.cpu().numpy() == GUARD).all(), (what, "written")


def _row_major(inv16):
    return None if inv16 is None else np.asarray(inv16, np.float32).reshape(4, 4).T


def _carve(api, ff, s, frames, slots, old=None, flags=0, what=""):
    """dsm_grid_carve of `frames` (already in their slots) into a guarded device set holding `old` (None: empty): (bits, count)"""
    shape = sc.words(s)
    buf = _words(int(np.prod(shape)), np.zeros(shape, np.uint32) if old is None else old)
    invs = None if all(f[1] is None for f in frames) else [_row_major(f[1] if f[1] is not None else sc.closed_form_inverse(f[0])) for f in frames]
    n = ff.grid_carve(_spec(api, s), slots, [f[0] for f in frames], buf.data_ptr(), _params(api, s), flags, invs)
    bits = _read(buf, shape, what=what)
    assert n == int(gc.unpack(bits, s.nx).sum()), (what, "n_free is the population count")
    return bits, n


# ------------------------------------------------------------------ 1. carve parity
@pytest.mark.parametrize("g", sc.GRIDS, ids=[sc.grid_id(g) for g in sc.GRIDS])
def test_carve_parity(api, g):
    rng = np.random.default_rng(31)
    for cam_name, cam in sc.CAMS.items():
        ff = _engine(api, cam)
        for kind in sc.POSES:
            s, frames = sc.case(g, cam_name, kind)
            what = (g, cam_name, kind)
            _load(ff, 1, frames[0][2])
            exp, n_exp = sc.expected(g, cam_name, kind)
            bits, n = _carve(api, ff, s, frames, [1], what=what)
            assert np.array_equal(bits, exp) and n == n_exp, (what, int((bits != exp).sum()))
            # the old contents are OR-ed in, their dirty pad bits written 0; with DSM_CARVE_REPLACE they are ignored
            old = sc.dirty_pads(gc.pack(rng.random(g[::-1]) < 0.1), g[0], rng)
            bits, n = _carve(api, ff, s, frames, [1], old=old, what=what)
            assert np.array_equal(bits, sc.host_carve(s, frames, old)[0]), (what, "OR")
            bits, n = _carve(api, ff, s, frames, [1], old=old, flags=sc.REPLACE, what=what)
            assert np.array_equal(bits, exp) and n == n_exp, (what, "replace")
            t = sc.with_flags(s, sc.TRUST_INFINITE)
            bits, n = _carve(api, ff, t, frames, [1], flags=sc.TRUST_INFINITE, what=what)
            assert np.array_equal(bits, sc.host_carve(t, frames)[0]), (what, "trust infinite")
        ff.close()


def test_census_case_on_the_device(api):
    s, frames, _ = sc.census_case()
    ff = _engine(api, sc.CAM_64)
    for k, f in enumerate(frames):
        _load(ff, k, f[2])
    for flags in (0, sc.TRUST_INFINITE):
        t = sc.with_flags(s, flags)
        for pick in ([0], [1], [2], [0, 1, 2]):
            bits, n = _carve(api, ff, t, [frames[k] for k in pick], pick, flags=flags, what=(flags, pick))
            exp, n_exp = sc.host_carve(t, [frames[k] for k in pick])
            assert np.array_equal(bits, exp) and n == n_exp, (flags, pick, int((bits != exp).sum()))
    ff.close()


# ------------------------------------------------------------------ 2. many frames in one call
def test_frames_in_one_call_and_one_by_one(api):
    rng = np.random.default_rng(8)
    cam = sc.CAM_70
    ff = _engine(api, cam, slots=4)
    planes = [sc.depth_plane(cam, 70 + k) for k in range(4)]
    for k, p in enumerate(planes):
        _load(ff, k, p)
    for g in ((65, 4, 3), (37, 21, 13)):
        s = sc.make(g, cam)
        frames32 = [(pose, inv, planes[k % 4]) for k, (pose, inv, _) in enumerate(sc.many_frames(cam, 32))]
        old = gc.pack(rng.random(g[::-1]) < 0.03)
        for n_frames in (1, 2, 32):
            frames, slots = frames32[:n_frames], [k % 4 for k in range(n_frames)]
            exp, n_exp = sc.host_carve(s, frames, old)
            bits, n = _carve(api, ff, s, frames, slots, old=old, what=(g, n_frames))
            assert np.array_equal(bits, exp) and n == n_exp, (g, n_frames, "one call")
            assert not (old & ~bits).any()
            acc = old
            for f, slot in zip(frames, slots):
                acc, n_acc = _carve(api, ff, s, [f], [slot], old=acc, what=(g, n_frames, "one by one"))
            assert np.array_equal(acc, exp) and n_acc == n_exp, (g, n_frames, "one by one")
            fresh, n_fresh = _carve(api, ff, s, frames, slots, old=old, flags=sc.REPLACE, what=(g, n_frames, "replace"))
            assert np.array_equal(fresh, sc.host_carve(s, frames)[0]) and (n_frames < 32 or (fresh != bits).any())
    ff.close()


def test_origin_a_kilometre_out(api):
    """512 x 64 x 8 voxels whose origin lies at 1e3 m: grid_centre's roundings decide which pixel a centre falls on"""
    cam = sc.CAM_64
    g = (512, 64, 8)
    centre = (1000.0, 1000.0, 1001.6)
    s = sc.make(g, cam, origin=sc.origin_of(g, centre), far=30.0)
    frames = [(sc.pose_at((1000.0 - 20.0, 1000.0, 1001.2), yaw=np.pi / 2 - 0.05), None, sc.depth_plane(cam, 3) * np.float32(6.0)),
              (sc.pose_at((1000.0 + 5.0, 1000.3, 1001.0), yaw=-np.pi / 2 + 0.2, pitch=0.02), None, sc.depth_plane(cam, 4) * np.float32(4.0))]
    ff = _engine(api, cam)
    for k, f in enumerate(frames):
        _load(ff, k, f[2])
    exp, n_exp = sc.host_carve(s, frames)
    assert n_exp > 5000
    bits, n = _carve(api, ff, s, frames, [0, 1], what="origin at 1e3")
    assert np.array_equal(bits, exp) and n == n_exp, int((bits != exp).sum())
    ff.close()


# ------------------------------------------------------------------ 3. classify parity
def _classify(api, ff, g, occ_bits, fre_bits, planes=("state", "known_free", "frontier", "cells"), cap=None, what=""):
    """dsm_grid_classify into guarded buffers: ({plane: array}, n_frontier, the DsmError or None)"""
    nx, ny, nz = g
    n_vox, shape = nx * ny * nz, (nz, ny, (nx + 31) // 32)
    n_words = int(np.prod(shape))
    cap = n_vox if cap is None else cap
    occ, fre = _words(n_words, occ_bits), _words(n_words, fre_bits)
    bufs = {"state": _bytes(n_vox), "known_free": _words(n_words), "frontier": _words(n_words), "cells": _words(max(cap, 1))}
    err = None
    try:
        n = ff.grid_classify(g, occ.data_ptr(), fre.data_ptr(), {k: bufs[k].data_ptr() for k in planes}, cells_cap=cap)
    except api.DsmError as e:
        if e.code != api.DSM_E_CAPACITY:
            raise
        err, n = e, e.n_frontier
    for k in bufs:
        if k not in planes:
            _untouched(bufs[k], (what, k))
    out = {}
    if "state" in planes:
        out["state"] = _read(bufs["state"], (nz, ny, nx), np.uint8, what)
    for k in ("known_free", "frontier"):
        if k in planes:
            out[k] = _read(bufs[k], shape, what=what)
    if "cells" in planes:
        cells = bufs["cells"].cpu().numpy()
        assert (cells[4 * min(n, cap):] == GUARD).all(), (what, "written past the count or the cap")
        out["cells"] = cells[:4 * min(n, cap)].view(np.int32).copy()
    assert np.array_equal(_read(occ, shape), occ_bits) and np.array_equal(_read(fre, shape), fre_bits), (what, "the sources are read only")
    return out, n, err


def _same_space(got, exp, what):
    for k in ("state", "known_free", "frontier", "cells"):
        if k in got:
            assert got[k].dtype == exp[k].dtype and np.array_equal(got[k], exp[k]), (what, k)


@pytest.mark.parametrize("g", sc.CLASSIFY_GRIDS, ids=[sc.grid_id(g) for g in sc.CLASSIFY_GRIDS])
def test_classify_parity(api, g):
    rng = np.random.default_rng(12)
    ff = _engine(api, sc.CAM_64)
    for k, (name, (occ, fre)) in enumerate(sc.classify_sets(g).items()):
        ob, fb = sc.dirty_pads(gc.pack(occ), g[0], rng), sc.dirty_pads(gc.pack(fre), g[0], rng)
        exp = sc.host_classify(ob, fb, g[0])
        got, n, err = _classify(api, ff, g, ob, fb, what=(g, name))
        assert err is None and n == exp["n_frontier"], (g, name)
        _same_space(got, exp, (g, name))
        for one in ("state", "known_free", "frontier", "cells"):  # the planes one at a time: the count is always reported
            got, n, err = _classify(api, ff, g, ob, fb, planes=(one,), what=(g, name, one))
            assert err is None and n == exp["n_frontier"], (g, name, one)
            _same_space(got, exp, (g, name, one))
        if exp["n_frontier"] > 1:  # DSM_E_CAPACITY: the count needed, the other planes complete, nothing past the cap
            cap = exp["n_frontier"] // 2
            got, n, err = _classify(api, ff, g, ob, fb, cap=cap, what=(g, name, "cap"))
            assert err is not None and n == exp["n_frontier"], (g, name, "cap")
            _same_space(got, dict(exp, cells=exp["cells"][:cap]), (g, name, "cap"))
            got, n, err = _classify(api, ff, g, ob, fb, cap=exp["n_frontier"], what=(g, name, "exact cap"))
            assert err is None
            _same_space(got, exp, (g, name, "exact cap"))
    ff.close()


def test_frontier_by_hand_on_the_device(api):
    ff = _engine(api, sc.CAM_64)
    for name, g, occ, fre, frontier in sc.by_hand():
        ob, fb = gc.pack(sc.voxels(g, occ)), gc.pack(sc.voxels(g, fre))
        got, n, err = _classify(api, ff, g, ob, fb, what=name)
        want = sc.voxels(g, frontier)
        assert err is None and n == len(frontier) and np.array_equal(gc.unpack(got["frontier"], g[0]), want), name
        assert np.array_equal(got["cells"], np.flatnonzero(want.ravel())), name
        _same_space(got, sc.host_classify(ob, fb, g[0]), name)
    ff.close()


# ------------------------------------------------------------------ 4. refusals
def test_refusals_touch_nothing(api):
    cam = sc.CAM_64
    g = (33, 9, 5)
    s = sc.make(g, cam)
    ff = _engine(api, cam, slots=2)
    plane = sc.depth_plane(cam, 1)
    _load(ff, 0, plane)
    lib, h = ff._lib, ff._h
    n_words, n_vox = 2 * 9 * 5, 33 * 9 * 5
    dst = _words(n_words)
    pose = np.ascontiguousarray(np.eye(4, dtype=np.float32).ravel())

    def spec_with(**kw):
        sp = _spec(api, s)
        for k, v in kw.items():
            setattr(sp, k, v)
        return sp

    def params_with(**kw):
        p = _params(api, s)
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def bad_pose(k, v):
        p = pose.copy()
        p[k] = v
        return p

    nan, inf = float("nan"), float("inf")
    ok = dict(spec=_spec(api, s), params=_params(api, s), flags=0, n=1, slots=np.array([0], np.int32), pose=pose, inv=None, dst=dst.data_ptr())
    bad = [dict(spec=None), dict(params=None), dict(slots=None), dict(pose=None), dict(dst=None), dict(dst=dst.data_ptr() + 2), dict(dst=dst.data_ptr() + 1),
           dict(flags=4), dict(flags=0x80000000), dict(flags=7),
           dict(spec=spec_with(struct_size=32)), dict(spec=spec_with(voxel=0.0)), dict(spec=spec_with(voxel=nan)), dict(spec=spec_with(nx=0)), dict(spec=spec_with(nz=-1)),
           dict(spec=spec_with(nx=1 << 13, ny=1 << 13, nz=8)), dict(spec=spec_with(inflate=17)), dict(spec=spec_with(inflate=-1)),
           dict(params=params_with(struct_size=12)), dict(params=params_with(near_dist=0.0)), dict(params=params_with(near_dist=-1.0)), dict(params=params_with(near_dist=nan)),
           dict(params=params_with(far_dist=inf)), dict(params=params_with(far_dist=nan)), dict(params=params_with(far_dist=0.2)), dict(params=params_with(near_dist=4.0)),
           dict(params=params_with(margin=-0.01)), dict(params=params_with(margin=nan)), dict(params=params_with(margin=inf)),
           dict(pose=bad_pose(3, nan)), dict(pose=bad_pose(12, inf)), dict(inv=bad_pose(5, nan)), dict(inv=bad_pose(14, -inf)),
           dict(slots=np.array([2], np.int32)), dict(slots=np.array([-1], np.int32)), dict(n=0), dict(n=-1), dict(n=33)]
    origin_nan = _spec(api, s)
    origin_nan.origin[1] = nan
    bad.append(dict(spec=origin_nan))
    for case in bad:
        kw = dict(ok, **case)
        n = C.c_int64(-7)
        n_frames = kw["n"]
        slots = kw["slots"] if kw["slots"] is None or n_frames <= 1 else np.zeros(n_frames, np.int32)
        poses = kw["pose"] if kw["pose"] is None or n_frames <= 1 else np.tile(pose, n_frames)
        rc = lib.dsm_grid_carve(h, None if kw["spec"] is None else C.byref(kw["spec"]), None if kw["params"] is None else C.byref(kw["params"]), kw["flags"], n_frames,
                                None if slots is None else slots.ctypes.data, None if poses is None else poses.ctypes.data,
                                None if kw["inv"] is None else kw["inv"].ctypes.data, kw["dst"], C.byref(n))
        assert rc == api.DSM_E_INVALID and n.value == -7, (case, rc)
        _untouched(dst, case)
    # dsm_grid_classify
    occ, fre = _words(n_words, np.zeros((5, 9, 2), np.uint32)), _words(n_words, np.zeros((5, 9, 2), np.uint32))
    bufs = {"state": _bytes(n_vox), "known_free": _words(n_words), "frontier": _words(n_words), "cells": _words(64)}
    p = {k: t.data_ptr() for k, t in bufs.items()}

    def planes(**kw):
        q = dict(p, cells_cap=64)
        q.update(kw)
        return api._SpacePlanes(q["state"], q["known_free"], q["frontier"], q["cells"], q["cells_cap"])

    okc = dict(dims=g, occ=occ.data_ptr(), fre=fre.data_ptr(), planes=planes(), n=True)
    badc = [dict(occ=None), dict(fre=None), dict(planes=None), dict(n=False), dict(dims=(0, 9, 5)), dict(dims=(33, -1, 5)), dict(dims=(1 << 13, 1 << 13, 8)),
            dict(occ=occ.data_ptr() + 2), dict(fre=fre.data_ptr() + 1),
            dict(planes=planes(state=None, known_free=None, frontier=None, cells=None)), dict(planes=planes(cells_cap=-1)),
            dict(planes=planes(frontier=p["known_free"])), dict(planes=planes(cells=p["frontier"])),
            dict(planes=planes(known_free=p["known_free"] + 2)), dict(planes=planes(frontier=p["frontier"] + 1)), dict(planes=planes(cells=p["cells"] + 2)),
            dict(planes=planes(state=occ.data_ptr())), dict(planes=planes(known_free=fre.data_ptr())), dict(planes=planes(frontier=occ.data_ptr() + n_words * 4 - 4)),
            dict(planes=planes(state=fre.data_ptr() - n_vox + 1))]
    for case in badc:
        kw = dict(okc, **case)
        n = C.c_int32(-7)
        rc = lib.dsm_grid_classify(h, *kw["dims"], kw["occ"], kw["fre"], None if kw["planes"] is None else C.byref(kw["planes"]), C.byref(n) if kw["n"] else None)
        assert rc == api.DSM_E_INVALID and n.value == -7, (case, rc)
        for t in bufs.values():
            _untouched(t, case)
    with pytest.raises(api.DsmError) as e:  # the Python wrappers raise the same
        ff.grid_carve(_spec(api, s), [0], [np.eye(4)], dst.data_ptr(), params_with(margin=-1.0))
    assert e.value.code == api.DSM_E_INVALID
    with pytest.raises(api.DsmError) as e:
        ff.grid_classify(g, occ.data_ptr(), fre.data_ptr(), {})
    assert e.value.code == api.DSM_E_INVALID
    _untouched(dst)
    # ... and the handle still works
    frames = [(np.eye(4, dtype=np.float32), None, plane)]
    bits, n = _carve(api, ff, s, frames, [0])
    exp, n_exp = sc.host_carve(s, frames)
    assert np.array_equal(bits, exp) and n == n_exp > 0
    ff.close()


# ------------------------------------------------------------------ 5. the node and msglog
NODE_VOXEL, NODE_DIMS = 0.5, (32, 160, 16)  # around the origin, where the first camera sits; it drives along +y, z is up
NODE_CARVE = dict(near_dist=0.5, far_dist=25.0, margin=0.9)


def _slot_plane(node, slot):
    """the pitched depth plane of an engine slot of the node, through the engine's debug tap"""
    lib = node._lib
    lib.dsm_surfel_map_engine.restype = C.c_void_p
    eng = C.c_void_p(lib.dsm_surfel_map_engine(node._h))
    pitch = C.c_int32(0)
    lib.dsm_frame_pitch.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.dsm_frame_pitch(eng, C.byref(pitch)) == 0
    dep = np.zeros((node.cam.height, pitch.value), np.float32)
    lib.dsm_debug_frame_planes.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    assert lib.dsm_debug_frame_planes(eng, slot, 0, None, dep.ctypes.data) == 0
    return dep


def test_node_accumulates_free_space(api, tmp_path):
    from densesurfelmapping_amd import msglog, surfel_map, synth
    import node_state
    case = node_state.SCENARIOS[0]  # one lap and ONE loop closure
    (cam, scene), dfp = node_state.camera_and_scene(case, synth), case["drift_free_poses"]
    events = list(synth.node_messages(cam, scene, case["frames"], **case["kw"]))
    log = str(tmp_path / "node.dsmlog")
    msglog.write_log(log, cam, dfp, iter(events))
    spec = api.grid_spec_around((0.0, 0.0, 0.0), NODE_VOXEL, NODE_DIMS)  # (what msglog --save-space takes)
    nx, ny, nz = NODE_DIMS
    # the same replay with the accumulator off: the reference state
    plain = surfel_map.SurfelMap(cam, drift_free_poses=dfp)
    for ev in events:
        plain.feed(ev)
    want_state = node_state.digest(node_state.snapshot(plain))
    plain.save_cloud(str(tmp_path / "plain.pcd"))
    plain.close()

    node = surfel_map.SurfelMap(cam, drift_free_poses=dfp)
    for call in (node.free_space, node.space):  # DSM_E_STATE before set_free_space ...
        with pytest.raises(api.DsmError) as e:
            call()
        assert e.value.code == api.DSM_E_STATE
    with pytest.raises(api.DsmError) as e:  # ... a refused request changes nothing ...
        node.set_free_space(spec, dict(NODE_CARVE, margin=-1.0))
    assert e.value.code == api.DSM_E_INVALID
    node.set_free_space(spec, NODE_CARVE)
    for call in (node.free_space, node.space):  # ... and before the first fuse
        with pytest.raises(api.DsmError) as e:
            call()
        assert e.value.code == api.DSM_E_STATE
    import torch
    with pytest.raises(api.DsmError) as e:
        node.carve_last(spec, torch.zeros(16, dtype=torch.int32, device="cuda").data_ptr())
    assert e.value.code == api.DSM_E_STATE
    fused, reset_at = [], []
    for ev in events:
        before, resets = node.frames_fused, node.free_space_resets
        node.feed(ev)
        assert node.frames_fused - before <= 1
        if node.free_space_resets != resets:
            reset_at.append(before)  # frames [before, ...) were fused after the warp
        if node.frames_fused > before:
            fused.append((node.last_pose(), None, _slot_plane(node, before & 1)))
    assert node.frames_fused == len(fused) > 40
    # one loop closure: one reset, and the set holds only the frames fused since
    assert node.free_space_resets == 1 and len(reset_at) == 1 and 0 < reset_at[0] < len(fused), (node.free_space_resets, reset_at)
    c = sc.Cam(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)
    assert fused[0][2].shape == (c.h, c.pitch)
    s = sc.make(NODE_DIMS, c, origin=spec.origin[:], near=NODE_CARVE["near_dist"], far=NODE_CARVE["far_dist"], margin=NODE_CARVE["margin"], voxel=NODE_VOXEL)
    exp, n_exp = sc.host_carve(s, fused[reset_at[0]:])
    everything = sc.host_carve(s, fused)[0]
    free, n_free = node.free_space()
    print("node free space:", n_free, "voxels of", nx * ny * nz, "since the reset;", int(gc.unpack(everything, nx).sum()), "over all frames")
    assert n_exp > 100 and (everything != exp).any()
    assert np.array_equal(free, exp) and n_free == n_exp, int((free != exp).sum())
    dev = _words(exp.size)
    assert node.free_space(dev.data_ptr()) == n_exp and np.array_equal(_read(dev, exp.shape), exp)
    # the stateless counterpart: the latest frame alone into a caller's set
    own = _words(exp.size, np.zeros_like(exp))
    node.carve_last(spec, own.data_ptr(), NODE_CARVE)
    assert np.array_equal(_read(own, exp.shape), sc.host_carve(s, fused[-1:])[0])
    # the three states: dsm_surfel_map_grid's occupied set against the accumulated free set
    for kind in ("all", "active"):
        occ = node.grid(kind, spec=spec, planes=("occupied",))
        want = sc.host_classify(occ["occupied"], exp, nx)
        got = node.space(kind)
        assert got["n_surfels"] == occ["n_surfels"] and got["n_frontier"] == want["n_frontier"] > 0
        _same_space(got, want, kind)
        assert (got["state"] == sc.OCCUPIED).any() and (got["state"] == sc.FREE).any() and (got["state"] == sc.UNKNOWN).any()
        with pytest.raises(api.DsmError) as e:
            node.space(kind, cells_cap=want["n_frontier"] - 1)
        assert e.value.code == api.DSM_E_CAPACITY and e.value.n_frontier == want["n_frontier"]
        cut = e.value.planes  # the other planes are complete, the list holds what fits
        _same_space({k: cut[k] for k in ("state", "known_free", "frontier")}, want, (kind, "cap"))
        assert np.array_equal(cut["cells"][:want["n_frontier"] - 1], want["cells"][:-1]), (kind, "cap")
        bufs = {"state": _bytes(nx * ny * nz), "frontier": _words(exp.size), "cells": _words(want["n_frontier"])}
        assert node.space(kind, dst_ptrs={k: t.data_ptr() for k, t in bufs.items()}, cells_cap=want["n_frontier"]) == (occ["n_surfels"], want["n_frontier"])
        assert np.array_equal(_read(bufs["state"], (nz, ny, nx), np.uint8), want["state"]) and np.array_equal(_read(bufs["frontier"], exp.shape), want["frontier"])
        assert np.array_equal(_read(bufs["cells"], (want["n_frontier"],), np.int32), want["cells"])
    with pytest.raises(api.DsmError) as e:
        node.space("raw")
    assert e.value.code == api.DSM_E_INVALID
    space_all = node.space("all")
    # the map, the poses and the exports are those of the replay with the accumulator off
    assert node_state.digest(node_state.snapshot(node)) == want_state
    node.save_cloud(str(tmp_path / "carved.pcd"))
    assert open(str(tmp_path / "carved.pcd"), "rb").read() == open(str(tmp_path / "plain.pcd"), "rb").read()
    # a new spec clears the set; switching off releases it
    node.set_free_space(spec, NODE_CARVE)
    assert node.free_space()[1] == 0 and not node.free_space()[0].any() and node.free_space_resets == 1
    node.set_free_space(None)
    with pytest.raises(api.DsmError) as e:
        node.free_space()
    assert e.value.code == api.DSM_E_STATE
    node.close()
    # msglog --save-space writes the same arrays (a process of its own: that is what the command is)
    out = str(tmp_path / "space.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "densesurfelmapping_amd.msglog", log, "--save-space", out, "--grid-voxel", str(NODE_VOXEL), "--grid-dims"]
                         + [str(d) for d in NODE_DIMS] + ["--carve-near", "0.5", "--carve-far", "25", "--carve-margin", "0.9"], capture_output=True, text=True, env=env, cwd=ROOT)
    assert run.returncode == 0, run.stderr[-2000:]
    summary = json.loads(run.stdout.strip().splitlines()[-1])
    assert summary["frames_fused"] == len(fused) and summary["free_voxels"] == n_exp and summary["free_space_resets"] == 1
    assert summary["frontier_cells"] == space_all["n_frontier"]
    saved = np.load(out)
    assert saved["origin"].tolist() == list(spec.origin) and saved["dims"].tolist() == list(NODE_DIMS) and saved["voxel"] == np.float32(NODE_VOXEL)
    assert int(saved["resets"]) == 1 and int(saved["n_free"]) == n_exp and saved["margin"] == np.float32(0.9)
    assert np.array_equal(saved["state"], space_all["state"]) and np.array_equal(saved["frontier_cells"], space_all["cells"]) and np.array_equal(saved["free"], exp)
