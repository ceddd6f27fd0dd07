"""The map renderer on the GPU (dsm_render_compose, dsm_surfel_map_render*): all four planes bit-identical, for host and device
destinations, to the brute-force host renderer of tests/render_host.cpp, which evaluates the same csrc/dsm_math.h functions
as the kernels and which tests/test_cpu_render.py pins to a float64 restatement of the definition."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mesh_cases as mc
import render_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GUARD = 77  # bytes 0x4d: as float 2.15e8, as int 1296911693 -- no plane value of these scenes
N_GUARD = 64


@pytest.fixture(scope="module")
def api():
    import torch
    torch.cuda.init()  # (before the library's first HIP call, as in the other GPU suites)
    from densesurfelmapping_amd import api as api_mod
    return api_mod


def _engine(api, cap=1 << 15, flags=0):
    ff = api.FusionFunctions()
    ff.initialize(64, 32, 57.25, 55.5, 31.3, 15.7, 30.0, 0.3, surfel_capacity=cap, frame_slots=2, flags=flags)
    return ff


def _device_buffers(api, cam, planes=None):
    """a torch byte buffer per plane with N_GUARD guard elements behind it, all bytes GUARD"""
    import torch
    bufs = {}
    for k in (planes or api.RENDER_PLANES):
        dt, tail = api.RENDER_PLANE_TYPES[k]
        n = cam.height * cam.width * int(np.prod(tail, dtype=np.int64)) + N_GUARD
        bufs[k] = torch.full((n * np.dtype(dt).itemsize,), GUARD, dtype=torch.uint8, device="cuda")
    return bufs


def _read_device(api, cam, bufs, what=""):
    out = {}
    for k, t in bufs.items():
        dt, tail = api.RENDER_PLANE_TYPES[k]
        a = t.cpu().numpy().view(dt)
        n = cam.height * cam.width * int(np.prod(tail, dtype=np.int64))
        assert (a[n:].view(np.uint8) == GUARD).all(), (what, k, "guard elements written")
        out[k] = a[:n].reshape((cam.height, cam.width) + tail)
    return out


def _render_both(api, ff, select, segs, cam, pose, flags=0, pose_inv=None, what=""):
    """host destination and device destination (with guards): the same planes; returns them"""
    host = ff.render(select, segs, cam, pose, pose_inv=pose_inv, flags=flags)
    bufs = _device_buffers(api, cam)
    n = ff.render(select, segs, cam, pose, pose_inv=pose_inv, flags=flags, dst_ptrs={k: t.data_ptr() for k, t in bufs.items()})
    assert n == host["n_surfels"], what
    rc.same_planes(_read_device(api, cam, bufs, what), host, (what, "device vs host destination"))
    return host


def _check(api, ff, seq, select, segs, cam, pose, flags=0, eigen33=False, what=""):
    got = _render_both(api, ff, select, segs, cam, pose, flags, what=what)
    assert got["n_surfels"] == len(seq), (what, got["n_surfels"], len(seq))
    exp = rc.host_render(seq, cam, pose, flags=flags, eigen33=eigen33, brute=True)
    rc.same_planes(got, exp, what)
    return got


# ------------------------------------------------------------------ 1. the crafted set
@pytest.mark.parametrize("cam", [rc.CAM_70, rc.CAM_96], ids=["70x37", "96x64"])
def test_crafted_set(api, cam):
    ff = _engine(api)
    m, names = rc.crafted_records(api.SURFEL_DTYPE, cam)
    ff.map_upload(m)
    box, keep = rc.host_boxes(m, cam, rc.IDENTITY)
    big = keep & (((box[:, 2] - box[:, 0]) > 16) | ((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1]) > 256))
    for name in ("covers the whole image", "the camera centre inside a disc's reach: the plane x = 2.5", "inf size"):
        assert big[names.index(name)], name  # these force the workgroup-per-splat tier
    assert (keep & ~big).sum() >= 10
    shown = set()
    for pose in (rc.IDENTITY, rc.oblique_pose()):
        for select in (1, 2):
            for flags in (0, rc.CULL_BACKFACES):
                seq = rc.keep_select(m, select)
                got = _check(api, ff, seq, select, (), cam, pose, flags, what=("crafted", cam.width, select, flags))
                shown |= set(seq["color"][np.unique(got["index"][got["index"] >= 0])].tolist())
    # update_times 0 / 4 / 5 (colours 190 / 200 / 210) against select 1 and 2
    assert 210.0 in shown and 200.0 in shown and 190.0 not in shown
    got1 = ff.render(1, (), cam, rc.IDENTITY)
    seq1 = rc.keep_select(m, 1)
    assert 200.0 not in set(seq1["color"][np.unique(got1["index"][got1["index"] >= 0])].tolist())
    ff.close()


# ------------------------------------------------------------------ 2. store runs, then the map part
def test_store_runs_then_map(api):
    rng = np.random.default_rng(5)
    cam, pose = rc.CAM_96, rc.oblique_pose()
    ff = _engine(api)
    world = rc.render_records(rng, 5000, api.SURFEL_DTYPE)  # placed for a camera at the origin: move them in front of `pose`
    P = pose.astype(np.float64)
    pw = np.stack([world["px"], world["py"], world["pz"]], 1).astype(np.float64) @ P[:3, :3].T + P[:3, 3]
    nw = np.stack([world["nx"], world["ny"], world["nz"]], 1).astype(np.float64) @ P[:3, :3].T
    for k, f in enumerate(("px", "py", "pz")):
        world[f] = pw[:, k]
    for k, f in enumerate(("nx", "ny", "nz")):
        world[f] = nw[:, k]
    # (no arbitrary bit patterns here: the link to the mesh below is a statement about surfels with unit normals)
    world["last_update"] = rng.integers(0, 9, len(world))
    ff.map_upload(world)
    for key in (3, 0, 7, 5):
        ff.store_deactivate(key)
    store_n = ff.store_size()
    store, _ = ff.store_download(0, store_n)
    live = ff.map_download()
    assert store_n > 1000 and len(live) > 1000
    cases = [[], [(0, store_n)], [(5, 0), (0, 0)],
             [(store_n - 1, 1), (0, 3), (100, 50), (7, 0), (100, 50)],        # out of store order, length 1, repeated, empty
             [(3, 63), (900, 2), (50, 700)], [(store_n - 300, 300), (0, 300)]]
    for segs in cases:
        runs = np.concatenate([store[b:b + c] for b, c in segs]) if segs else store[:0]
        for sel in ((0, 1, 2) if len(segs) in (0, 5) else (1,)):
            seq = np.concatenate([runs, rc.keep_select(live, sel)])  # the runs FIRST, then the map part
            got = _check(api, ff, seq, sel, segs, cam, pose, what=("runs", segs, sel))
            if sel == 0 and not segs:
                assert (got["index"] == -1).all() and (got["depth"] == 0).all() and (got["normal"] == 0).all() and (got["intensity"] == 0).all()
                continue
            # the sanity link to the mesh: index i names hexagon i of mesh_compose's output
            ref6 = ff.mesh_compose(sel, segs, mc.REF6).reshape(-1, 6, 6)
            assert len(ref6) == len(seq)
            idx = np.unique(got["index"][got["index"] >= 0])
            assert len(idx) > 20 or not len(seq)
            centre = ref6[idx, :, :3].astype(np.float64).mean(1)
            pos = np.stack([seq["px"], seq["py"], seq["pz"]], 1).astype(np.float64)[idx]
            assert (np.linalg.norm(centre - pos, axis=1) <= 1e-3 * np.abs(seq["size"][idx].astype(np.float64))).all(), (segs, sel)
    ff.close()


# ------------------------------------------------------------------ 3. the small / big threshold
def test_tier_threshold(api):
    """boxes just below, at and above 16 pixels of width and 256 pixels of area: which tier splats a surfel changes nothing"""
    rng = np.random.default_rng(3)
    cam = rc.CAM_96
    n, z = 4000, 2.0
    a = np.zeros(n, api.SURFEL_DTYPE)
    u, v = rng.uniform(20, 76, n), rng.uniform(15, 49, n)
    a["px"], a["py"], a["pz"] = (u - cam.cx) / cam.fx * z, (v - cam.cy) / cam.fy * z, z
    t = rng.uniform(-0.5, 0.5, (n, 2))
    nn = np.stack([t[:, 0], t[:, 1], -np.ones(n)], 1)
    nn /= np.linalg.norm(nn, axis=1, keepdims=True)
    a["nx"], a["ny"], a["nz"] = nn.T
    a["size"] = rng.uniform(0.12, 0.19, n)
    a["color"] = rng.uniform(0, 255, n)
    a["update_times"] = 7
    box, keep = rc.host_boxes(a, cam, rc.IDENTITY)
    bw, area = box[:, 2] - box[:, 0], (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    assert keep.all()
    for name, cls in (("width 15", bw == 15), ("width 16", bw == 16), ("width 17", bw == 17), ("area 256", (bw <= 16) & (area == 256)),
                      ("area just below", (bw <= 16) & (area >= 250) & (area < 256)), ("area just above", (bw <= 16) & (area > 256) & (area <= 275))):
        assert cls.sum() >= 10, name
    ff = _engine(api)
    # each tier on its own, then everything at once (4000 overlapping discs: most pixels are contested across the tiers)
    small = (bw <= 16) & (area <= 256)
    for what, part in (("small tier only", a[small][:300]), ("big tier only", a[~small][:300]), ("both", a)):
        ff.map_upload(part)
        _check(api, ff, part, 2, (), cam, rc.IDENTITY, what=what)
    ff.close()


# ------------------------------------------------------------------ 4. a map grown by the pipeline; 5. determinism
@pytest.mark.parametrize("eigen33", [False, True], ids=["eigen32", "eigen33"])
def test_pipeline_map(api, eigen33):
    from densesurfelmapping_amd import synth
    cam, scene = synth.TINY, synth.Scene()
    ff = api.FusionFunctions.from_camera(cam, surfel_capacity=65536, flags=api.DSM_FLAG_EIGEN33_PRODUCTS if eigen33 else 0)
    local = np.zeros(0, api.SURFEL_DTYPE)
    for t, img, dep, pose, ref in synth.sequence(cam, scene, 8):
        local, _ = ff.fuse_map(ref, img, dep, pose, local)
    assert len(local) > 200
    rcam = api.render_camera(cam)
    side = np.array(pose, np.float32).copy()
    side[:3, 3] += side[:3, 0] * np.float32(0.2)  # 0.2 m along the camera's x axis
    for what, p in (("last pose", np.asarray(pose, np.float32)), ("0.2 m to the side", side)):
        for select in (1, 2):
            seq = rc.keep_select(local, select)
            got = _check(api, ff, seq, select, (), rcam, p, eigen33=eigen33, what=(what, select, eigen33))
            if select == 2:
                assert (got["index"] >= 0).mean() > 0.3, what  # the map does predict the view
            again = ff.render(select, (), rcam, p)  # 5. the same render twice: identical bytes
            for k in api.RENDER_PLANES:
                assert got[k].tobytes() == again[k].tobytes(), (what, k)
    # the caller's own inverse is used as given
    inv = np.linalg.inv(np.asarray(pose, np.float64)).astype(np.float32)
    got = _render_both(api, ff, 2, (), rcam, pose, pose_inv=inv, what="own inverse")
    rc.same_planes(got, rc.host_render(rc.keep_select(local, 2), rcam, pose, inv=inv, eigen33=eigen33), "own inverse")
    ff.close()


# ------------------------------------------------------------------ 6. guard bands and NULL planes
def test_null_planes_and_guards(api):
    rng = np.random.default_rng(8)
    cam = rc.CAM_70
    ff = _engine(api)
    m = rc.mixed_records(rng, 3000, api.SURFEL_DTYPE)
    ff.map_upload(m)
    full = _check(api, ff, rc.keep_select(m, 2), 2, (), cam, rc.IDENTITY, what="all planes")
    assert (full["index"] >= 0).mean() > 0.5
    for planes in (("depth",), ("index",), ("normal",), ("intensity",), ("depth", "intensity"), ("index", "normal")):
        host = ff.render(2, (), cam, rc.IDENTITY, planes=planes)
        assert set(host) == set(planes) | {"n_surfels"}
        rc.same_planes(host, {k: full[k] for k in planes}, planes)
        # device: the planes asked for are written, the buffers of the others stay as they were although they are not passed ...
        bufs = _device_buffers(api, cam)
        ff.render(2, (), cam, rc.IDENTITY, dst_ptrs={k: bufs[k].data_ptr() for k in planes})
        got = _read_device(api, cam, {k: bufs[k] for k in planes}, planes)
        rc.same_planes(got, {k: full[k] for k in planes}, ("device", planes))
        for k in set(api.RENDER_PLANES) - set(planes):
            assert (bufs[k].cpu().numpy() == GUARD).all(), (planes, k)
    ff.close()


# ------------------------------------------------------------------ 7. error returns
def test_invalid_arguments_touch_nothing(api):
    rng = np.random.default_rng(9)
    cam = rc.CAM_70
    ff = _engine(api)
    m = rc.mixed_records(rng, 2000, api.SURFEL_DTYPE)
    m["last_update"] = rng.integers(0, 3, len(m))
    ff.map_upload(m)
    ff.store_deactivate(1)
    store_n = ff.store_size()
    assert store_n > 100
    bufs = _device_buffers(api, cam)
    ptrs = {k: t.data_ptr() for k, t in bufs.items()}
    nan_pose, inf_pose = rc.IDENTITY.copy(), rc.IDENTITY.copy()
    nan_pose[1, 3], inf_pose[0, 0] = np.nan, np.inf

    def cam_with(**kw):
        c = api.render_camera(cam)
        c = api._RenderCamera(c.width, c.height, c.fx, c.fy, c.cx, c.cy, c.near_dist, c.far_dist)
        for k, v in kw.items():
            setattr(c, k, v)
        return c

    bad = [dict(segs=[(0, store_n + 1)]), dict(segs=[(-1, 2)]), dict(segs=[(store_n, 1)]), dict(segs=[(3, -1)]), dict(segs=[(0, 5), (store_n - 1, 2)]),
           dict(camera=cam_with(width=0)), dict(camera=cam_with(width=8193)), dict(camera=cam_with(height=0)), dict(camera=cam_with(height=8193)),
           dict(camera=cam_with(width=-5)), dict(camera=cam_with(fx=0.0)), dict(camera=cam_with(fy=-1.0)), dict(camera=cam_with(fx=float("nan"))),
           dict(camera=cam_with(near_dist=0.0)), dict(camera=cam_with(near_dist=-1.0)), dict(camera=cam_with(near_dist=30.0)),
           dict(camera=cam_with(near_dist=31.0)), dict(pose=nan_pose), dict(pose=inf_pose), dict(pose_inv=nan_pose), dict(none=True), dict(select=3)]
    for case in bad:
        kw = dict(select=1, segs=(), camera=cam, pose=rc.IDENTITY, pose_inv=None)
        none = case.pop("none", False)
        kw.update(case)
        for dst in ("device", "host"):
            with pytest.raises(api.DsmError) as e:
                if none:
                    ff.render(kw["select"], kw["segs"], kw["camera"], kw["pose"], planes=(), dst_ptrs={} if dst == "device" else None)
                else:
                    ff.render(kw["select"], kw["segs"], kw["camera"], kw["pose"], pose_inv=kw["pose_inv"], dst_ptrs=ptrs if dst == "device" else None)
            assert e.value.code == api.DSM_E_INVALID, case
        for k, t in bufs.items():
            assert (t.cpu().numpy() == GUARD).all(), (case, k)
    # host destinations stay untouched as well
    host = {k: np.full(cam.height * cam.width * (3 if k == "normal" else 1), GUARD, api.RENDER_PLANE_TYPES[k][0]) for k in api.RENDER_PLANES}
    st = api._RenderPlanes(*(host[k].ctypes.data for k in api.RENDER_PLANES))
    c = cam_with(near_dist=40.0)
    n = C.c_int32(-7)
    p = api.pose_to_colmajor(rc.IDENTITY)
    assert ff._lib.dsm_render_compose(ff._h, 1, 0, None, None, C.byref(c), p.ctypes.data, None, 0, C.byref(st), 0, C.byref(n)) == api.DSM_E_INVALID
    assert all((host[k] == GUARD).all() for k in host) and n.value == -7
    # ... and the handle still renders
    _check(api, ff, rc.keep_select(ff.map_download(), 1), 1, (), cam, rc.IDENTITY, what="after the refusals")
    ff.close()


# ------------------------------------------------------------------ 8. the node
def _driftfree(links, root, rng_):
    """SurfelMap::get_driftfree_poses"""
    if root >= len(links):
        return []
    out, level = [root], [root]
    for _ in range(1, rng_):
        nxt = []
        for p in level:
            for q in links[p]:
                if q not in out:
                    nxt.append(q)
                    out.append(q)
        level = nxt
    return out


def _pose_matrix(p7):
    """geometry_msgs/Pose (px py pz qx qy qz qw) -> 4x4 float32, as the node casts its double matrix"""
    x, y, z, w = (np.float64(v) for v in p7[3:])
    n = x * x + y * y + z * z + w * w
    s = 2.0 / n
    m = np.eye(4)
    m[:3, :3] = [[1 - s * (y * y + z * z), s * (x * y - z * w), s * (x * z + y * w)],
                 [s * (x * y + z * w), 1 - s * (x * x + z * z), s * (y * z - x * w)],
                 [s * (x * z - y * w), s * (y * z + x * w), 1 - s * (x * x + y * y)]]
    m[:3, 3] = p7[:3]
    return m.astype(np.float32)


def test_node_render(api, tmp_path):
    import torch
    from densesurfelmapping_amd import msglog, surfel_map, synth
    cam, scene, dfp = synth.NODE_CAM, synth.Scene(), 2
    events = list(synth.node_messages(cam, scene, 12, lap=40, keyframe_every=2))
    log = str(tmp_path / "node.dsmlog")
    msglog.write_log(log, cam, dfp, iter(events))
    node = surfel_map.SurfelMap(cam, drift_free_poses=dfp)
    with pytest.raises(api.DsmError) as e:
        node.render("all")
    assert e.value.code == api.DSM_E_STATE
    last = {}
    node.set_publish(("active",), lambda pub: last.update(pub))
    for ev in events:
        node.feed(ev)
    node.set_publish((), None)
    assert node.frames_fused == 12
    poses = [node.pose(i) for i in range(node.pose_count)]
    attached = [node.attached_surfels(i) for i in range(node.pose_count)]
    local = node.local_surfels()
    inactive = np.concatenate(attached)  # keyframe by keyframe in poses_database order: the mesh's order
    assert len(inactive) > 0 and (local["update_times"] >= 5).any()
    neighbor = [attached[p] for p in _driftfree([pp["links"] for pp in poses], last["relative_index"], 2 * dfp)
                if not poses[p]["is_local"] and poses[p]["n_attached"] > 0]
    seqs = {"active": local[local["update_times"] >= 5], "inactive": inactive,
            "all": np.concatenate([inactive, local[local["update_times"] >= 5]]),
            "neighbor": np.concatenate(neighbor + [local[local["update_times"] != 0]])}
    rcam = api.render_camera(cam)
    view = rc.Camera(70, 37, 60.5, 58.25, 34.3, 18.1, 0.3, 30.0)  # a camera of the caller's own
    fuse_pose = _pose_matrix(last["fuse_pose"])
    aside = fuse_pose.copy()
    aside[:3, 3] -= aside[:3, 2] * np.float32(0.5)  # half a metre back
    for kind, seq in seqs.items():
        for c, p in ((rcam, fuse_pose), (view, aside)):
            got = node.render(kind, camera=c, pose=p)
            assert got["n_surfels"] == len(seq), kind
            rc.same_planes(got, rc.host_render(seq, c, p), (kind, c.width))
            bufs = _device_buffers(api, c)
            assert node.render(kind, camera=c, pose=p, dst_ptrs={k: t.data_ptr() for k, t in bufs.items()}) == len(seq)
            rc.same_planes(_read_device(api, c, bufs, kind), got, (kind, "device"))
    assert (node.render("all", camera=rcam, pose=fuse_pose)["index"] >= 0).mean() > 0.3
    # camera = NULL, pose = NULL: the node's camera at the pose of the latest fuse
    default = node.render("all")
    rc.same_planes(default, rc.host_render(seqs["all"], rcam, fuse_pose), "camera = NULL, pose = NULL")
    rc.same_planes(node.render("all", pose=fuse_pose), default, "camera = NULL")
    rc.same_planes(node.render("all", camera=rcam), default, "pose = NULL")
    # "all" numbers its surfels as get_mesh does
    assert default["n_surfels"] == len(node.get_mesh())
    with pytest.raises(api.DsmError) as e:
        node.render("raw")
    assert e.value.code == api.DSM_E_INVALID
    node.close()
    del torch
    # msglog --render writes the same planes (a process of its own: that is what the command is)
    out = str(tmp_path / "render.npz")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "densesurfelmapping_amd.msglog", log, "--render", out], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["frames_fused"] == 12
    saved = np.load(out)
    rc.same_planes({k: saved[k] for k in api.RENDER_PLANES}, default, "msglog --render")
